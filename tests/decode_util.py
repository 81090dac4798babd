"""Shared by the decoder tests (test_hip_beam.py, test_hip_joint_beam.py, test_hip_ctc_beam_decode.py): the peaked toy models and the
Tester set-up.  A plain helper module like beam_ref.py: no fixtures, no tests."""
from types import SimpleNamespace

import torch

import hybrid_ref
from masr_amd.engine import MasrEngine
from oracle import ref_cpu
from oracle.make_goldens import BLSTM_TINY, ODIM, write_toy_shard
from test_hip_fomaml import make_run

# 12 classes and an output projection scaled by 10: log-probabilities that spread like a trained model's (the reasoning: test_hip_beam.py)
C_SMALL, OUT_SCALE = 12, 10.0


def peaked_state_dict(cfg, seed):
    sd = ref_cpu.deterministic_state_dict(cfg, C_SMALL, seed=seed)
    sd["char_trans.weight"] = sd["char_trans.weight"] * OUT_SCALE
    if "pre_embed.weight" in sd:
        sd["pre_embed.weight"] = sd["char_trans.weight"]
    return sd


# The peaked model plus a CTC head (hybrid_ref.with_head) scaled by HEAD_SCALE so that its log-probs spread.  The random decoder prefers
# token 0 (sos, which is also the CTC blank and never a joint candidate); its bias is lowered so that the attention term ranks real tokens.
# Tolerances: the joint score carries the CTC prefix score, a log-sum over T_b frames of the head's log-probs.  The engine's encoder
# memory differs from the restatement's by bf16-level rounding (test_hip_beam), and the scaled head turns that into ~1e-2 nats per
# frame of log-prob: measured score differences reach 0.08 nats at -2.7 on TINY and 0.2 nats at -90 on hkust geometry.  So JOINT_DELTA is
# 0.05 nats (test_hip_beam: 0.02) and the score tolerance 0.1 + 3e-3 |score|; a near-tie under that noise can swap a hypothesis, so only
# utterances whose every decision gap exceeds JOINT_DELTA are compared, and the count that qualifies is checked over all weight pairs.
JOINT_DELTA = 0.05
HEAD_SCALE = 6.0


def joint_state_dict(cfg, seed):
    sd = hybrid_ref.with_head(peaked_state_dict(cfg, seed), C_SMALL, seed=seed + 100)
    sd[hybrid_ref.HEAD[0]] = sd[hybrid_ref.HEAD[0]] * HEAD_SCALE
    sd["char_trans.bias"] = sd["char_trans.bias"].clone()
    sd["char_trans.bias"][0] = -30.0
    return sd


def joint_engine(cfg, sd, C=C_SMALL):
    e = MasrEngine(dict(cfg, ctc_weight=0.3), C)
    e.load_state_dict(sd)
    return e


def make_tester(tmp_path, monkeypatch, mode, beam_decode=None, *, model_name="transformer", hybrid=False, blstm_sd=None, resume=False, bs=4, suffix=None):
    """A Tester in `mode` over six toy test utterances and a deterministic checkpoint under tmp_path -> (Tester, log_dir, state dict, cfg).
    The TINY transformer of make_run (hybrid: with a CTC head), or, where blstm_sd is given, BLSTM_TINY with that state dict."""
    from masr_amd.tester import Tester
    monkeypatch.chdir(tmp_path)
    data = tmp_path / "data"
    if blstm_sd is None:
        cfg, paras, id2accent = make_run(tmp_path)
        if hybrid:
            cfg["asr_model"]["ctc_weight"] = 0.3
        paras.accent, paras.eval_suffix, paras.pretrain_suffix, paras.algo = "af", "ev", None, "no"
        paras.test_model, paras.decode_batch_size, paras.model_name, paras.overwrite = "model.wer.best", bs, model_name, True
        sd = ref_cpu.deterministic_state_dict(cfg["asr_model"], ODIM, seed=7)
        if hybrid:
            sd = hybrid_ref.with_head(sd, ODIM, seed=3)
    else:
        data.mkdir(exist_ok=True)
        (data / "units.txt").write_text("".join(f"u{i} {i}\n" for i in range(1, 366)))
        cfg = {"asr_model": dict(BLSTM_TINY), "solver": {"setting": "gold", "data_root": str(data), "spm_mapping": str(data / "units.txt"),
                                                         "spm_model": "unused"}}
        paras = SimpleNamespace(accent="af", algo="no", pretrain_suffix=None, eval_suffix="ev", runs=0, model_name="blstm", test_model="model.wer.best",
                                decode_batch_size=bs, njobs=1, overwrite=True, is_memmap=True, device="cuda:0")
        id2accent, sd = {"af": "african"}, blstm_sd
    if beam_decode is not None:
        cfg["solver"]["beam_decode"] = beam_decode
    if not (data / "african" / "test").exists():
        write_toy_shard(data, "african", "test", 6, seed=300)
    paras.decode_suffix, paras.decode_mode, paras.resume = suffix or f"{mode}_decode", mode, resume
    log_dir = tmp_path / "testing-logs" / "evaluation" / "gold" / "no" / "ev" / "ev" / "african" / "0"
    log_dir.mkdir(parents=True, exist_ok=True)
    torch.save(sd, log_dir / "model.wer.best")
    return Tester(cfg, paras, id2accent), log_dir, sd, cfg
