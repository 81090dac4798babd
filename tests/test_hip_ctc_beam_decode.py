"""CTC prefix beam decoding through the models: BlstmEngine.ctc_beam / MonoBLSTM.ctc_beam_decode, MasrEngine.recog_ctc_beam /
MyTransformer.ctc_beam_decode (masr_recog_ctc_beam) and the Tester's `ctc_beam` mode, against the restatement of tests/ctc_beam_ref.py.

Both models are checked on the fp32 logits the search itself read -- the BLSTM's last_logits(), the hybrid transformer's head logits in
the workspace (include/masr_test.h masr_test_ctc_beam_logits) -- so no encoder noise enters and the rule is the kernel test's: an
utterance is compared where the restatement's slack is positive, there the N-best token lists are equal and the scores within
1e-4 + 2e-5 |s|, and at most a quarter of the utterances may be left out.  The BLSTM's head is scaled so that the tiny random model's rows
spread; scale and batches were picked on the CPU oracle's logits (oracle.blstm_cpu), where every utterance qualifies at every K used."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_beam_ref as cr  # noqa: E402
import hybrid_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.blstm_engine import BlstmEngine  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import blstm_cpu, ref_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, ODIM, TINY, synth_batch  # noqa: E402
from decode_util import JOINT_DELTA as ENC_DELTA  # noqa: E402
from decode_util import C_SMALL, joint_engine, joint_state_dict, make_tester  # noqa: E402

BLSTM_HEAD_SCALE = 30.0
BLSTM_BATCHES = ((22, [57, 57, 44, 12]), (24, [36, 28, 20, 13]))


def _blstm_sd(scale=BLSTM_HEAD_SCALE):
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    sd["head.weight"] = sd["head.weight"] * scale
    return sd


@pytest.mark.parametrize("K,nbest", [(1, 1), (4, 2), (8, 1)])
def test_blstm_ctc_beam_vs_restatement(K, nbest):
    eng = BlstmEngine(BLSTM_TINY, ODIM)
    eng.load_state_dict(_blstm_sd())
    ok = total = 0
    for seed, ilens in BLSTM_BATCHES:
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        got = eng.ctc_beam(xs, il, K, nbest)
        logits, lens = eng.last_logits()                         # the forward ctc_beam ran
        rs = cr.ctc_beam_ref_batch(logits.cpu().numpy(), lens.cpu().tolist(), K, 0, ODIM - 1, nbest)
        for b, r in enumerate(rs):
            total += 1
            assert all(0 < t < ODIM - 1 for hyp, _ in got[b] for t in hyp)
            print(f"blstm K={K} seed={seed} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} best {got[b][0]}")
            if not r["slack"] > 0:
                continue
            ok += 1
            assert len(got[b]) == len(r["nbest"])
            for (hyp, s), (pre, want) in zip(got[b], r["nbest"]):
                assert tuple(hyp) == pre and abs(s - want) <= cr.tol(want), (K, seed, b, hyp, pre, s, want)
    assert 4 * (total - ok) <= total, (ok, total)


def test_hybrid_ctc_beam_vs_restatement_and_plain_model_errors():
    sd = joint_state_dict(TINY, 7)
    eng = joint_engine(TINY, sd)
    for K, nbest in ((1, 1), (4, 3), (20, 3)):
        ok = total = 0
        for seed, ilens in ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60])):
            xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
            B, T = xs.shape[0], xs.shape[1]
            got = eng.recog_ctc_beam(xs, il, K, nbest)
            logits, lens = eng.last_ctc_beam_logits(B, T, K)       # what the search read: head logits [B][T/4][Cp], enc_lens
            assert lens.cpu().tolist() == [n // 4 for n in ilens] and logits.shape[1] == T // 4 and logits.shape[2] >= C_SMALL
            z = logits[..., :C_SMALL].cpu().numpy()
            rs = cr.ctc_beam_ref_batch(z, lens.cpu().tolist(), K, 0, C_SMALL - 1, nbest)
            for b, r in enumerate(rs):
                total += 1
                assert all(0 < t < C_SMALL - 1 for hyp, _ in got[b] for t in hyp)
                print(f"hybrid K={K} seed={seed} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} got {got[b][0]} want {r['nbest'][0]}")
                if not r["slack"] > 0:
                    continue
                ok += 1
                assert len(got[b]) == len(r["nbest"]), (K, seed, b, got[b], r["nbest"])
                for (hyp, s), (pre, want) in zip(got[b], r["nbest"]):
                    assert tuple(hyp) == pre and abs(s - want) <= cr.tol(want), (K, seed, b, hyp, pre, s, want)
        assert 4 * (total - ok) <= total, (K, ok, total)
    xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
    # a plain model has no CTC head
    plain = MasrEngine(TINY, C_SMALL)
    l = lib()
    assert l.masr_ctc_beam_workspace_bytes(plain.h, 4, 64, 4) < 0 and b"no CTC head" in l.masr_last_error()
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_ctc_beam(xs, il, 4)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        eng.recog_ctc_beam(xs, il, 65)
    with pytest.raises(ValueError, match="nbest"):
        eng.recog_ctc_beam(xs, il, 4, 5)


def _blstm_tester(tmp_path, monkeypatch, mode, bs, beam_decode, resume=False):
    return make_tester(tmp_path, monkeypatch, mode, beam_decode, blstm_sd=_blstm_sd(), bs=bs, resume=resume)[:2]


def _joint_tester(tmp_path, monkeypatch, beam_decode, hybrid, **kw):
    return make_tester(tmp_path, monkeypatch, "beam", beam_decode, hybrid=hybrid, **kw)


def _run(t):
    t.load_data(); t.set_model(); t.exec()


def test_tester_blstm_ctc_beam(tmp_path, monkeypatch):
    t, log_dir = _blstm_tester(tmp_path, monkeypatch, "ctc_beam", 4, {"beam_size": 8})
    _run(t)
    hyp_file = log_dir / "ctc_beam_decode" / "best-hyp"
    full = hyp_file.read_text()
    lines = full.splitlines()
    assert len(lines) == 6 and all("\t" in l for l in lines)
    assert any(l.split("\t")[1] for l in lines)
    for l in lines:
        assert all(0 < int(x) < ODIM - 1 for x in l.split("\t")[1].split())
    for keep in (5, 1):                                          # --resume after a cut file
        hyp_file.write_text("".join(l + "\n" for l in lines[:keep]))
        t2, _ = _blstm_tester(tmp_path, monkeypatch, "ctc_beam", 4, {"beam_size": 8}, resume=True)
        assert t2.prev_decode_step == keep
        _run(t2)
        assert hyp_file.read_text() == full, f"resume after {keep} lines"
    for bad, pat in ((None, "beam_decode"), ({"beam_size": 0}, r"\[1, 64\]"), ({"beam_size": 65}, r"\[1, 64\]")):
        t, _ = _blstm_tester(tmp_path, monkeypatch, "ctc_beam", 4, bad)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match=pat):
            t.exec()
    t, _ = _blstm_tester(tmp_path, monkeypatch, "beam", 4, {"beam_size": 8})          # `beam` keeps its meaning for the BLSTM
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="transformer"):
        t.exec()


def test_tester_blstm_ctc_beam_lines_do_not_depend_on_the_batch_size(tmp_path, monkeypatch):
    """The lines of batch size 4 and batch size 1 are exactly equal (the loader's order of the utterances depends on the batch size, so
    they are compared as sorted lists).  The search is batch-independent (test_hip_ctc_beam_kernel.py::test_permuted_batch_bit_for_bit);
    the BLSTM's logits in a padded batch are not (the VGG front end reads the padded frames: for synth_batch(21, [61, 50, 38, 30]) the three
    padded utterances' logits moved by up to 0.24 at a head scale of 8, the longest one's not at all), which is why
    MonoBLSTM.ctc_beam_decode runs every utterance alone at its own length.  The last assertions pin both halves of that."""
    t, log_dir = _blstm_tester(tmp_path, monkeypatch, "ctc_beam", 4, {"beam_size": 8})
    _run(t)
    hyp_file = log_dir / "ctc_beam_decode" / "best-hyp"
    lines4 = hyp_file.read_text().splitlines()
    t, _ = _blstm_tester(tmp_path, monkeypatch, "ctc_beam", 1, {"beam_size": 8})
    _run(t)
    assert sorted(hyp_file.read_text().splitlines()) == sorted(lines4)
    # the model's decode of a padded batch is each utterance's decode alone, bit for bit
    xs, il, _, _ = synth_batch(21, [61, 50, 38, 30], [3] * 4)
    got = t.asr_model.ctc_beam_decode(xs, il, 8, 2)
    eng = t.asr_model.engine
    batch = eng.forward(xs, il)[0].cpu().clone()
    moved = []
    for b in range(4):
        n = int(il[b])
        assert got[b] == eng.ctc_beam(xs[b:b + 1, :n], il[b:b + 1], 8, 2)[0]
        alone, ln = eng.last_logits()
        moved.append(float((alone[0, :int(ln[0])].cpu() - batch[b, :int(ln[0])]).abs().max()))
    print("max |logit alone - logit in the padded batch| per utterance:", moved)
    assert moved[0] == 0.0 and max(moved[1:]) > 1e-3             # the unpadded utterance is bit-identical, padded ones are not


def test_tester_transformer_ctc_beam(tmp_path, monkeypatch):
    def tester(bs, hybrid=True, block={"beam_size": 8}):
        t, log_dir, sd, cfg = _joint_tester(tmp_path, monkeypatch, block, hybrid=hybrid, bs=bs, suffix="ctc_beam_decode")
        t.decode_mode = t.paras.decode_mode = "ctc_beam"
        return t, log_dir, sd, cfg
    t, log_dir, sd, cfg = tester(4)
    _run(t)
    hyp_file = log_dir / "ctc_beam_decode" / "best-hyp"
    lines4 = hyp_file.read_text().splitlines()
    assert len(lines4) == 6
    for l in lines4:
        assert all(0 < int(x) < ODIM - 1 for x in l.split("\t")[1].split())
    # the lines are what the engine gives on the Tester's own batches
    eng = MasrEngine(cfg["asr_model"], ODIM)
    eng.load_state_dict(sd)
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        want += ["{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(str(v) for v in n[0][0])) for n, y in zip(eng.recog_ctc_beam(xs, il, 8), ys)]
    assert lines4 == want
    # batch size 1: the encoder's GEMMs tile by row count, so a line may differ where the restatement on the oracle's log-probs has a
    # decisive gap below the encoder tolerance of test_hip_joint_beam.py
    t1, _, _, _ = tester(1)
    _run(t1)
    lines1 = hyp_file.read_text().splitlines()
    by_ref = dict(l.split("\t") for l in lines4)                # (the loader's order of the utterances depends on the batch size)
    assert len(lines1) == 6 and len(by_ref) == 6 and sorted(l.split("\t")[0] for l in lines1) == sorted(by_ref)
    p = hybrid_ref.leafify(sd, cfg["asr_model"])
    n = 0
    for idxs in t1.eval_set.iter_indices():
        xs, il, _, _ = t1.eval_set.materialize(idxs)
        with ref_cpu.bf16_emulation(), torch.no_grad():
            lp, el = hybrid_ref.ctc_log_probs(p, cfg["asr_model"], xs, il)
        r = cr.ctc_beam_ref(np.ascontiguousarray(lp[:int(el[0]), 0].numpy().astype(np.float32)), 8, 0, ODIM - 1, 1)
        ref, hyp = lines1[n].split("\t")
        print(f"utterance {n}: min_gap {r['min_gap']:.3g} bs1 '{hyp}' bs4 '{by_ref[ref]}'")
        if r["min_gap"] > ENC_DELTA:
            assert hyp == by_ref[ref], n
        n += 1
    # a plain transformer has no CTC output layer; beam_size is vetted as for `beam`
    t, _, _, _ = tester(4, hybrid=False)
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="asr_model.ctc_weight"):
        t.exec()
    t, _, _, _ = tester(4, block={"beam_size": 100})
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        t.exec()
