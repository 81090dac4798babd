"""`--decode_mode nlm_beam` without a device: the mode table's entry, and what Tester.exec() refuses before the checkpoint is read, with the
full message -- in the stubbed style of test_tester_settings_cpu.py (a Tester made with Tester.__new__ that carries only what the settings
function reads).  What is raised once the checkpoint is read stays with the GPU tests, except the reader's own refusal of a file that is no
LSTM LM, which needs no device."""
from types import SimpleNamespace

import pytest
import torch

import masr_amd  # noqa: F401
from masr_amd import tester as tester_module


def vetted(block, *, model="transformer", head=True, path="no/such/file.pt"):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=path)
    t.decode_mode, t.model_name = "nlm_beam", model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, 0
    return t


def test_mode_table_entry():
    assert "nlm_beam" in tester_module.Tester.MODES
    settings, best, what = tester_module.Tester.MODES["nlm_beam"]
    assert settings is tester_module.Tester._nlm_beam_settings and callable(best)
    assert what(SimpleNamespace(beam_size=7)) == "beam decoding with LSTM LM fusion (beam 7)"
    calls = []
    stub = SimpleNamespace(beam_size=4, nlm="LM", lm_weight=0.3, min_step_ratio=0.1, max_step_ratio=0.9,
                           asr_model=SimpleNamespace(nlm_beam_decode=lambda *a: (calls.append(a), (["hyp"], None))[1]))
    assert best(stub, "xs", "il") == ["hyp"] and calls == [("xs", "il", 4, "LM", 0.3, 0.1, 0.9)]


OK = {"beam_size": 4}
NO_BLOCK = "decode_mode 'nlm_beam' needs a solver.beam_decode block with at least beam_size in the config"
EXPECTED = [
    ("no path", OK, dict(path=None), NotImplementedError,
     "nlm_beam: no language model given; pass --lm_model_path (a torch checkpoint of an LSTM LM over the output units)"),
    ("no path + blstm + no block", None, dict(path=None, model="blstm"), NotImplementedError,
     "nlm_beam: no language model given; pass --lm_model_path (a torch checkpoint of an LSTM LM over the output units)"),
    ("blstm", OK, dict(model="blstm"), NotImplementedError,
     "nlm_beam: LM fusion is only implemented for the transformer's attention beam; use --decode_mode ctc_beam or greedy"),
    ("no block", None, {}, ValueError, NO_BLOCK),
    ("block without beam_size", {"lm_w": 0.3}, {}, ValueError, NO_BLOCK),
    ("beam_size 0", {"beam_size": 0}, {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 0"),
    ("beam_size 65", {"beam_size": 65}, {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 65"),
    ("lm_w -0.5", dict(OK, lm_w=-0.5), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got -0.5"),
    ("lm_w nan", dict(OK, lm_w=float("nan")), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got nan"),
    ("lm_w inf", dict(OK, lm_w=float("inf")), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got inf"),
    ("lm_start bos", dict(OK, lm_start="bos"), {}, ValueError, "solver.beam_decode.lm_start must be sos or eos, got 'bos'"),
    ("ctc_w -1", dict(OK, ctc_w=-1.0), {}, ValueError, "solver.beam_decode.ctc_w must be finite and >= 0, got -1.0"),
    ("ctc_w 0.3 on a hybrid model", dict(OK, ctc_w=0.3), {}, ValueError,
     "nlm_beam: the LSTM LM is not fused into the joint CTC/attention beam (beam_decode.ctc_w = 0.3); set beam_decode.ctc_w: 0 to fuse it into the "
     "attention beam, or use --decode_mode beam without an LM"),
    ("ctc_w 0.3 on a hybrid model + lm_w -1", dict(OK, ctc_w=0.3, lm_w=-1.0), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got -1.0"),
]


@pytest.mark.parametrize("label, block, kw, exc, text", EXPECTED, ids=[e[0] for e in EXPECTED])
def test_refusals_before_the_checkpoint_is_read(label, block, kw, exc, text):
    with pytest.raises(exc) as e:
        vetted(block, **kw).exec()
    assert str(e.value) == text


@pytest.mark.parametrize("block, head", [(OK, True), (dict(OK, ctc_w=0.0), True), (dict(OK, ctc_w=0.3), False), (dict(OK, lm_start="eos"), True)])
def test_valid_settings_get_as_far_as_the_checkpoint(block, head):
    """everything before the file is accepted: the first complaint is the missing file's"""
    with pytest.raises(FileNotFoundError):
        vetted(block, head=head).exec()


def test_a_checkpoint_that_is_no_lstm_lm_is_refused_by_name(tmp_path):
    path = tmp_path / "other.pt"
    torch.save({"embed.weight": torch.zeros(13, 4), "lo.weight": torch.zeros(13, 4)}, path)
    with pytest.raises(ValueError, match="missing keys") as e:
        vetted(OK, path=str(path)).exec()
    assert "lo.bias" in str(e.value) and "rnn.weight_ih_l0" in str(e.value)
