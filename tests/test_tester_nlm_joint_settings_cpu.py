"""`--decode_mode nlm_joint_beam` without a device: the mode table's entry, and what Tester.exec() refuses before the checkpoint is read, with
the full message -- in the stubbed style of test_tester_nlm_settings_cpu.py (a Tester made with Tester.__new__ that carries only what the
settings function reads).  What is raised once the checkpoint is read (the class count) stays with the GPU tests."""
from types import SimpleNamespace

import pytest

import masr_amd  # noqa: F401
from masr_amd import tester as tester_module


def vetted(block, *, model="transformer", head=True, path="no/such/file.pt"):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=path)
    t.decode_mode, t.model_name = "nlm_joint_beam", model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, 0
    return t


def test_mode_table_entry():
    assert "nlm_joint_beam" in tester_module.Tester.MODES
    settings, best, what = tester_module.Tester.MODES["nlm_joint_beam"]
    assert settings is tester_module.Tester._nlm_joint_settings and callable(best)
    assert what(SimpleNamespace(beam_size=7)) == "joint CTC/attention beam decoding with LSTM LM fusion (beam 7)"
    calls = []
    stub = SimpleNamespace(beam_size=4, nlm="LM", lm_weight=0.3, len_bonus=0.5, nbest=2, min_step_ratio=0.1, max_step_ratio=0.9, att_weight=0.6,
                           ctc_weight=0.4,
                           asr_model=SimpleNamespace(nlm_joint_beam_decode=lambda *a: (calls.append(a), [[([5, 6], -1.0), ([5], -2.0)], []])[1]))
    assert best(stub, "xs", "il") == [[5, 6], []]             # the best entry of each list; an empty list writes an empty hypothesis
    assert calls == [("xs", "il", 4, "LM", 0.3, 0.5, 2, 0.1, 0.9, 0.6, 0.4)]


def test_the_decode_mode_is_a_command_line_choice():
    import train
    choices = next(a.choices for a in train.build_parser()._actions if a.dest == "decode_mode")
    assert "nlm_joint_beam" in choices and set(choices) == set(tester_module.Tester.MODES)


OK = {"beam_size": 4, "ctc_w": 0.3}
NO_BLOCK = "decode_mode 'nlm_joint_beam' needs a solver.beam_decode block with at least beam_size in the config"
NO_PATH = "nlm_joint_beam: no language model given; pass --lm_model_path (a torch checkpoint of an LSTM LM over the output units)"
NO_CTC_W = ("nlm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LSTM LM into the attention beam alone use "
            "--decode_mode nlm_beam")
EXPECTED = [
    ("no path", OK, dict(path=None), NotImplementedError, NO_PATH),
    ("no path + blstm + no block", None, dict(path=None, model="blstm"), NotImplementedError, NO_PATH),
    ("blstm", OK, dict(model="blstm"), NotImplementedError,
     "nlm_joint_beam: the joint CTC/attention beam needs the transformer's decoder, the BLSTM has none; use --decode_mode ctc_beam or greedy"),
    ("no block", None, {}, ValueError, NO_BLOCK),
    ("block without beam_size", {"ctc_w": 0.3}, {}, ValueError, NO_BLOCK),
    ("beam_size 0", dict(OK, beam_size=0), {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 0"),
    ("beam_size 65", dict(OK, beam_size=65), {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 65"),
    ("no CTC head", OK, dict(head=False), ValueError,
     "decode_mode 'nlm_joint_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
     "use --decode_mode nlm_beam, beam or greedy"),
    ("ctc_w absent", {"beam_size": 4}, {}, ValueError, NO_CTC_W),
    ("ctc_w 0", dict(OK, ctc_w=0.0), {}, ValueError, NO_CTC_W),
    ("ctc_w -1", dict(OK, ctc_w=-1.0), {}, ValueError, "solver.beam_decode.ctc_w must be finite and >= 0, got -1.0"),
    ("ctc_w 1.5 without att_w", dict(OK, ctc_w=1.5), {}, ValueError, "solver.beam_decode.att_w must be finite and >= 0, got -0.5"),
    ("att_w inf", dict(OK, att_w=float("inf")), {}, ValueError, "solver.beam_decode.att_w must be finite and >= 0, got inf"),
    ("lm_w -0.5", dict(OK, lm_w=-0.5), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got -0.5"),
    ("lm_w nan", dict(OK, lm_w=float("nan")), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got nan"),
    ("len_bonus inf", dict(OK, len_bonus=float("inf")), {}, ValueError, "solver.beam_decode.len_bonus must be finite, got inf"),
    ("len_bonus nan", dict(OK, len_bonus=float("nan")), {}, ValueError, "solver.beam_decode.len_bonus must be finite, got nan"),
    ("nbest 0", dict(OK, nbest=0), {}, ValueError, "solver.beam_decode.nbest must be in [1, beam_size], got 0"),
    ("nbest 5", dict(OK, nbest=5), {}, ValueError, "solver.beam_decode.nbest must be in [1, beam_size], got 5"),
    ("lm_start bos", dict(OK, lm_start="bos"), {}, ValueError, "solver.beam_decode.lm_start must be sos or eos, got 'bos'"),
]


@pytest.mark.parametrize("label, block, kw, exc, text", EXPECTED, ids=[e[0] for e in EXPECTED])
def test_refusals_before_the_checkpoint_is_read(label, block, kw, exc, text):
    with pytest.raises(exc) as e:
        vetted(block, **kw).exec()
    assert str(e.value) == text


@pytest.mark.parametrize("block", [OK, dict(OK, att_w=0.0), dict(OK, ctc_w=1.0), dict(OK, lm_w=0.0, len_bonus=-0.5, nbest=4), dict(OK, lm_start="eos")])
def test_valid_settings_get_as_far_as_the_checkpoint(block):
    """everything before the file is accepted: the first complaint is the missing file's"""
    t = vetted(block)
    with pytest.raises(FileNotFoundError):
        t.exec()
    assert t.ctc_weight == block["ctc_w"] and t.att_weight == pytest.approx(block.get("att_w", 1.0 - block["ctc_w"]))
    assert (t.lm_weight, t.len_bonus, t.nbest) == (block.get("lm_w", 0.3), block.get("len_bonus", 0.0), block.get("nbest", 1))


def test_nlm_beam_still_refuses_the_joint_weight_and_says_where_to_go():
    """nlm_beam's refusal of ctc_w > 0 on a hybrid model is unchanged; the module's documentation names the mode that takes it"""
    t = vetted(dict(OK))
    t.decode_mode = "nlm_beam"
    with pytest.raises(ValueError, match="nlm_beam: the LSTM LM is not fused into the joint CTC/attention beam"):
        t.exec()
    doc = tester_module.__doc__
    assert "nlm_joint_beam" in doc and "masr_recog_beam_ctc_nlm" in doc
