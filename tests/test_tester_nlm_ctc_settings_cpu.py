"""`--decode_mode nlm_ctc_beam` and `nlm_rescore` without a device: the mode table's entries, and what Tester.exec() refuses before the
checkpoint is read, with the full message -- the twin of test_tester_nlm_joint_settings_cpu.py (a Tester made with Tester.__new__ that
carries only what the settings function reads).  What is raised once the checkpoint is read (the class count) stays with the GPU tests."""
from types import SimpleNamespace

import pytest

import masr_amd  # noqa: F401
from masr_amd import tester as tester_module

MODES = ("nlm_ctc_beam", "nlm_rescore")


def vetted(mode, block, *, model="transformer", head=True, path="no/such/file.pt", blank=0):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=path)
    t.decode_mode, t.model_name = mode, model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, blank
    return t


def test_mode_table_entries():
    T = tester_module.Tester
    for mode in MODES:
        assert mode in T.MODES and T.MODES[mode][0] is T._nlm_ctc_settings and callable(T.MODES[mode][1])
    assert T.MODES["nlm_ctc_beam"][2](SimpleNamespace(beam_size=7)) == "LSTM-LM-fused CTC prefix beam decoding (beam 7)"
    assert T.MODES["nlm_rescore"][2](SimpleNamespace(beam_size=7)) == "attention rescoring of the LSTM-LM-fused CTC beam (beam 7)"
    calls = []
    lists = [[([5, 6], -1.0, -0.5), ([5], -2.0, -1.5)], [([], -3.0, -3.0)]]
    stub = SimpleNamespace(beam_size=4, nlm="LM", lm_weight=0.3, len_bonus=0.5, nbest=2, att_weight=0.6, ctc_weight=0.4, model_name="transformer",
                           asr_model=SimpleNamespace(nlm_ctc_beam_decode=lambda *a: (calls.append(("ctc",) + a), lists)[1],
                                                     nlm_rescore_decode=lambda *a: (calls.append(("rs",) + a), lists)[1]))
    stub._ctc_best = lambda l: T._ctc_best(stub, l)
    stub._nlm_ctc_beam_lists = lambda xs, il: T._nlm_ctc_beam_lists(stub, xs, il)
    assert T.MODES["nlm_ctc_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert T.MODES["nlm_rescore"][1](stub, "xs", "il") == [[5, 6], []]
    assert calls == [("ctc", "xs", "il", 4, "LM", 0.3, 0.5), ("rs", "xs", "il", 4, "LM", 0.3, 0.5, 2, 0.6, 0.4)]
    # the BLSTM's search runs per utterance through ctc_beam_decode, the LM in the n-gram's argument
    calls.clear()
    stub.model_name, stub.eos_id = "blstm", 12
    stub.trim = lambda h: T.trim(stub, h)
    stub.asr_model = SimpleNamespace(ctc_beam_decode=lambda *a: (calls.append(a), lists)[1])
    assert T.MODES["nlm_ctc_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert calls == [("xs", "il", 4, 1, "LM", 0.3, 0.5)]


def test_the_decode_modes_are_command_line_choices():
    import train
    choices = next(a.choices for a in train.build_parser()._actions if a.dest == "decode_mode")
    assert set(MODES) <= set(choices) and set(choices) == set(tester_module.Tester.MODES)


OK = {"beam_size": 4}
NO_PATH = "{}: no language model given; pass --lm_model_path (a torch checkpoint of an LSTM LM over the output units)"
NO_BLOCK = "decode_mode '{}' needs a solver.beam_decode block with at least beam_size in the config"
NO_HEAD = ("decode_mode '{}' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use --decode_mode {}")
BOTH = [
    ("no path", OK, dict(path=None), NotImplementedError, NO_PATH),
    ("no path + no block", None, dict(path=None), NotImplementedError, NO_PATH),
    ("no block", None, {}, ValueError, NO_BLOCK),
    ("block without beam_size", {"lm_w": 0.3}, {}, ValueError, NO_BLOCK),
    ("beam_size 0", dict(OK, beam_size=0), {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 0"),
    ("beam_size 65", dict(OK, beam_size=65), {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 65"),
    ("lm_w -0.5", dict(OK, lm_w=-0.5), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got -0.5"),
    ("lm_w nan", dict(OK, lm_w=float("nan")), {}, ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got nan"),
    ("len_bonus inf", dict(OK, len_bonus=float("inf")), {}, ValueError, "solver.beam_decode.len_bonus must be finite, got inf"),
    ("len_bonus nan", dict(OK, len_bonus=float("nan")), {}, ValueError, "solver.beam_decode.len_bonus must be finite, got nan"),
    ("lm_start bos", dict(OK, lm_start="bos"), {}, ValueError, "solver.beam_decode.lm_start must be sos or eos, got 'bos'"),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label, block, kw, exc, text", BOTH, ids=[e[0] for e in BOTH])
def test_refusals_before_the_checkpoint_is_read(mode, label, block, kw, exc, text):
    with pytest.raises(exc) as e:
        vetted(mode, block, **kw).exec()
    assert str(e.value) == text.format(mode)


def test_refusals_by_model():
    with pytest.raises(ValueError) as e:
        vetted("nlm_ctc_beam", OK, head=False).exec()
    assert str(e.value) == NO_HEAD.format("nlm_ctc_beam", "nlm_beam, beam or greedy")
    with pytest.raises(ValueError) as e:
        vetted("nlm_rescore", OK, head=False).exec()
    assert str(e.value) == NO_HEAD.format("rescore", "beam or greedy")
    with pytest.raises(NotImplementedError) as e:
        vetted("nlm_rescore", OK, model="blstm").exec()
    assert str(e.value) == ("rescore: attention rescoring needs the transformer's decoder, the BLSTM has none; use --decode_mode ctc_beam or greedy")
    with pytest.raises(ValueError) as e:
        vetted("nlm_ctc_beam", OK, model="blstm", blank=3).exec()
    assert str(e.value) == "decode_mode 'nlm_ctc_beam' needs the blank at id 0 (the search never emits class 0), got 3"
    with pytest.raises(FileNotFoundError):                    # a BLSTM with the blank at id 0 is allowed: the next complaint is the file's
        vetted("nlm_ctc_beam", OK, model="blstm").exec()


RESCORE_ONLY = [
    ("nbest 0", dict(OK, nbest=0), "solver.beam_decode.nbest must be in [1, beam_size], got 0"),
    ("nbest 5", dict(OK, nbest=5), "solver.beam_decode.nbest must be in [1, beam_size], got 5"),
    ("ctc_w -1", dict(OK, ctc_w=-1.0), "solver.beam_decode.ctc_w must be finite and >= 0, got -1.0"),
    ("att_w 0", dict(OK, att_w=0.0), "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
    ("ctc_w 1 without att_w", dict(OK, ctc_w=1.0), "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
]


@pytest.mark.parametrize("label, block, text", RESCORE_ONLY, ids=[e[0] for e in RESCORE_ONLY])
def test_nlm_rescore_vets_the_rescoring_settings(label, block, text):
    with pytest.raises(ValueError) as e:
        vetted("nlm_rescore", block).exec()
    assert str(e.value) == text


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", [OK, dict(OK, lm_w=0.0, len_bonus=-0.5), dict(OK, lm_start="eos"), dict(OK, nbest=3, ctc_w=0.25)])
def test_valid_settings_get_as_far_as_the_checkpoint(mode, block):
    """everything before the file is accepted: the first complaint is the missing file's"""
    t = vetted(mode, block)
    with pytest.raises(FileNotFoundError):
        t.exec()
    assert (t.lm_weight, t.len_bonus, t.beam_size) == (block.get("lm_w", 0.3), block.get("len_bonus", 0.0), 4)
    if mode == "nlm_rescore":
        ctc_w = block.get("ctc_w", 0.5)
        assert (t.nbest, t.ctc_weight) == (block.get("nbest", 4), ctc_w) and t.att_weight == pytest.approx(1.0 - ctc_w)


def test_the_documentation_names_the_modes():
    doc = tester_module.__doc__
    for word in MODES + ("masr_recog_ctc_beam_nlm", "masr_recog_rescore_nlm", "masr_ctc_beam_search_nlm"):
        assert word in doc
