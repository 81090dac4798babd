"""`--decode_mode bias_ctc_beam` and `bias_rescore` without a device: the mode table's entries, what Tester.exec() refuses before the checkpoint
is read, with the full message, and what the phrase file reader refuses -- the twin of test_tester_nlm_ctc_settings_cpu.py (a Tester made with
Tester.__new__ that carries only what the settings function reads)."""
from types import SimpleNamespace

import pytest

import masr_amd  # noqa: F401
from masr_amd import bias as bias_module
from masr_amd import tester as tester_module

MODES = ("bias_ctc_beam", "bias_rescore")


def vetted(mode, block, *, model="transformer", head=True, ctx="no/such/phrases.txt", lm_path=None, blank=0):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=lm_path, context_path=ctx)
    t.decode_mode, t.model_name = mode, model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, blank
    return t


def test_mode_table_entries():
    T = tester_module.Tester
    for mode in MODES:
        assert mode in T.MODES and T.MODES[mode][0] is T._bias_ctc_settings and callable(T.MODES[mode][1])
    who = SimpleNamespace(beam_size=7, bias=SimpleNamespace(phrases=31))
    assert T.MODES["bias_ctc_beam"][2](who) == "phrase-biased CTC prefix beam decoding (bias_ctc_beam, beam 7, 31 phrases)"
    assert T.MODES["bias_rescore"][2](who) == "attention rescoring of the phrase-biased CTC beam (bias_rescore, beam 7, 31 phrases)"
    calls = []
    lists = [[([5, 6], -1.0, -0.5, 2), ([5], -2.0, -1.5, 0)], [([], -3.0, -3.0, 0)]]
    stub = SimpleNamespace(beam_size=4, lm=None, bias="PH", bias_weight=3.0, lm_weight=0.0, len_bonus=0.0, nbest=2, att_weight=0.6, ctc_weight=0.4,
                           model_name="transformer",
                           asr_model=SimpleNamespace(bias_ctc_beam_decode=lambda *a: (calls.append(("ctc",) + a), lists)[1],
                                                     bias_rescore_decode=lambda *a: (calls.append(("rs",) + a), lists)[1]))
    stub._ctc_best = lambda l: T._ctc_best(stub, l)
    stub._bias_ctc_beam_lists = lambda xs, il: T._bias_ctc_beam_lists(stub, xs, il)
    assert T.MODES["bias_ctc_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert T.MODES["bias_rescore"][1](stub, "xs", "il") == [[5, 6], []]
    assert calls == [("ctc", "xs", "il", 4, "PH", 3.0, None, 0.0, 0.0), ("rs", "xs", "il", 4, "PH", 3.0, None, 0.0, 0.0, 2, 0.6, 0.4)]
    # the BLSTM's search runs per utterance through ctc_beam_decode, the phrase list in its keyword arguments
    calls.clear()
    stub.model_name, stub.eos_id, stub.lm, stub.lm_weight = "blstm", 12, "LM", 0.3
    stub.trim = lambda h: T.trim(stub, h)
    stub.asr_model = SimpleNamespace(ctc_beam_decode=lambda *a, **kw: (calls.append((a, kw)), lists)[1])
    assert T.MODES["bias_ctc_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert calls == [(("xs", "il", 4, 1, "LM", 0.3, 0.0), dict(bias="PH", bias_weight=3.0))]


def test_the_decode_modes_are_command_line_choices():
    import train
    parser = train.build_parser()
    choices = next(a.choices for a in parser._actions if a.dest == "decode_mode")
    assert set(MODES) <= set(choices) and set(choices) == set(tester_module.Tester.MODES)
    ctx = next(a for a in parser._actions if a.dest == "context_path")
    assert ctx.default is None and "--context_path" in ctx.option_strings


OK = {"beam_size": 4}
NO_CTX = "{}: no phrase list given; pass --context_path (one phrase per line as space-separated unit ids)"
NO_BLOCK = "decode_mode '{}' needs a solver.beam_decode block with at least beam_size in the config"
NO_HEAD = ("decode_mode '{}' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use --decode_mode {}")
BOTH = [
    ("no context path", OK, dict(ctx=None), NotImplementedError, NO_CTX),
    ("no context path, nothing else looked at", None, dict(ctx=None, head=False), NotImplementedError, NO_CTX),
    ("no block", None, {}, ValueError, NO_BLOCK),
    ("beam_size 0", {"beam_size": 0}, {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 0"),
    ("beam_size 65", {"beam_size": 65}, {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 65"),
    ("bias_w negative", dict(OK, bias_w=-0.5), {}, ValueError, "solver.beam_decode.bias_w must be finite and >= 0, got -0.5"),
    ("bias_w nan", dict(OK, bias_w=float("nan")), {}, ValueError, "solver.beam_decode.bias_w must be finite and >= 0, got nan"),
    ("bias_w inf", dict(OK, bias_w=float("inf")), {}, ValueError, "solver.beam_decode.bias_w must be finite and >= 0, got inf"),
    ("lm_w negative with an LM", dict(OK, lm_w=-1.0), dict(lm_path="no/such.arpa"), ValueError, "solver.beam_decode.lm_w must be finite and >= 0, got -1.0"),
    ("len_bonus nan with an LM", dict(OK, len_bonus=float("nan")), dict(lm_path="no/such.arpa"), ValueError,
     "solver.beam_decode.len_bonus must be finite, got nan"),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what,block,kw,exc,msg", BOTH, ids=[b[0] for b in BOTH])
def test_refusals_of_both_modes(mode, what, block, kw, exc, msg):
    with pytest.raises(exc) as e:
        vetted(mode, block, **kw)._bias_ctc_settings()
    assert str(e.value) == msg.format(mode)


def test_refusals_of_one_mode():
    def refused(mode, block, exc, **kw):
        with pytest.raises(exc) as e:
            vetted(mode, block, **kw)._bias_ctc_settings()
        return str(e.value)
    assert refused("bias_ctc_beam", OK, ValueError, head=False) == NO_HEAD.format("bias_ctc_beam", "beam or greedy")
    assert refused("bias_rescore", OK, ValueError, head=False) == NO_HEAD.format("rescore", "beam or greedy")
    assert refused("bias_ctc_beam", OK, ValueError, model="blstm", blank=3) == \
        "decode_mode 'bias_ctc_beam' needs the blank at id 0 (the search never emits class 0), got 3"
    assert refused("bias_rescore", OK, NotImplementedError, model="blstm").startswith("rescore: attention rescoring needs the transformer's decoder")
    assert refused("bias_rescore", dict(OK, nbest=5), ValueError) == "solver.beam_decode.nbest must be in [1, beam_size], got 5"
    assert refused("bias_rescore", dict(OK, ctc_w=1.0), ValueError) == "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"


def test_lm_settings_are_not_read_without_an_lm(tmp_path):
    # without --lm_model_path a bad lm_w is nobody's business: the settings get as far as the phrase file
    t = vetted("bias_ctc_beam", dict(OK, lm_w=-1.0, len_bonus=float("nan")), ctx=str(tmp_path / "missing.txt"))
    with pytest.raises(FileNotFoundError):
        t._bias_ctc_settings()
    assert t.bias_weight == 3.0 and t.lm is None and t.lm_weight == 0.0 and t.len_bonus == 0.0      # WeNet's default weight


def test_phrase_file_reader(tmp_path):
    good = tmp_path / "good.txt"
    good.write_text("3 4 5\n\n  \n7\n3 4\n")
    assert bias_module.read_phrases(good, 13) == [[3, 4, 5], [7], [3, 4]]

    def refused(text, C=13):
        p = tmp_path / "bad.txt"
        p.write_text(text)
        with pytest.raises(ValueError) as e:
            bias_module.ContextBias.from_file(p, C)           # (the reader runs before the library is looked for)
        return str(e.value).replace(str(p), "FILE")
    assert refused("3 4\n5 x 6\n") == "FILE:2: a phrase is a list of unit ids, got '5 x 6'"
    assert refused("3 4\n\n5 12\n") == "FILE:3: unit ids must lie in [1, 11]"
    assert refused("0 4\n") == "FILE:1: unit ids must lie in [1, 11]"
    assert refused("3 4\n-1\n") == "FILE:2: unit ids must lie in [1, 11]"
    assert refused("3 4\n5\n3 4\n") == "FILE:3: duplicate phrase"
    assert refused(" ".join(["3"] * 65) + "\n") == "FILE:1: a phrase holds at most 64 ids, got 65"
    assert refused("\n\n") == "FILE: no phrase"
    with pytest.raises(FileNotFoundError):
        bias_module.ContextBias.from_file(tmp_path / "nothing.txt", 13)


def test_python_side_weight_check():
    with pytest.raises(ValueError, match="bias_w must be finite and >= 0"):
        bias_module.check_bias_args(None, -1.0)
    with pytest.raises(ValueError, match="bias_w must be finite and >= 0"):
        bias_module.check_bias_args(None, float("nan"))
    with pytest.raises(ValueError, match="bias must be a live ContextBias"):
        bias_module.check_bias_args(SimpleNamespace(h=1), 1.0)
