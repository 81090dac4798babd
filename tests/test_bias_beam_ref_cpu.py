"""The CPU restatement of the phrase-biased attention and joint beams (tests/bias_beam_ref.py) against independent facts: at
bias_w = 0 it is lm_ref's / joint_lm_beam_ref's search, the bound stop rule gives what the search run to maxlen gives, each rule of the
contract matters (a mutated restatement differs somewhere), and the cases tests/test_hip_bias_beam.py compares on the GPU are fit for that.
Also the settings of Tester's bias_beam / bias_joint_beam modes without a device.  CPU only.

The old stop rule.  On the toy models no case was found where today's rule (best ended >= best running) loses the best hypothesis: their
running scores never dip below an ended one and recover (the attention model repeats one token, the joint searches end within a step or two of
maxlen).  The rule's failure needs exactly that -- a stretch of unrewarded tokens and a phrase behind it -- so it is shown on a scripted
decoder: beam_ref.last_logits replaced by a table in which every token costs 0.97 nats, eos 0.47 nats, and the phrase starts at the third token."""
import math
from types import SimpleNamespace

import pytest
import torch

import masr_amd  # noqa: F401
import beam_ref
import bias_beam_ref as bb
import bias_ref
import joint_lm_beam_ref as jl
import lm_ref
from decode_util import JOINT_DELTA
from masr_amd import tester as tester_module
from oracle import ref_cpu

ALL = [("att", n) for n in bb.ATT_CASES] + [("joint", n) for n in bb.JOINT_CASES_ALL]
GPU = [("att", n) for n in bb.ATT_CASES] + [("joint", n) for n in bb.JOINT_CASES]


def key(r):
    return (r["nbest"] if "nbest" in r else r["tokens"], r["score"], r["nbias"])


def differs(kind, name, **kw):
    return sum(key(a) != key(b) for a, b in zip(bb.case_results(kind, name), bb.case_results(kind, name, **kw)))


@pytest.mark.parametrize("kind, name", ALL)
def test_the_stop_rule_gives_the_search_run_to_maxlen(kind, name):
    got, full = bb.case_results(kind, name), bb.case_results(kind, name, stop=False)
    assert [key(r) for r in got] == [key(r) for r in full]
    assert all(a["steps"] <= b["steps"] for a, b in zip(got, full))


def test_bias_weight_zero_is_the_unbiased_restatement():
    m = bb._models()
    cs = bb.make_case("att", "k4_lm")
    with ref_cpu.bf16_emulation():
        want = [r for xs, il in m["batches"] for r in lm_ref.beam_search_lm(m["p_att"], m["cfg"], xs, il, cs["K"], m["lm"], cs["lm_w"])]
    assert [(r["tokens"], r["score"]) for r in cs["unbiased"]] == [(r["tokens"], r["score"]) for r in want]
    cs = bb.make_case("joint", "k6_lm")
    with ref_cpu.bf16_emulation():
        want = [r for xs, il in m["batches"]
                for r in jl.search(m["p"], m["cfg"], xs, il, cs["K"], cs["N"], cs["att_w"], cs["ctc_w"], m["lm"], cs["lm_w"], cs["len_bonus"])]
    assert [[(t, s) for t, s, _ in r["nbest"]] for r in cs["unbiased"]] == [r["nbest"] for r in want]


def test_every_rule_matters():
    hits = {mut: [(k, n) for k, n in ALL if not (k == "att" and mut == "bias_not_in_prebeam") and differs(k, n, mutate=mut)]
            for mut in bb.MUTATIONS if mut != "old_stop_rule"}
    print({m: len(h) for m, h in hits.items()})
    for mut, h in hits.items():
        assert h, mut


# ---------------------------------------------------------------- the scripted decoder (see the module's docstring)
SEQ = [1, 2, 3, 4, 1, 2, 1, 2]
SCRIPT_PHRASES = [[3, 4, 1]]


def scripted_logits(p, cfg, memory_b, mask_b, prefixes):
    """logits 0 for the scripted token, 0.5 for eos, -30 elsewhere: a token costs log(1 + e^0.5) = 0.974 nats, eos 0.474"""
    z = torch.full((len(prefixes), 6), -30.0)
    for i, h in enumerate(prefixes):
        z[i, SEQ[len(h)]] = 0.0
        z[i, 5] = 0.5
    return z


def test_the_old_stop_rule_loses_the_best_hypothesis(monkeypatch):
    monkeypatch.setattr(beam_ref, "last_logits", scripted_logits)
    p = {"char_trans.weight": torch.zeros(6, 1)}
    trie = bias_ref.build(SCRIPT_PHRASES)
    run = lambda **kw: bb.att_search_one(p, None, None, None, 2, len(SEQ), 0, None, 0.0, trie, 3.0, **kw)      # noqa: E731
    new, full, old = run(), run(stop=False), run(mutate="old_stop_rule")
    print(new["tokens"], new["score"], new["steps"], "| old rule:", old["tokens"], old["score"], old["steps"])
    assert key(new) == key(full)
    tok, eos = -math.log(1.0 + math.exp(0.5)), 0.5 - math.log(1.0 + math.exp(0.5))
    assert new["tokens"] == [1, 2, 3, 4, 1] and new["nbias"] == 3 and abs(new["score"] - (5 * tok + 9.0 + eos)) < 1e-4
    assert old["tokens"] == [] and old["steps"] == 1 and abs(old["score"] - eos) < 1e-5
    # the unbiased search on the same decoder stops there too, rightly: nothing can be gained
    plain = bb.att_search_one(p, None, None, None, 2, len(SEQ), 0, None, 0.0, trie, 0.0)
    assert plain["tokens"] == [] and plain["steps"] == 1


# ---------------------------------------------------------------- the cases are fit for purpose
@pytest.mark.parametrize("kind, name", GPU)
def test_at_most_a_quarter_of_a_case_is_without_slack(kind, name):
    gap = bb.att_min_gap if kind == "att" else bb.joint_min_gap
    res = bb.case_results(kind, name)
    ok = sum(gap(r) > JOINT_DELTA for r in res)
    print(f"{kind} {name}: {ok} of {len(res)} utterances have every decision gap > {JOINT_DELTA}")
    assert len(res) - ok <= len(res) // 4, (kind, name, ok)


def test_the_cases_exercise_the_feature():
    changed = revoked = rescued = credited = 0
    for kind, name in GPU:
        cs, res = bb.make_case(kind, name), bb.case_results(kind, name)
        changed += sum(a["tokens"] != b["tokens"] for a, b in zip(res, cs["unbiased"]))
        revoked += sum(r["revoked"] for r in res)
        rescued += sum(len(r.get("rescued", ())) for r in res)
        credited += sum(r["nbias"] > 0 for r in res)
        for r in res:                                        # nbias is a function of the tokens alone
            assert r["nbias"] == bias_ref.count(cs["trie"], r["tokens"]) >= 0
    print(f"changed {changed}, revoked {revoked}, rescued into the pre-beam {rescued}, with credit {credited}")
    assert changed >= 1 and revoked >= 1 and rescued >= 1 and credited >= 1


def test_phrase_lists_hold_a_phrase_inside_a_phrase_and_broken_pieces():
    for kind, name in GPU:
        ph = [tuple(x) for x in bb.make_case(kind, name)["phrases"]]
        assert len(set(ph)) == len(ph) and all(1 <= len(x) <= 5 for x in ph)
        assert any(a != b and b[:len(a)] == a for a in ph for b in ph), (kind, name)


# ---------------------------------------------------------------- the Tester's settings, in the manner of test_tester_bias_settings_cpu.py
MODES = ("bias_beam", "bias_joint_beam")


def vetted(mode, block, *, model="transformer", head=True, ctx="no/such/phrases.txt", lm_path=None):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=lm_path, context_path=ctx)
    t.decode_mode, t.model_name = mode, model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, 0
    return t


def test_mode_table_entries():
    T = tester_module.Tester
    for mode in MODES:
        assert mode in T.MODES and T.MODES[mode][0] is T._bias_step_settings and callable(T.MODES[mode][1])
    who = SimpleNamespace(beam_size=7, bias=SimpleNamespace(phrases=31))
    assert T.MODES["bias_beam"][2](who) == "phrase-biased beam decoding (bias_beam, beam 7, 31 phrases)"
    assert T.MODES["bias_joint_beam"][2](who) == "phrase-biased joint CTC/attention beam decoding (bias_joint_beam, beam 7, 31 phrases)"
    calls = []
    stub = SimpleNamespace(beam_size=4, lm=None, bias="PH", bias_weight=3.0, lm_weight=0.0, len_bonus=0.5, nbest=2, att_weight=0.6, ctc_weight=0.4,
                           min_step_ratio=0.0, max_step_ratio=1.0,
                           asr_model=SimpleNamespace(bias_beam_decode=lambda *a: (calls.append(("att",) + a), ([[5, 6], []], "scores", "nbias"))[1],
                                                     bias_joint_beam_decode=lambda *a: (calls.append(("joint",) + a), [[([5, 6], -1.0, 2)], []])[1]))
    assert T.MODES["bias_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert T.MODES["bias_joint_beam"][1](stub, "xs", "il") == [[5, 6], []]
    assert calls == [("att", "xs", "il", 4, "PH", 3.0, None, 0.0, 0.0, 1.0), ("joint", "xs", "il", 4, "PH", 3.0, None, 0.0, 0.5, 2, 0.0, 1.0, 0.6, 0.4)]


def test_the_decode_modes_are_command_line_choices():
    import train
    parser = train.build_parser()
    choices = next(a.choices for a in parser._actions if a.dest == "decode_mode")
    assert set(MODES) <= set(choices) and set(choices) == set(tester_module.Tester.MODES)


OK = {"beam_size": 4, "ctc_w": 0.4}
NO_CTX = "{}: no phrase list given; pass --context_path (one phrase per line as space-separated unit ids)"
BOTH = [
    ("no context path", OK, dict(ctx=None), NotImplementedError, NO_CTX),
    ("no context path, nothing else looked at", None, dict(ctx=None, model="blstm"), NotImplementedError, NO_CTX),
    ("a BLSTM", OK, dict(model="blstm"), NotImplementedError,
     "{}: the attention and joint beams need the transformer's decoder, the BLSTM has none; use --decode_mode bias_ctc_beam"),
    ("no block", None, {}, ValueError, "decode_mode '{}' needs a solver.beam_decode block with at least beam_size in the config"),
    ("beam_size 65", {"beam_size": 65}, {}, ValueError, "solver.beam_decode.beam_size must be in [1, 64], got 65"),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what,block,kw,exc,msg", BOTH, ids=[b[0] for b in BOTH])
def test_refusals_of_both_modes(mode, what, block, kw, exc, msg):
    if mode == "bias_beam" and block is OK:
        kw = dict(kw, head=False)                            # (a hybrid model with ctc_w > 0 is bias_joint_beam's)
    with pytest.raises(exc) as e:
        vetted(mode, block, **kw)._bias_step_settings()
    assert str(e.value) == msg.format(mode)


def test_refusals_of_one_mode():
    def refused(mode, block, exc, **kw):
        with pytest.raises(exc) as e:
            vetted(mode, block, **kw)._bias_step_settings()
        return str(e.value)
    assert "--decode_mode bias_joint_beam" in refused("bias_beam", OK, ValueError)
    assert refused("bias_joint_beam", OK, ValueError, head=False) == \
        ("decode_mode 'bias_joint_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
         "use --decode_mode bias_beam, beam or greedy")
    for block in ({"beam_size": 4}, {"beam_size": 4, "ctc_w": 0.0}):
        assert refused("bias_joint_beam", block, ValueError).startswith("bias_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0)")
    assert refused("bias_joint_beam", dict(OK, nbest=5), ValueError) == "solver.beam_decode.nbest must be in [1, beam_size], got 5"
    for mode, kw in (("bias_beam", dict(head=False)), ("bias_joint_beam", {})):
        assert refused(mode, dict(OK, bias_w=-0.5), ValueError, **kw) == "solver.beam_decode.bias_w must be finite and >= 0, got -0.5"
        assert refused(mode, dict(OK, bias_w=float("nan")), ValueError, **kw) == "solver.beam_decode.bias_w must be finite and >= 0, got nan"
        assert refused(mode, dict(OK, lm_w=-1.0), ValueError, lm_path="no/such.arpa", **kw) == "solver.beam_decode.lm_w must be finite and >= 0, got -1.0"


def test_defaults_and_the_optional_lm(tmp_path):
    # without --lm_model_path a bad lm_w is nobody's business: the settings get as far as the phrase file
    for mode, kw in (("bias_beam", dict(head=False)), ("bias_joint_beam", {})):
        t = vetted(mode, dict(OK, lm_w=-1.0), ctx=str(tmp_path / "missing.txt"), **kw)
        with pytest.raises(FileNotFoundError):
            t._bias_step_settings()
        assert t.bias_weight == 3.0 and t.lm is None and t.lm_weight == 0.0
        assert (t.min_step_ratio, t.max_step_ratio) == (0.0, 1.0)
    assert t.ctc_weight == 0.4 and abs(t.att_weight - 0.6) < 1e-12 and t.nbest == 1 and t.len_bonus == 0.0
    # a plain model: ctc_w is ignored by bias_beam
    t = vetted("bias_beam", OK, head=False, ctx=str(tmp_path / "missing.txt"))
    with pytest.raises(FileNotFoundError):
        t._bias_step_settings()
