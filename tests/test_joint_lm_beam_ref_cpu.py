"""The CPU restatement of the joint beam with LM, bonus and N-best (tests/joint_lm_beam_ref.py) against independent facts: its
degenerate settings are joint_beam_ref and lm_ref, a beam that prunes nothing finds the exhaustive best-N, the bound stop rule gives what
the beam run to maxlen gives, and each rule of the contract matters (a mutated restatement differs somewhere).  It also asserts, on the
restatement alone, that enough utterances of tests/test_hip_joint_lm_beam.py's cases have every decision gap above JOINT_DELTA.  CPU only."""
import itertools
import math

import pytest
import torch

import hybrid_ref
import joint_beam_ref as jr
import joint_lm_beam_ref as jl
import lm_ref
from decode_util import C_SMALL, JOINT_DELTA, joint_state_dict
from oracle import ref_cpu
from oracle.make_goldens import TINY, synth_batch
from test_hip_engine import HKUST


@pytest.fixture(scope="module")
def tiny_p():
    return hybrid_ref.leafify(joint_state_dict(TINY, 7), TINY)


@pytest.fixture(scope="module")
def lm():
    return lm_ref.toy_lm(C_SMALL, jl.LM_ORDER, jl.LM_SEED)


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in jl.TINY_BATCHES]


_RUNS = {}


def run(p, lm, batches, K, setting, **kw):
    """all nine utterances' results (no bf16 emulation: these tests compare restatements with one another); computed once per setting"""
    key = (K, setting, tuple(sorted(kw.items())))
    if key not in _RUNS:
        aw, cw, lw, bo, N = setting
        _RUNS[key] = [r for xs, il in batches for r in jl.search(p, TINY, xs, il, K, N, aw, cw, lm, lw, bo, **kw)]
    return _RUNS[key]


def same(a, b):
    return [r["nbest"] for r in a] == [r["nbest"] for r in b]


def test_no_lm_no_bonus_one_best_is_the_joint_beam(tiny_p, lm, batches):
    for K, (aw, cw) in itertools.product((4, 20), ((0.5, 0.5), (0.7, 0.3), (0.0, 1.0))):
        got = run(tiny_p, lm, batches, K, (aw, cw, 0.0, 0.0, 1))
        want = [r for xs, il in batches for r in jr.joint_beam_search(tiny_p, TINY, xs, il, K, aw, cw)]
        for g, w in zip(got, want):
            assert g["tokens"] == w["tokens"] and g["score"] == w["score"], (K, aw, cw, g["nbest"], w["tokens"], w["score"])
            assert g["sel_gaps"] == w["sel_gaps"] and g["stop_gaps"] == w["stop_gaps"]


def test_without_the_ctc_terms_it_is_the_lm_beam(tiny_p, lm, batches):
    """drop_ctc: no CTC term, no pre-beam cut, class 0 admitted -- lm_ref.beam_search_lm's candidates.  The tokens are equal; the scores are
    the same sums grouped differently, fl(fl(s + lp) + lm) here and fl(s + fl(lp + lm)) there, so they agree to a few ulp per step"""
    pa = ref_cpu.leafify({k: v for k, v in joint_state_dict(TINY, 7).items() if k not in hybrid_ref.HEAD}, TINY)
    for K, lw in ((4, 0.5), (20, 1.0)):
        got = run(tiny_p, lm, batches, K, (1.0, 0.0, lw, 0.0, 1), drop_ctc=True)
        want = [r for xs, il in batches for r in lm_ref.beam_search_lm(pa, TINY, xs, il, K, lm, lw)]
        for g, w in zip(got, want):
            assert g["tokens"] == w["tokens"], (K, lw, g["nbest"], w["tokens"])
            assert abs(g["score"] - w["score"]) <= 1e-5 * max(1.0, abs(w["score"]))


def test_a_beam_that_prunes_nothing_is_the_exhaustive_best_n():
    C = 4                                                    # blank 0, tokens 1 and 2, eos 3
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, C, seed=5), C, seed=105)
    sd[hybrid_ref.HEAD[0]] = sd[hybrid_ref.HEAD[0]] * 4.0
    p = hybrid_ref.leafify(sd, TINY)
    lm4 = lm_ref.toy_lm(C, 3, 1, n_sent=20, max_len=4)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3
    n = 0
    for (aw, cw, lw, bo, N), minr in itertools.product(((0.5, 0.5, 0.5, 0.0, 1), (0.7, 0.3, 1.0, 1.0, 3), (0.0, 1.0, 0.5, -0.5, 4), (0.5, 0.5, 0.5, 3.0, 5)),
                                                      (0.0, 0.5)):
        got = jl.search(p, TINY, xs, il, 64, N, aw, cw, lm4, lw, bo, min_step_ratio=minr)
        want = jl.exhaustive(p, TINY, xs, il, N, aw, cw, lm4, lw, bo, min_step_ratio=minr)
        for g, w in zip(got, want):
            assert len(g["nbest"]) == len(w)
            for (gt, gs), (wt, ws) in zip(g["nbest"], w):
                assert gs == ws, (aw, cw, lw, bo, N, g["nbest"], w)
            if all(d > 1e-5 for d in g["nb_gaps"]):
                assert [t for t, _ in g["nbest"]] == [t for t, _ in w]
                n += 1
            assert len({tuple(t) for t, _ in g["nbest"]}) == len(g["nbest"])       # distinct sequences
    assert n >= 16, n


@pytest.mark.parametrize("K", jl.TINY_KS)
def test_the_stop_rule_gives_the_beam_run_to_maxlen(tiny_p, lm, batches, K):
    for s in jl.SETTINGS + ((0.5, 0.5, 0.5, 3.0, 2), (0.7, 0.3, 0.3, 0.0, 4)):
        assert same(run(tiny_p, lm, batches, K, s), run(tiny_p, lm, batches, K, s, stop="none")), s


# (K, setting): the GPU file's settings at K = 4, a large bonus at ctc_w = 1 (the old rule loses the best hypothesis there) and four entries
# without a bonus at K = 20 (the list fills early and its best entry is far above its fourth)
MUT_CASES = tuple((4, s) for s in jl.SETTINGS + ((0.0, 1.0, 0.5, 6.0, 1), (0.5, 0.5, 0.5, 4.0, 2))) + ((20, (0.7, 0.3, 0.3, 0.0, 4)),)


def _differs(p, lm, batches, **mut):
    return [(K, s) for K, s in MUT_CASES if not same(run(p, lm, batches, K, s), run(p, lm, batches, K, s, **mut))]


def test_the_old_stop_rule_loses_the_best_hypothesis_under_a_bonus(tiny_p, lm, batches):
    """DESIGN 9's rule (best >= run_best) stops too early once a running hypothesis can still collect bonuses"""
    hit = [(K, s) for K, s in _differs(tiny_p, lm, batches, stop="old") if s[3] > 0
           and any(a["tokens"] != b["tokens"] for a, b in zip(run(tiny_p, lm, batches, K, s), run(tiny_p, lm, batches, K, s, stop="old")))]
    assert hit


def test_the_stop_test_needs_the_nth_score(tiny_p, lm, batches):
    hit = [(K, s) for K, s in _differs(tiny_p, lm, batches, stop="best") if s[4] > 1]
    assert hit


def test_every_rule_matters(tiny_p, lm, batches):
    assert _differs(tiny_p, lm, batches, bonus_on_eos=True)
    assert _differs(tiny_p, lm, batches, lm_in_prebeam=False)
    assert _differs(tiny_p, lm, batches, stop="old")
    assert _differs(tiny_p, lm, batches, stop="best")


def test_the_lm_and_the_bonus_change_the_result(tiny_p, lm, batches):
    s = (0.7, 0.3, 0.3, 1.0, 2)
    base = run(tiny_p, lm, batches, 4, s)
    no_lm = run(tiny_p, lm, batches, 4, (0.7, 0.3, 0.0, 1.0, 2))
    assert any(a["tokens"] != b["tokens"] for a, b in zip(base, no_lm))
    bonus = run(tiny_p, lm, batches, 4, (0.5, 0.5, 0.5, 5.0, 1))
    no_bonus = run(tiny_p, lm, batches, 4, (0.5, 0.5, 0.5, 0.0, 1))
    assert sum(len(a["tokens"]) > len(b["tokens"]) for a, b in zip(bonus, no_bonus)) >= 3
    assert not any(len(a["tokens"]) < len(b["tokens"]) for a, b in zip(bonus, no_bonus))


def _share(results):
    return sum(jl.min_gap(r) > JOINT_DELTA for r in results), len(results)


@pytest.mark.parametrize("K", jl.TINY_KS)
def test_enough_utterances_qualify_tiny(tiny_p, lm, batches, K):
    """the condition tests/test_hip_joint_lm_beam.py relies on, for exactly its cases and under the engine's bf16 operand rounding"""
    ok = n = 0
    for s in jl.SETTINGS:
        aw, cw, lw, bo, N = s
        with ref_cpu.bf16_emulation():
            res = [r for xs, il in batches for r in jl.search(tiny_p, TINY, xs, il, K, N, aw, cw, lm, lw, bo)]
        a, b = _share(res)
        print(f"K = {K}, {s}: {a} of {b} qualify")
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_enough_utterances_qualify_hkust_geometry(lm):
    p = hybrid_ref.leafify(joint_state_dict(HKUST, 3), HKUST)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor(jl.HKUST_ILENS)
    ok = n = 0
    for s in jl.HKUST_SETTINGS:
        aw, cw, lw, bo, N = s
        with ref_cpu.bf16_emulation():
            a, b = _share(jl.search(p, HKUST, xs, il, 4, N, aw, cw, lm, lw, bo))
        print(f"hkust geometry, {s}: {a} of {b} qualify")
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)
