"""The CPU restatement of the joint beam with the LSTM LM, a bonus and N-best (tests/nlm_joint_beam_ref.py) against independent
facts: with lm_w = 0 it is joint_lm_beam_ref's search at lm_w = 0, without the CTC terms it is nlm_ref's beam, a beam that prunes nothing finds
the exhaustive best-N, the bound stop rule gives what the beam run to maxlen gives, and each rule of the contract matters (a mutated restatement
differs somewhere; reading the LM state from the row's own slot differs on an utterance that qualifies).  It also asserts, on the restatement
alone, that enough utterances of tests/test_hip_nlm_joint_beam.py's cases have every decision gap above JOINT_DELTA.  CPU only."""
import itertools

import pytest
import torch

import hybrid_ref
import joint_lm_beam_ref as jl
import lm_ref
import nlm_joint_beam_ref as nj
import nlm_ref
from decode_util import C_SMALL, JOINT_DELTA, joint_state_dict
from oracle import ref_cpu
from oracle.make_goldens import TINY, synth_batch
from test_hip_engine import HKUST


@pytest.fixture(scope="module")
def tiny_p():
    return hybrid_ref.leafify(joint_state_dict(TINY, 7), TINY)


@pytest.fixture(scope="module")
def nlm():
    return nj.tiny_nlm(C_SMALL)


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in nj.TINY_BATCHES]


_RUNS = {}


def run(p, m, batches, K, setting, emu=False, **kw):
    """all nine utterances' results; emu: under the engine's bf16 operand rounding (the GPU file's reference), else plain fp32 (these tests
    compare restatements with one another); computed once per case"""
    key = (K, setting, emu, tuple(sorted(kw.items())))
    if key not in _RUNS:
        aw, cw, lw, bo, N = setting

        def go():
            return [r for xs, il in batches for r in nj.search(p, TINY, xs, il, K, N, aw, cw, m, lw, bo, **kw)]
        if emu:
            with ref_cpu.bf16_emulation():
                _RUNS[key] = go()
        else:
            _RUNS[key] = go()
    return _RUNS[key]


def same(a, b):
    return [r["nbest"] for r in a] == [r["nbest"] for r in b]


def lists(r):
    return [t for t, _ in r["nbest"]]


@pytest.mark.parametrize("K", nj.TINY_KS)
def test_with_lm_weight_zero_it_is_the_joint_lm_beam_at_zero(tiny_p, nlm, batches, K):
    """any LM weighs nothing at lm_w = 0: tokens and scores of every list entry equal joint_lm_beam_ref's with an n-gram LM"""
    ngram = lm_ref.toy_lm(C_SMALL, jl.LM_ORDER, jl.LM_SEED)
    for aw, cw, _, bo, N in nj.SETTINGS:
        got = run(tiny_p, nlm, batches, K, (aw, cw, 0.0, bo, N))
        want = [r for xs, il in batches for r in jl.search(tiny_p, TINY, xs, il, K, N, aw, cw, ngram, 0.0, bo)]
        assert same(got, want), (K, aw, cw, bo, N)
        for g, w in zip(got, want):
            assert g["sel_gaps"] == w["sel_gaps"] and g["stop_gaps"] == w["stop_gaps"] and g["pre_gaps"] == w["pre_gaps"]


def test_without_the_ctc_terms_it_is_the_nlm_beam(tiny_p, nlm, batches):
    """drop_ctc: no CTC term, no pre-beam cut, class 0 admitted -- nlm_ref.beam_search_nlm's candidates, the LM state in the same K slots.  The
    tokens are equal; the scores are the same sums grouped differently, so they agree to a few ulp per step"""
    pa = ref_cpu.leafify({k: v for k, v in joint_state_dict(TINY, 7).items() if k not in hybrid_ref.HEAD}, TINY)
    for K, lw in ((4, 0.5), (20, 1.0)):
        got = run(tiny_p, nlm, batches, K, (1.0, 0.0, lw, 0.0, 1), drop_ctc=True)
        want = [r for xs, il in batches for r in nlm_ref.beam_search_nlm(pa, TINY, xs, il, K, nlm, lw)]
        for g, w in zip(got, want):
            assert g["tokens"] == w["tokens"], (K, lw, g["nbest"], w["tokens"])
            assert abs(g["score"] - w["score"]) <= 1e-5 * max(1.0, abs(w["score"]))


def test_the_slots_carry_the_row_of_the_whole_history(nlm):
    """a row stepped from its parent's slot is nlm_ref.lm_row of its tokens: what the contract's lm(c | h) means"""
    h, state = (), nlm_ref.zero_state(nlm)
    for tok in (3, 7, 7, 1, 10):
        row, state = nlm_ref.step(nlm, h[-1] if h else nlm["start_id"], state)
        assert (row == nlm_ref.lm_row(nlm, h)).all()
        h += (tok,)


def test_a_beam_that_prunes_nothing_is_the_exhaustive_best_n():
    C = 4                                                    # blank 0, tokens 1 and 2, eos 3
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, C, seed=5), C, seed=105)
    sd[hybrid_ref.HEAD[0]] = sd[hybrid_ref.HEAD[0]] * 4.0
    p = hybrid_ref.leafify(sd, TINY)
    m4 = nlm_ref.toy_nlm(C, 8, 12, 2, 1)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3
    n = 0
    for (aw, cw, lw, bo, N), minr in itertools.product(((0.5, 0.5, 0.5, 0.0, 1), (0.7, 0.3, 1.0, 1.0, 3), (0.0, 1.0, 0.5, -0.5, 4), (0.5, 0.5, 0.5, 3.0, 5)),
                                                      (0.0, 0.5)):
        got = nj.search(p, TINY, xs, il, 64, N, aw, cw, m4, lw, bo, min_step_ratio=minr)
        want = nj.exhaustive(p, TINY, xs, il, N, aw, cw, m4, lw, bo, min_step_ratio=minr)
        for g, w in zip(got, want):
            assert len(g["nbest"]) == len(w)
            for (gt, gs), (wt, ws) in zip(g["nbest"], w):
                assert gs == ws, (aw, cw, lw, bo, N, g["nbest"], w)
            if all(d > 1e-5 for d in g["nb_gaps"]):
                assert lists(g) == [t for t, _ in w]
                n += 1
            assert len({tuple(t) for t in lists(g)}) == len(g["nbest"])       # distinct sequences
    assert n >= 16, n


@pytest.mark.parametrize("K", nj.TINY_KS)
def test_the_stop_rule_gives_the_beam_run_to_maxlen(tiny_p, nlm, batches, K):
    for s in nj.SETTINGS + ((0.5, 0.5, 0.5, 3.0, 2), (0.7, 0.3, 0.3, 0.0, 4)):
        assert same(run(tiny_p, nlm, batches, K, s), run(tiny_p, nlm, batches, K, s, stop="none")), s


# (K, setting): joint_lm_beam_ref's mutation cases -- the GPU file's settings at K = 4, a large bonus at ctc_w = 1 (the old rule loses the best
# hypothesis there) and four entries without a bonus at K = 20
MUT_CASES = tuple((4, s) for s in nj.SETTINGS + ((0.0, 1.0, 0.5, 6.0, 1), (0.5, 0.5, 0.5, 4.0, 2))) + ((20, (0.7, 0.3, 0.3, 0.0, 4)),)


def _differs(p, m, batches, **mut):
    return [(K, s) for K, s in MUT_CASES if not same(run(p, m, batches, K, s), run(p, m, batches, K, s, **mut))]


def test_every_rule_matters(tiny_p, nlm, batches):
    # the pre-beam's cut decides at narrow beams only (12 classes: at K = 4 the P = 6 best by lp hold every candidate the search keeps, with or
    # without the LM term): K = 2 and 3, P = 3 and 4, the GPU file's settings with N cut to K
    narrow = [(K, s[:4] + (min(s[4], K),)) for K in (2, 3) for s in nj.SETTINGS]
    assert [c for c in narrow if not same(run(tiny_p, nlm, batches, *c), run(tiny_p, nlm, batches, *c, lm_in_prebeam=False))]
    assert _differs(tiny_p, nlm, batches, bonus_on_eos=True)
    assert _differs(tiny_p, nlm, batches, stop="old")


def test_the_state_must_come_from_the_parents_slot_and_the_lm_matters(tiny_p, nlm, batches):
    """at the GPU file's own_slot setting, under its bf16 rounding: an utterance whose every decision gap is above JOINT_DELTA -- one the GPU
    test compares token for token -- gets other lists when a row reads its own slot, and other tokens when the LM weighs nothing"""
    K, s = nj.OWN_SLOT_K, nj.OWN_SLOT_SETTING
    base = run(tiny_p, nlm, batches, K, s, emu=True)
    own = run(tiny_p, nlm, batches, K, s, emu=True, own_slot=True)
    no_lm = run(tiny_p, nlm, batches, K, s[:2] + (0.0,) + s[3:], emu=True)
    qual = [i for i, r in enumerate(base) if nj.min_gap(r) > JOINT_DELTA]
    hit_own = [i for i in qual if lists(base[i]) != lists(own[i])]
    hit_lm = [i for i in qual if base[i]["tokens"] != no_lm[i]["tokens"]]
    print(f"K = {K}, {s}: qualifying {qual}; own_slot differs on {hit_own}; lm_w = 0 differs on {hit_lm}; "
          f"lengths {[len(r['tokens']) for r in base]}")
    assert hit_own and hit_lm
    assert max(len(base[i]["tokens"]) for i in hit_own) >= 3      # the chain is more than one step long there


def _share(results):
    return sum(nj.min_gap(r) > JOINT_DELTA for r in results), len(results)


@pytest.mark.parametrize("K", nj.TINY_KS)
def test_enough_utterances_qualify_tiny(tiny_p, nlm, batches, K):
    """the condition tests/test_hip_nlm_joint_beam.py relies on, for exactly its cases and under the engine's bf16 operand rounding"""
    ok = n = 0
    for s in nj.SETTINGS:
        a, b = _share(run(tiny_p, nlm, batches, K, s, emu=True))
        print(f"K = {K}, {s}: {a} of {b} qualify")
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_enough_utterances_qualify_hkust_geometry():
    p = hybrid_ref.leafify(joint_state_dict(HKUST, 3), HKUST)
    m = nj.tiny_nlm(C_SMALL, nj.NLM_SEED_HKUST)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor(nj.HKUST_ILENS)
    ok = n = 0
    for s in nj.HKUST_SETTINGS:
        aw, cw, lw, bo, N = s
        with ref_cpu.bf16_emulation():
            a, b = _share(nj.search(p, HKUST, xs, il, 4, N, aw, cw, m, lw, bo))
        print(f"hkust geometry, {s}: {a} of {b} qualify")
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)
