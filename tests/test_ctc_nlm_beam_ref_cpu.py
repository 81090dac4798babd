"""The restatement of the LSTM-LM-fused CTC prefix beam (tests/ctc_nlm_beam_ref.py) checked on the CPU: against the plain
restatement at lm_w = 0, against a brute force over all paths on tiny shapes, its lmacc against recomputation from the tokens, its two
mutations, and the conditions the GPU test's cases were chosen for."""
import numpy as np
import pytest

import ctc_beam_ref as cr
import ctc_nlm_beam_ref as nr
import nlm_ref


@pytest.mark.parametrize("name", ["basic", "few_classes", "peaky_merge", "neg_inf"])
def test_zero_weight_reproduces_the_plain_restatement(name):
    cs, z, lens = cr.make_case(name)
    row = nr.default_lm_row(nlm_ref.toy_nlm(cs["C"], *nr.NLM_DIMS, 0))
    for K in cs["Ks"]:
        want = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, K, 0, cs["C"] - 1, cs["nbest"])
        got = nr.ctc_nlm_beam_ref_batch(z[..., :cs["C"]], lens, K, row, 0.0, 0.0, cs["nbest"])
        for w, g in zip(want, got):
            assert [e[0] for e in g["nbest"]] == [e[0] for e in w["nbest"]]
            assert [e[1] for e in g["nbest"]] == [e[1] for e in w["nbest"]] and [e[2] for e in g["nbest"]] == [e[1] for e in w["nbest"]]


@pytest.mark.parametrize("T,seed,lm_w,bonus", [(3, 0, 0.8, 0.0), (4, 1, 0.8, 0.5), (5, 2, 0.5, -0.3)])
def test_tiny_shapes_equal_brute_force(T, seed, lm_w, bonus):
    C = 5                                                   # blank, 3 emittable classes, eos
    z = (np.random.default_rng(seed).standard_normal((T, C)) * 2.0).astype(np.float32)
    row = nr.default_lm_row(nlm_ref.toy_nlm(C, *nr.NLM_DIMS, seed))
    bf = nr.brute_force(z, row, lm_w, bonus)
    K = len(bf)                                             # every reachable prefix fits the beam: the search is exhaustive
    r = nr.ctc_nlm_beam_ref(z, K, row, lm_w, bonus)
    assert len(r["nbest"]) == len(bf)
    got = {e[0]: (e[1], e[2]) for e in r["nbest"]}
    for h, fin, am in bf:
        assert abs(got[h][0] - fin) < 1e-9 and abs(got[h][1] - am) < 1e-9, (h, got[h], fin, am)
    assert r["nbest"][0][0] == bf[0][0]


@pytest.mark.parametrize("name", list(nr.NLM_CASES))
def test_lmacc_is_a_function_of_the_tokens(name):
    cs, z, lens, m = nr.make_nlm_case(name)
    row = nr.default_lm_row(m)
    for K, refs in nr.case_refs(name).items():
        for r in refs:
            for h, acc in r["beam_lmacc"]:
                want = nr.lmacc32(row, h, cs["lm_w"], cs["len_bonus"])
                assert np.float32(acc).tobytes() == np.float32(want).tobytes(), (name, K, h)


@pytest.mark.parametrize("mut", nr.MUTATIONS)
def test_each_mutation_changes_an_nbest_list(mut):
    changed = 0
    for name in ("basic", "peaky_merge", "few_classes"):
        cs, z, lens, m = nr.make_nlm_case(name)
        row = nr.default_lm_row(m)
        for K, refs in nr.case_refs(name).items():
            if K == 1:
                continue
            bad = nr.ctc_nlm_beam_ref_batch(z[..., :cs["C"]], lens, K, row, cs["lm_w"], cs["len_bonus"], cs["nbest"], mutate=mut)
            for r, b in zip(refs, bad):
                if r["slack"] > 0 and [(e[0], e[1]) for e in r["nbest"]] != [(e[0], e[1]) for e in b["nbest"]]:
                    changed += 1
    assert changed >= 1, mut


@pytest.mark.parametrize("name", list(nr.NLM_CASES))
def test_cases_have_slack_and_the_lm_matters(name):
    cs, z, lens, m = nr.make_nlm_case(name)
    moved = 0
    for K, refs in nr.case_refs(name).items():
        ok = sum(r["slack"] > 0 for r in refs)
        plain = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, K, 0, cs["C"] - 1, cs["nbest"])
        moved_k = sum(r["nbest"][0][0] != q["nbest"][0][0] for r, q in zip(refs, plain))
        moved = max(moved, moved_k)
        print(f"{name} K={K}: slack > 0 on {ok}/{len(refs)}, best hypotheses the LM changes {moved_k}, recreated "
              f"{sum(r['recreated'] for r in refs)}, smallest positive slack {min((r['slack'] for r in refs if r['slack'] > 0), default=0):.3g}")
        assert 4 * ok >= 3 * len(refs), (name, K, ok)
    assert moved >= 1, name
