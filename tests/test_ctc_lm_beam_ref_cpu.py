"""The CPU restatement of the LM-fused CTC prefix beam search (tests/ctc_lm_beam_ref.py) checked against itself: against the
plain restatement at lm_w = 0, against brute force over all prefixes on tiny shapes, its lmacc against recomputation from the tokens, and
the two conditions its cases were chosen for -- so that tests/test_hip_ctc_lm_beam_kernel.py cannot skip its way to green."""
import numpy as np
import pytest

import ctc_beam_ref as cr
import ctc_lm_beam_ref as lr
import lm_ref


@pytest.mark.parametrize("name", ["basic", "few_classes", "peaky_merge", "neg_inf"])
def test_zero_weight_reproduces_the_plain_restatement(name):
    cs, z, lens = cr.make_case(name)
    lm = lm_ref.toy_lm(cs["C"], 3, 0)
    for K in cs["Ks"]:
        plain = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, K, 0, cs["eos"], cs["nbest"])
        fused = lr.ctc_lm_beam_ref_batch(z[..., :cs["C"]], lens, K, lm, 0.0, 0.0, cs["nbest"])
        for p, f in zip(plain, fused):
            assert [(h, s) for h, s, am, acc in f["nbest"]] == p["nbest"]
            assert all(s == am and acc == 0.0 for h, s, am, acc in f["nbest"])
            assert (f["slack"], f["min_gap"], f["merges"], f["recreated"]) == (p["slack"], p["min_gap"], p["merges"], p["recreated"])


@pytest.mark.parametrize("T,C,order,lm_w,bonus,seed", [(5, 4, 3, 0.8, 0.0, 0), (6, 4, 2, 0.5, 0.7, 1), (4, 4, 4, 1.5, -0.3, 2), (6, 3, 3, 0.8, 0.4, 3)])
def test_brute_force_on_tiny_shapes(T, C, order, lm_w, bonus, seed):
    # K above the number of reachable prefixes (at most 2^(T + 1) - 1 over two emittable classes): nothing is pruned, so the search is exact
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
    lm = lm_ref.toy_lm(C, order, seed)
    want = lr.brute_force(z, lm, lm_w, bonus)
    K = 2 ** (T + 1)
    got = lr.ctc_lm_beam_ref(z, K, lm, lm_w, bonus)["nbest"]
    assert len(got) == len(want) < K
    for (h, s, am, acc), (h2, s2, am2) in zip(got, want):
        assert h == h2 and abs(s - s2) < 1e-9 and abs(am - am2) < 1e-9


@pytest.mark.parametrize("name", list(lr.LM_CASES))
def test_case_conditions(name):
    cs, z, lens, lm = lr.make_lm_case(name)
    refs = lr.case_refs(name)
    C = cs["C"]
    differs = False
    for K in cs["Ks"]:
        rs = refs[K]
        # at least 3/4 of the utterances are compared on the GPU
        assert 4 * sum(not r["slack"] > 0 for r in rs) <= len(rs), (name, K, [r["slack"] for r in rs])
        # lmacc of every returned entry is a function of its tokens alone
        for r in rs:
            for h, s, am, acc in r["nbest"]:
                want = lr.lmacc32(lm, h, cs["lm_w"], cs["len_bonus"])
                assert acc.dtype == np.float32 and acc == want, (name, K, h)
                assert s == am + float(acc) + float(lr.eos_term32(lm, h, cs["lm_w"], C - 1))
        plain = cr.ctc_beam_ref_batch(z[..., :C], lens, K, 0, C - 1, cs["nbest"])
        differs |= any(r["nbest"][0][0] != p["nbest"][0][0] for r, p in zip(rs, plain))
    assert differs, name                                        # a no-op LM cannot pass


def test_cases_cover_what_they_are_for():
    assert lr.LM_CASES["basic_order1"]["order"] == 1 and lr.LM_CASES["full_buffer"]["order"] == 4
    assert {lr.LM_CASES[n]["len_bonus"] for n in ("basic", "basic_bonus_pos", "basic_bonus_neg")} == {0.0, 0.7, -0.3}
    assert 0 in lr.make_lm_case("few_classes")[0]["lens"] and 1 in lr.make_lm_case("basic")[0]["lens"]
    assert lr.make_lm_case("wide_367")[0]["ld"] == 369
    assert lr.table_max_probe(lr.make_lm_case("wide_367")[3]) >= 2      # a probe that does not end at its first slot
    r = lr.case_refs("peaky_merge")[3]
    assert sum(x["merges"] for x in r) > 0 and sum(x["recreated"] for x in r) > 0


@pytest.mark.parametrize("mutate", ["lm_in_pnb", "no_eos", "bonus_on_stay"])
def test_mutated_restatements_differ(mutate):
    hit = []
    for name in ("basic", "basic_bonus_pos", "basic_bonus_neg", "peaky_merge"):
        cs, z, lens, lm = lr.make_lm_case(name)
        K = cs["Ks"][-1]
        bad = lr.ctc_lm_beam_ref_batch(z[..., :cs["C"]], lens, K, lm, cs["lm_w"], cs["len_bonus"], cs["nbest"], mutate=mutate)
        for r, m in zip(lr.case_refs(name)[K], bad):
            same = len(r["nbest"]) == len(m["nbest"]) and all(
                a[0] == b[0] and abs(a[1] - b[1]) <= cr.tol(a[1]) and abs(a[2] - b[2]) <= cr.tol(a[2]) for a, b in zip(r["nbest"], m["nbest"]))
            if not same:
                hit.append(name)
    assert hit, mutate
    if mutate == "bonus_on_stay":
        assert "basic" not in hit                               # without a bonus there is nothing to misapply
