"""The phrase automaton (tests/bias_ref.py) and the CPU restatement of the phrase-biased CTC prefix beam search (tests/ctc_bias_beam_ref.py,
DESIGN 5.13) checked against themselves: the automaton's identities, the restatement against the unbiased ones at bias_w = 0 and against brute
force over all prefixes on tiny shapes, and the conditions its cases were chosen for -- so that tests/test_hip_ctc_bias_beam_kernel.py cannot
skip its way to green."""
import numpy as np
import pytest

import bias_ref
import ctc_beam_ref as cr
import ctc_bias_beam_ref as br
import ctc_lm_beam_ref as lr
import lm_ref


# ---------------------------------------------------------------- the automaton
def test_a_phrase_inside_a_phrase_earns_its_tokens():
    t = bias_ref.build([[1, 2], [1, 2, 3, 4], [5]])
    assert t["nodes"] == 6 and t["revoke"] == [0, 1, 0, 1, 0, 0]
    assert bias_ref.count(t, [1, 2]) == 2 and bias_ref.count(t, [1, 2, 3, 4]) == 4
    assert bias_ref.count(t, [1, 2, 3]) == 2                  # the longer match is unfinished: its third token is revoked, `1 2` stays
    assert bias_ref.count(t, [1, 2, 3, 6]) == 2 and bias_ref.count(t, [1, 2, 3, 5]) == 3
    assert bias_ref.count(t, [1]) == 0 and bias_ref.count(t, [1, 6]) == 0 and bias_ref.count(t, [5, 5]) == 2
    assert bias_ref.count(t, [1, 1, 2]) == 2                  # the token that broke `1 ?` starts the next match


def test_overlapping_restarts_are_missed_on_purpose():
    t = bias_ref.build([[1, 1, 2]])
    assert bias_ref.count(t, [1, 1, 2]) == 3 and bias_ref.count(t, [1, 1, 1, 2]) == 0      # no failure links
    assert bias_ref.state_of(t, [1, 1, 1]) == (1, 1)


@pytest.mark.parametrize("C,P,seed,maxlen", [(12, 6, 0, 4), (5, 5, 1, 3), (40, 200, 2, 6), (4096, 3000, 3, 6)])
def test_automaton_identities(C, P, seed, maxlen):
    phrases = bias_ref.toy_phrases(C, P, seed, maxlen)
    assert len(phrases) == P == len({tuple(p) for p in phrases}) and all(1 <= len(p) <= maxlen and all(1 <= c <= C - 2 for c in p) for p in phrases)
    t = bias_ref.build(phrases)
    assert t["revoke"][0] == 0 and all(0 <= r <= d for r, d in zip(t["revoke"], t["depth"]))
    rng = np.random.default_rng(seed)
    alphabet = sorted({c for p in phrases for c in p})[:6]     # a few tokens only, so matches start, continue and break
    for _ in range(200):
        h = [int(c) for c in rng.choice(alphabet, size=int(rng.integers(0, 12)))]
        s = bias_ref.ROOT
        for i, c in enumerate(h):
            back = bias_ref.revoked_by(t, s, c)
            s2 = bias_ref.step(t, s, c)
            assert s2 == bias_ref.state_of(t, h[:i + 1])      # a function of the tokens alone
            assert s2[1] >= 0 and bias_ref.n_final(t, s2) >= 0
            # a token either extends the match (+1), or takes back exactly the unearned tokens and may start a new match
            assert s2[1] in (s[1] + 1, s[1] - back, s[1] - back + 1) and (back == 0 or (s[0], c) not in t["child"])
            assert s2[1] >= t["depth"][s2[0]] >= t["revoke"][s2[0]]           # the running match's tokens are all credited for now
            s = s2
    for p in phrases:                                          # a whole phrase, alone, earns all its tokens; its leaf revokes nothing
        assert bias_ref.count(t, p) == len(p) and t["revoke"][bias_ref.state_of(t, p)[0]] == 0


def test_table_rule():
    t = bias_ref.build(bias_ref.toy_phrases(4096, 3000, 3, 6))
    assert bias_ref.table_max_probe(t) >= 2                    # linear probing is exercised
    assert bias_ref.table_max_probe(bias_ref.build([[1]])) == 1


# ---------------------------------------------------------------- the search
@pytest.mark.parametrize("name", ["basic", "few_classes", "peaky_merge", "neg_inf"])
def test_zero_weight_reproduces_the_unbiased_restatements(name):
    cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
    lm = lr.make_lm_case(name)[3]
    C = cs["C"]
    for K in cs["Ks"]:
        plain = cr.ctc_beam_ref_batch(z[..., :C], lens, K, 0, C - 1, cs["nbest"])
        got = br.ctc_bias_beam_ref_batch(z[..., :C], lens, K, None, 0.0, 0.0, trie, 0.0, cs["nbest"])
        for p, g in zip(plain, got):
            assert [(h, s) for h, s, am, acc, n in g["nbest"]] == p["nbest"]
            assert all(s == am and acc is None and n == bias_ref.count(trie, h) for h, s, am, acc, n in g["nbest"])
            assert (g["slack"], g["min_gap"], g["merges"], g["recreated"]) == (p["slack"], p["min_gap"], p["merges"], p["recreated"])
        fused = lr.ctc_lm_beam_ref_batch(z[..., :C], lens, K, lm, cs["lm_w"], cs["len_bonus"], cs["nbest"])
        got = br.ctc_bias_beam_ref_batch(z[..., :C], lens, K, lm, cs["lm_w"], cs["len_bonus"], trie, 0.0, cs["nbest"])
        for f, g in zip(fused, got):
            assert [e[:4] for e in g["nbest"]] == f["nbest"] and (g["slack"], g["merges"]) == (f["slack"], f["merges"])


@pytest.mark.parametrize("T,C,with_lm,bias_w,seed", [(5, 5, False, 1.5, 0), (5, 5, True, 1.0, 1), (5, 4, False, 3.0, 2), (4, 5, True, 0.7, 3),
                                                      (5, 5, False, 0.4, 4)])
def test_brute_force_on_tiny_shapes(T, C, with_lm, bias_w, seed):
    # K above the number of reachable prefixes (at most sum of 3^l, l <= T, over three emittable classes): nothing is pruned, so the provisional
    # counts decide nothing and the search is exact
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
    lm = lm_ref.toy_lm(C, 3, seed) if with_lm else None
    trie = bias_ref.build(bias_ref.toy_phrases(C, 4, seed, 3))
    want = br.brute_force(z, lm, 0.8, 0.3, trie, bias_w)
    K = 3 ** (T + 1)
    got = br.ctc_bias_beam_ref(z, K, lm, 0.8, 0.3, trie, bias_w)["nbest"]
    assert len(got) == len(want) < K
    assert got[0][0] == want[0][0]
    by_h = {h: (s, am, n) for h, s, am, n in want}
    for h, s, am, acc, n in got:
        s2, am2, n2 = by_h[h]
        assert abs(s - s2) < 1e-9 and abs(am - am2) < 1e-9 and n == n2
    assert [round(e[1], 9) for e in got] == sorted((round(e[1], 9) for e in got), reverse=True)


@pytest.mark.parametrize("name", list(br.BIAS_CASES))
def test_case_conditions(name):
    cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
    refs = br.case_refs(name)
    C = cs["C"]
    assert all(1 <= len(p) <= 64 and all(1 <= c <= C - 2 for c in p) for p in phrases) and len({tuple(p) for p in phrases}) == len(phrases)
    differs, revocations = False, 0
    for K in cs["Ks"]:
        rs = refs[K]
        # at least 3/4 of the utterances are compared on the GPU
        assert 4 * sum(not r["slack"] > 0 for r in rs) <= len(rs), (name, K, [r["slack"] for r in rs])
        for r in rs:
            for h, s, am, acc, n in r["nbest"]:
                # the count and lmacc of every returned entry are functions of its tokens alone
                assert n == bias_ref.count(trie, h) >= 0, (name, K, h)
                y = am
                if lm is not None:
                    assert acc.dtype == np.float32 and acc == lr.lmacc32(lm, h, cs["lm_w"], cs["len_bonus"])
                    y = am + float(acc) + float(lr.eos_term32(lm, h, cs["lm_w"], C - 1))
                assert s == y + float(br.bias_term32(cs["bias_w"], n))
        plain = br.unbiased_refs(BASE(name), lm is not None)[K]
        differs |= any(r["nbest"][0][0] != p["nbest"][0][0] for r, p in zip(rs, plain))
        revocations += sum(r["revocations"] for r in rs)
    assert differs, name                                        # a phrase list without effect cannot pass
    assert revocations > 0, name                                # nor a search in which no match ever breaks


def BASE(name):
    return br.BIAS_CASES[name]["base"]


def test_cases_cover_what_they_are_for():
    assert {BASE(n) for n in br.BIAS_CASES} == {"basic", "few_classes", "peaky_merge", "full_buffer", "wide_367", "neg_inf"}
    for base in {BASE(n) for n in br.BIAS_CASES}:
        assert {br.BIAS_CASES[n]["with_lm"] for n in br.BIAS_CASES if BASE(n) == base} == {False, True}
    assert 0 in br.make_bias_case("few_classes")[0]["lens"] and br.make_bias_case("full_buffer")[0]["Ks"] == [64]
    assert br.make_bias_case("wide_367")[0]["ld"] == 369 and br.make_bias_case("wide_367")[0]["Ks"] == [20]
    r = br.case_refs("peaky_merge")[3]
    assert sum(x["merges"] for x in r) > 0 and sum(x["recreated"] for x in r) > 0
    # some case holds a phrase that is a proper prefix of another
    ph = {tuple(p) for p in br.make_bias_case("basic")[4]}
    assert any(p[:k] in ph for p in ph for k in range(1, len(p)))


@pytest.mark.parametrize("mutate", ["no_revoke", "no_final_revoke", "no_retry_from_root", "bias_in_pnb"])
def test_mutated_restatements_differ(mutate):
    hit = []
    for name in ("basic", "basic_lm", "peaky_merge", "neg_inf"):
        cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
        K = cs["Ks"][-1]
        bad = br.ctc_bias_beam_ref_batch(z[..., :cs["C"]], lens, K, lm, cs["lm_w"], cs["len_bonus"], trie, cs["bias_w"], cs["nbest"], mutate=mutate)
        for r, m in zip(br.case_refs(name)[K], bad):
            same = len(r["nbest"]) == len(m["nbest"]) and all(
                a[0] == b[0] and abs(a[1] - b[1]) <= cr.tol(a[1]) and abs(a[2] - b[2]) <= cr.tol(a[2]) and a[4] == b[4]
                for a, b in zip(r["nbest"], m["nbest"]))
            if not same:
                hit.append(name)
    assert hit, mutate
