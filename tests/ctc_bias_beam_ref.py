"""CPU restatement of the phrase-biased CTC prefix beam search of masr_ctc_beam_search_bias (include/masr.h) and the cases that
tests/test_ctc_bias_beam_ref_cpu.py and tests/test_hip_ctc_bias_beam_kernel.py share.  A plain helper module like ctc_lm_beam_ref.py.

It is ctc_lm_beam_ref.ctc_lm_beam_ref extended with the state (node, credited tokens) of bias_ref's automaton; `lm` may be None, and then it
is ctc_beam_ref.ctc_beam_ref extended the same way (no lmacc, no eos term).  The acoustic recursion is fp64 and untouched; lmacc and the eos
term are fp32 in the written order; the bias term is fl(bias_w * (float)n), fp32.  A candidate ranks by am + lmacc + bias term of the
provisional count; the final beam is re-ranked by am + lmacc + eos term + bias term of n_final.

ctc_bias_beam_ref(logits [T, C], K, lm, lm_w, len_bonus, trie, bias_w, nbest) -> dict:
  nbest        the re-ranked final beam, at most `nbest` tuples (tokens, final, am, lmacc, n_final); lmacc is None without an LM
  slack, min_gap, merges, recreated   as ctc_lm_beam_ref's.  DELTA is ctc_lm_beam_ref._delta, on the larger of |am| and |ranking score| of both
               sides: the bias term adds two roundings of exact inputs (an integer count, a weight) on top of the LM's two, 4 * 6e-8 |s| in
               all, still far inside DELTA's 2e-5 |s| term
  revocations  kept extensions whose token broke a match with unearned tokens pending, plus returned entries that end inside one

`mutate` names a deliberately wrong variant (the CPU test shows that each differs from the restatement on some case):
  "no_revoke"           a broken match keeps its unearned tokens
  "no_final_revoke"     the match that is unfinished at the end of the utterance keeps them
  "no_retry_from_root"  the token that broke a match is not tried as the start of a new one
  "bias_in_pnb"         the bias increment is added to the extension's p_nb instead of the ranking alone (am then holds bias terms)
"""
import itertools
import math

import numpy as np

import bias_ref
import ctc_beam_ref as cr
import ctc_lm_beam_ref as lr

NEG_INF = -math.inf
_lae = cr._lae
_delta = lr._delta
f32 = np.float32


def bias_term32(bias_w, n):
    """fl(bias_w * (float)n), fp32"""
    return f32(f32(bias_w) * f32(n))


def final32(am, lmacc, eos_term, bias_w, n):
    """the kernel's final score from an fp32 acoustic total: fl(y + fl(bias_w * n)), y = fl(fl(am + lmacc) + eos term) or, without an LM, am"""
    y = f32(am) if lmacc is None else lr.final32(am, lmacc, eos_term)
    return f32(y + bias_term32(bias_w, n))


def ctc_bias_beam_ref(logits, K, lm, lm_w, len_bonus, trie, bias_w, blank=0, eos=None, nbest=None, mutate=None):
    z = np.asarray(logits)
    assert z.dtype == np.float32 and z.ndim == 2
    T, C = z.shape
    eos = C - 1 if eos is None else eos
    assert blank == 0 and eos == C - 1 and (lm is None or lm["C"] == C)
    nbest = K if nbest is None else nbest
    emit = [c for c in range(C) if c != blank and c != eos]
    P = min(K, len(emit))
    z64 = z.astype(np.float64)
    cache = {}
    zero = f32(0.0)
    smut = mutate if mutate in ("no_revoke", "no_retry_from_root") else None
    inc = (lambda pre, c: lr.lm_inc32(lm, cache, pre, c, lm_w, len_bonus)) if lm is not None else (lambda pre, c: zero)
    bt = lambda n: float(bias_term32(bias_w, n))  # noqa: E731
    beam = [((), 0.0, NEG_INF, -1, zero, bias_ref.ROOT)]      # (prefix, p_b, p_nb, frame the entry's current run began, lmacc, bias state)
    slack, min_gap, merges, recreated = math.inf, math.inf, 0, 0
    revocations = 0
    for t in range(T):
        row = z64[t]
        mx = row.max()
        x = row - (mx + math.log(np.exp(row - mx).sum()))
        S = sorted(emit, key=lambda c: (-z[t, c], c))[:P]  # by acoustic logit alone: neither the LM nor the phrases in the pre-beam
        index = {e[0]: k for k, e in enumerate(beam)}
        stay = [[_lae(pb, pnb) + x[blank], pnb + x[pre[-1]] if pre else NEG_INF] for pre, pb, pnb, born, acc, st in beam]
        ext = []                                           # (candidate index, parent k, class, p_nb', lmacc(h + c), state(h + c), revoked)
        for k, (pre, pb, pnb, born, acc, st) in enumerate(beam):
            for j, c in enumerate(S):
                v = (pb if pre and c == pre[-1] else _lae(pb, pnb)) + x[c]
                nst = bias_ref.step(trie, st, c, smut)
                if mutate == "bias_in_pnb" and v != NEG_INF:
                    v += bt(nst[1]) - bt(st[1])
                k2 = index.get(pre + (c,))
                if k2 is not None:
                    stay[k2][1] = _lae(stay[k2][1], v)
                    merges += 1
                    recreated += beam[k2][3] < born
                elif v != NEG_INF:                         # (a -inf candidate is never kept: no LM value and no step needed)
                    ext.append((k * (P + 1) + 1 + j, k, c, v, f32(acc + inc(pre, c)), nst, bias_ref.revoked_by(trie, st, c) > 0))
        rank_bias = (lambda st: 0.0) if mutate == "bias_in_pnb" else (lambda st: bt(st[1]))
        # (ranking score, candidate index, parent, class, am, lmacc, state, revoked)
        cands = [(_lae(*stay[k]) + float(e[4]) + rank_bias(e[5]), k * (P + 1), k, -1, _lae(*stay[k]), e[4], e[5], False) for k, e in enumerate(beam)]
        cands += [(v + float(nacc) + rank_bias(nst), i, k, c, v, nacc, nst, rv) for i, k, c, v, nacc, nst, rv in ext]
        cands = sorted((cd for cd in cands if cd[0] != NEG_INF), key=lambda cd: (-cd[0], cd[1]))
        if len(cands) > K:
            a, b = cands[K - 1], cands[K]
            slack, min_gap = min(slack, a[0] - b[0] - _delta((a[4], a[0]), (b[4], b[0]))), min(min_gap, a[0] - b[0])
        new = []
        for sc, i, k, c, am, nacc, nst, rv in cands[:K]:
            pre, pb, pnb, born, acc, st = beam[k]
            new.append((pre, stay[k][0], stay[k][1], born, nacc, nst) if c < 0 else (pre + (c,), NEG_INF, am, t, nacc, nst))
            revocations += rv
        beam = new
    final = []
    for rank, (pre, pb, pnb, _, acc, st) in enumerate(beam):
        am = _lae(pb, pnb)
        e = lr.eos_term32(lm, pre, lm_w, eos) if lm is not None else zero
        nf = bias_ref.n_final(trie, st, mutate)
        fin = am + float(acc) + float(e) + (0.0 if mutate == "bias_in_pnb" else bt(nf))
        final.append((pre, fin, am, acc if lm is not None else None, nf, rank, trie["revoke"][st[0]] > 0))
    final.sort(key=lambda f: (-f[1], f[5]))
    for a, b in zip(final[:nbest], final[1:nbest + 1]):
        slack, min_gap = min(slack, a[1] - b[1] - _delta((a[2], a[1]), (b[2], b[1]))), min(min_gap, a[1] - b[1])
    revocations += sum(f[6] for f in final[:nbest])
    return {"nbest": [f[:5] for f in final[:nbest]], "slack": slack, "min_gap": min_gap, "merges": merges, "recreated": recreated,
            "revocations": revocations}


def ctc_bias_beam_ref_batch(logits, lens, K, lm, lm_w, len_bonus, trie, bias_w, nbest=None, mutate=None):
    """logits [B, Tp, >= C] fp32 (pass the [:, :, :C] view), lens [B]; frames past lens[b] are not read"""
    return [ctc_bias_beam_ref(np.ascontiguousarray(logits[b, :max(0, min(int(n), logits.shape[1]))]), K, lm, lm_w, len_bonus, trie, bias_w, nbest=nbest,
                              mutate=mutate) for b, n in enumerate(lens)]


# ---------------------------------------------------------------- brute force (tiny shapes only)
def brute_force(logits, lm, lm_w, len_bonus, trie, bias_w):
    """every prefix over the emittable classes with its CTC likelihood by enumeration of all (blank + emittable)^T paths, its LM sum and eos
    term (lm None: neither) and the bias term of its n_final -> [(tokens, final, am, n_final)] sorted by final descending"""
    z = np.asarray(logits, np.float64)
    T, C = z.shape
    mx = z.max(1, keepdims=True)
    lp = z - (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))
    tot = {}
    for path in itertools.product(range(C - 1), repeat=T):             # class C - 1 = eos is never on a path
        h, prev = [], 0
        for c in path:
            if c != 0 and c != prev:
                h.append(c)
            prev = c
        s = sum(lp[t, c] for t, c in enumerate(path))
        h = tuple(h)
        tot[h] = _lae(tot.get(h, NEG_INF), s)
    out = []
    for h, am in tot.items():
        if am == NEG_INF:
            continue
        y = am if lm is None else am + float(lr.lmacc32(lm, h, lm_w, len_bonus)) + float(lr.eos_term32(lm, h, lm_w, C - 1))
        n = bias_ref.count(trie, h)
        out.append((h, y + float(bias_term32(bias_w, n)), am, n))
    return sorted(out, key=lambda r: -r[1])


# ---------------------------------------------------------------- the cases
# name -> dict(base: the ctc_lm_beam_ref.LM_CASES entry whose logits, shape and LM it reuses; with_lm; bias_w; pseed: the seed of the phrase
# choice).  The phrase list of a case is cut on the CPU from the UNBIASED search's hypotheses of ranks 2 .. K (case_phrases): pieces of 2 - 4
# tokens, a third of them with one more, random token behind (a phrase the hypotheses only half match, so matches break and are revoked), plus
# every piece's first token pair where it is longer (a phrase inside a phrase).  Seeds and weights were chosen on the CPU
# (test_ctc_bias_beam_ref_cpu.py asserts all three conditions) so that at least 3/4 of each case's utterances have slack > 0 for every K,
# biasing changes the best hypothesis of at least one utterance, and at least one kept entry suffers a revocation.
def _bias_case(base, with_lm, bias_w, pseed, Ks=None):
    return dict(base=base, with_lm=with_lm, bias_w=bias_w, pseed=pseed, Ks=Ks)


BIAS_CASES = {
    "basic": _bias_case("basic", False, 1.5, 3),
    "basic_lm": _bias_case("basic", True, 1.5, 1),
    "few_classes": _bias_case("few_classes", False, 1.5, 0),
    "few_classes_lm": _bias_case("few_classes", True, 1.5, 0),
    "peaky_merge": _bias_case("peaky_merge", False, 1.5, 0),
    "peaky_merge_lm": _bias_case("peaky_merge", True, 1.5, 0),
    "full_buffer": _bias_case("full_buffer", False, 1.5, 1),
    "full_buffer_lm": _bias_case("full_buffer", True, 1.5, 0),
    "wide_367": _bias_case("wide_367", False, 1.5, 3),
    "wide_367_lm": _bias_case("wide_367", True, 1.5, 1),
    "neg_inf": _bias_case("neg_inf", False, 1.5, 0),
    "neg_inf_lm": _bias_case("neg_inf", True, 1.5, 0),
}

_made, _refs, _plain = {}, {}, {}


def unbiased_refs(base, with_lm):
    """{K: the unbiased restatement of the base case with the full beam returned}, once per process"""
    key = (base, with_lm)
    if key not in _plain:
        cs, z, lens, lm = lr.make_lm_case(base)
        zc = z[..., :cs["C"]]
        if with_lm:
            _plain[key] = {K: lr.ctc_lm_beam_ref_batch(zc, lens, K, lm, cs["lm_w"], cs["len_bonus"], K) for K in cs["Ks"]}
        else:
            _plain[key] = {K: cr.ctc_beam_ref_batch(zc, lens, K, 0, cs["C"] - 1, K) for K in cs["Ks"]}
    return _plain[key]


def case_phrases(base, with_lm, pseed, per_utt=6):
    cs = lr.make_lm_case(base)[0]
    C = cs["C"]
    rng = np.random.default_rng(1000 + pseed)
    K = max(cs["Ks"])
    seen, out = set(), []

    def add(p):
        p = tuple(int(t) for t in p)
        if p and p not in seen:
            seen.add(p)
            out.append(list(p))

    for r in unbiased_refs(base, with_lm)[K]:
        hyps = [e[0] for e in r["nbest"][1:] if len(e[0]) >= 2]
        for _ in range(per_utt if hyps else 0):
            h = hyps[int(rng.integers(len(hyps)))]
            n = int(rng.integers(2, min(4, len(h)) + 1))
            at = int(rng.integers(0, len(h) - n + 1))
            piece = tuple(h[at:at + n])
            if rng.random() < 0.34:
                piece = piece + (int(rng.integers(1, C - 1)),)
            add(piece)
            if len(piece) > 2:
                add(piece[:2])
    if not out:
        out = [[1, 2]]
    return out


def make_bias_case(name):
    """-> (case dict with the base's shape fields and lm_w / len_bonus filled in, logits fp32 [B, Tp, ld] NaN-padded, lens int32 [B], the LM in
    lm_ref's dict form or None, the phrase list, its trie).  Built once per process and shared: callers leave the arrays unchanged."""
    if name not in _made:
        bc = BIAS_CASES[name]
        cs, z, lens, lm = lr.make_lm_case(bc["base"])
        cs = dict(cs, with_lm=bc["with_lm"], bias_w=bc["bias_w"])
        cs["Ks"] = bc["Ks"] or cs["Ks"]
        phrases = case_phrases(bc["base"], bc["with_lm"], bc["pseed"])
        _made[name] = (cs, z, lens, lm if bc["with_lm"] else None, phrases, bias_ref.build(phrases))
    return _made[name]


def case_refs(name):
    """{K: ctc_bias_beam_ref_batch of the case}, computed once per process"""
    if name not in _refs:
        cs, z, lens, lm, phrases, trie = make_bias_case(name)
        _refs[name] = {K: ctc_bias_beam_ref_batch(z[..., :cs["C"]], lens, K, lm, cs["lm_w"], cs["len_bonus"], trie, cs["bias_w"], cs["nbest"])
                       for K in cs["Ks"]}
    return _refs[name]
