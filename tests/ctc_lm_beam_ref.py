"""CPU restatement of the LM-fused CTC prefix beam search of masr_ctc_beam_search_lm (include/masr.h) and the cases that
tests/test_ctc_lm_beam_ref_cpu.py and tests/test_hip_ctc_lm_beam_kernel.py share.  A plain helper module like ctc_beam_ref.py.

It is ctc_beam_ref.ctc_beam_ref extended with the LM: the acoustic recursion in fp64 over tuples of tokens, untouched by the LM; lmacc and
the eos term in fp32 in the written order (lm_ref's fp32 walk, then fl(fl(lm_w * lm) + len_bonus) added to the parent's lmacc), so a prefix's
lmacc has the kernel's bits.  A candidate ranks by am + lmacc.

ctc_lm_beam_ref(logits [T, C], K, lm, lm_w, len_bonus, blank, eos, nbest) -> dict:
  nbest      the re-ranked final beam, at most `nbest` tuples (tokens, final, am, lmacc): final = am + lmacc + fl(lm_w * lm(eos | h)) with
             the acoustic am in fp64, lmacc an np.float32
  slack      as ctc_beam_ref's, on the fused scores: the K-th against the (K+1)-th candidate of every frame, and adjacent entries of the first
             nbest + 1 of the re-ranked final beam.  DELTA is ctc_beam_ref.delta taken on the larger of |am| and |fused score| of both sides:
             the acoustic part is what carries the fp32 log-sum-exp error; the fp32 additions on top are two roundings (2 * 6e-8 |s|), far
             inside the 2e-5 |s| term
  min_gap, merges, recreated   as ctc_beam_ref's

`mutate` names a deliberately wrong variant (the CPU test shows that each differs from the restatement on some case):
  "lm_in_pnb"     the LM increment is added to the extension's p_nb instead of being carried apart (am then holds LM terms)
  "no_eos"        the end-of-utterance term is left out
  "bonus_on_stay" a stay adds len_bonus to its lmacc, as if the bonus were per frame
"""
import itertools
import math

import numpy as np

import ctc_beam_ref as cr
import lm_ref

NEG_INF = -math.inf
_lae = cr._lae
f32 = np.float32


def lm_inc32(lm, cache, h, c, lm_w, len_bonus):
    """fl(fl(lm_w * lm(c | h)) + len_bonus), fp32"""
    ctx = lm_ref.lm_context(lm, h)
    v = cache.get((ctx, c))
    if v is None:
        v = cache[(ctx, c)] = lm_ref.lm_logprob_ctx32(lm, ctx, c)
    return f32(f32(f32(lm_w) * v) + f32(len_bonus))


def lmacc32(lm, h, lm_w, len_bonus, cache=None):
    """lmacc(h) recomputed from the tokens alone, fp32 in the written order"""
    cache = {} if cache is None else cache
    acc = f32(0.0)
    for i, c in enumerate(h):
        acc = f32(acc + lm_inc32(lm, cache, tuple(h[:i]), c, lm_w, len_bonus))
    return acc


def eos_term32(lm, h, lm_w, eos):
    """fl(lm_w * lm(eos | h)), fp32"""
    return f32(f32(lm_w) * lm_ref.lm_logprob(lm, tuple(h), eos))


def final32(am, lmacc, eos_term):
    """the kernel's final score from an fp32 acoustic total: fl(fl(am + lmacc) + eos term)"""
    return f32(f32(f32(am) + f32(lmacc)) + f32(eos_term))


def _delta(*pairs):
    """pairs of (am, fused): DELTA on the larger magnitude of each"""
    return cr.delta(*[max(abs(a), abs(s)) for a, s in pairs])


def ctc_lm_beam_ref(logits, K, lm, lm_w, len_bonus=0.0, blank=0, eos=None, nbest=None, mutate=None):
    z = np.asarray(logits)
    assert z.dtype == np.float32 and z.ndim == 2
    T, C = z.shape
    eos = C - 1 if eos is None else eos
    assert blank == 0 and eos == C - 1 and lm["C"] == C
    nbest = K if nbest is None else nbest
    emit = [c for c in range(C) if c != blank and c != eos]
    P = min(K, len(emit))
    z64 = z.astype(np.float64)
    cache = {}
    beam = [((), 0.0, NEG_INF, -1, f32(0.0))]             # (prefix, p_b, p_nb, frame the entry's current run began, lmacc)
    slack, min_gap, merges, recreated = math.inf, math.inf, 0, 0
    for t in range(T):
        row = z64[t]
        mx = row.max()
        x = row - (mx + math.log(np.exp(row - mx).sum()))
        S = sorted(emit, key=lambda c: (-z[t, c], c))[:P]  # by acoustic logit alone: no LM in the pre-beam
        index = {e[0]: k for k, e in enumerate(beam)}
        stay = [[_lae(pb, pnb) + x[blank], pnb + x[pre[-1]] if pre else NEG_INF] for pre, pb, pnb, born, acc in beam]
        ext = []                                           # (candidate index, parent k, class, p_nb', lmacc(h + c))
        for k, (pre, pb, pnb, born, acc) in enumerate(beam):
            for j, c in enumerate(S):
                v = (pb if pre and c == pre[-1] else _lae(pb, pnb)) + x[c]
                if mutate == "lm_in_pnb" and v != NEG_INF:
                    v += float(lm_inc32(lm, cache, pre, c, lm_w, len_bonus))
                k2 = index.get(pre + (c,))
                if k2 is not None:
                    stay[k2][1] = _lae(stay[k2][1], v)
                    merges += 1
                    recreated += beam[k2][3] < born
                elif v != NEG_INF:                         # (a -inf candidate is never kept: no LM value needed)
                    nacc = f32(0.0) if mutate == "lm_in_pnb" else f32(acc + lm_inc32(lm, cache, pre, c, lm_w, len_bonus))
                    ext.append((k * (P + 1) + 1 + j, k, c, v, nacc))
        sacc = [f32(e[4] + f32(len_bonus)) if mutate == "bonus_on_stay" else e[4] for e in beam]
        # (fused score, candidate index, parent, class, am, lmacc)
        cands = [(_lae(*stay[k]) + float(sacc[k]), k * (P + 1), k, -1, _lae(*stay[k]), sacc[k]) for k in range(len(beam))]
        cands += [(v + float(nacc), i, k, c, v, nacc) for i, k, c, v, nacc in ext]
        cands = sorted((cd for cd in cands if cd[0] != NEG_INF), key=lambda cd: (-cd[0], cd[1]))
        if len(cands) > K:
            a, b = cands[K - 1], cands[K]
            slack, min_gap = min(slack, a[0] - b[0] - _delta((a[4], a[0]), (b[4], b[0]))), min(min_gap, a[0] - b[0])
        new = []
        for sc, i, k, c, am, nacc in cands[:K]:
            pre, pb, pnb, born, acc = beam[k]
            new.append((pre, stay[k][0], stay[k][1], born, nacc) if c < 0 else (pre + (c,), NEG_INF, am, t, nacc))
        beam = new
    final = []
    for rank, (pre, pb, pnb, _, acc) in enumerate(beam):
        am = _lae(pb, pnb)
        e = f32(0.0) if mutate == "no_eos" else eos_term32(lm, pre, lm_w, eos)
        final.append((pre, am + float(acc) + float(e), am, acc, rank))
    final.sort(key=lambda f: (-f[1], f[4]))
    for a, b in zip(final[:nbest], final[1:nbest + 1]):
        slack, min_gap = min(slack, a[1] - b[1] - _delta((a[2], a[1]), (b[2], b[1]))), min(min_gap, a[1] - b[1])
    return {"nbest": [f[:4] for f in final[:nbest]], "slack": slack, "min_gap": min_gap, "merges": merges, "recreated": recreated}


def ctc_lm_beam_ref_batch(logits, lens, K, lm, lm_w, len_bonus=0.0, nbest=None, mutate=None):
    """logits [B, Tp, >= C] fp32 (pass the [:, :, :C] view), lens [B]; frames past lens[b] are not read"""
    return [ctc_lm_beam_ref(np.ascontiguousarray(logits[b, :max(0, min(int(n), logits.shape[1]))]), K, lm, lm_w, len_bonus, nbest=nbest, mutate=mutate)
            for b, n in enumerate(lens)]


# ---------------------------------------------------------------- brute force (tiny shapes only)
def brute_force(logits, lm, lm_w, len_bonus=0.0):
    """every prefix over the emittable classes with its CTC likelihood by enumeration of all (blank + emittable)^T paths, its LM sum and eos
    term -> [(tokens, final, am)] sorted by final descending; prefixes no path reaches are left out"""
    z = np.asarray(logits, np.float64)
    T, C = z.shape
    eos = C - 1
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
    out = [(h, am + float(lmacc32(lm, h, lm_w, len_bonus)) + float(eos_term32(lm, h, lm_w, eos)), am) for h, am in tot.items() if am != NEG_INF]
    return sorted(out, key=lambda r: -r[1])


# ---------------------------------------------------------------- the cases
# name -> dict(base: the ctc_beam_ref.CASES shape it reuses, Ks, order, lm_seed, lm_w, len_bonus, and optionally seed / scale of the logits
# in place of the base's).  The LM is lm_ref.toy_lm(C, order, lm_seed, **lm_kw).  Seeds, scales and weights were chosen on the CPU
# (test_ctc_lm_beam_ref_cpu.py asserts both conditions) so that at least 3/4 of each case's utterances have slack > 0 for every K, and the LM
# changes the best hypothesis of at least one utterance.
def _lm_case(base, order, lm_seed, lm_w, len_bonus=0.0, Ks=None, seed=None, scale=None, lm_kw=None):
    return dict(base=base, order=order, lm_seed=lm_seed, lm_w=lm_w, len_bonus=len_bonus, Ks=Ks, seed=seed, scale=scale, lm_kw=lm_kw or {})


LM_CASES = {
    "basic": _lm_case("basic", 3, 3, 0.8),
    "basic_bonus_pos": _lm_case("basic", 3, 0, 0.8, len_bonus=0.7),
    "basic_bonus_neg": _lm_case("basic", 3, 1, 0.8, len_bonus=-0.3),
    "basic_order1": _lm_case("basic", 1, 1, 0.8),                       # no tables at all
    "few_classes": _lm_case("few_classes", 3, 0, 0.8),                  # with an enc_len 0
    "peaky_merge": _lm_case("peaky_merge", 3, 0, 0.8),                  # merging and re-creation
    "full_buffer": _lm_case("full_buffer", 4, 1, 0.8),                  # K = 64, nbest 4, order 4
    # Tp 100, K 20, ld 369.  A toy LM over 365 units gives nearly every token the unigram floor, about -6.55: at lm_w 0.3 a 60-token
    # hypothesis would carry -120 of LM score and DELTA, which grows with |score|, would exceed the gaps between candidates.  The bonus
    # cancels the floor (0.3 * 6.55 = 1.96), so fused scores stay near the acoustic ones and what is left of the LM is its preferences.
    "wide_367": _lm_case("wide_367", 3, 4, 0.3, len_bonus=1.95),
    "neg_inf": _lm_case("neg_inf", 3, 0, 0.8),
}

_made = {}


def _logits(cs):
    """ctc_beam_ref.make_case's generator on a case dict"""
    rng = np.random.default_rng(cs["seed"])
    z = np.full((cs["B"], cs["Tp"], cs["ld"]), np.nan, np.float32)
    v = (rng.standard_normal((cs["B"], cs["Tp"], cs["C"])) * cs["scale"]).astype(np.float32)
    if cs["ninf"]:
        mask = rng.random(v.shape) < cs["ninf"]
        mask[..., 0] = False                                # blank stays finite: a row of -inf alone has no log_softmax
        v[mask] = -np.inf
    z[..., :cs["C"]] = v
    for b, n in enumerate(cs["lens"]):
        z[b, n:] = np.nan                                   # padded frames are never read
    return z, np.asarray(cs["lens"], np.int32)


def make_lm_case(name):
    """-> (case dict with the base's shape fields filled in, logits fp32 [B, Tp, ld] NaN-padded as ctc_beam_ref.make_case pads them,
    lens int32 [B], the LM in lm_ref's dict form).  Built once per process and shared: callers leave the arrays unchanged."""
    if name in _made:
        return _made[name]
    lc = LM_CASES[name]
    base = dict(cr.CASES[lc["base"]])
    if lc["seed"] is not None:
        base["seed"] = lc["seed"]
    if lc["scale"] is not None:
        base["scale"] = lc["scale"]
    z, lens = _logits(base)
    cs = dict(base, **{k: lc[k] for k in ("order", "lm_seed", "lm_w", "len_bonus")})
    cs["Ks"] = lc["Ks"] or cs["Ks"]
    lm = lm_ref.toy_lm(cs["C"], lc["order"], lc["lm_seed"], **lc["lm_kw"])
    _made[name] = (cs, z, lens, lm)
    return _made[name]


_refs = {}


def case_refs(name):
    """{K: ctc_lm_beam_ref_batch of the case}, computed once per process"""
    if name not in _refs:
        cs, z, lens, lm = make_lm_case(name)
        _refs[name] = {K: ctc_lm_beam_ref_batch(z[..., :cs["C"]], lens, K, lm, cs["lm_w"], cs["len_bonus"], cs["nbest"]) for K in cs["Ks"]}
    return _refs[name]


def table_max_probe(lm):
    """the longest probe chain (slots examined) an insertion walks when masr_lm_create builds this model's tables from lm_ref.to_arrays'
    order: the builder's hash and capacity rule restated"""
    worst = 1
    for n in range(2, lm["order"] + 1):
        keys = list(lm["grams"][n - 1])
        cap, bits = 16, 4
        while cap < 2 * len(keys):
            cap, bits = cap * 2, bits + 1
        used = set()
        for g in keys:
            key = 0
            for w in g:
                key = (key << 16) | (w + 1)
            at = ((key * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - bits)
            probes = 1
            while at & (cap - 1) in used:
                at, probes = at + 1, probes + 1
            used.add(at & (cap - 1))
            worst = max(worst, probes)
    return worst
