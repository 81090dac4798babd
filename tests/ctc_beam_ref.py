"""CPU restatement of the CTC prefix beam search of masr_ctc_beam_search (include/masr.h), fp64 over tuples of tokens, and the
cases (shapes, seeds, logit generators) that tests/test_ctc_beam_ref_cpu.py and tests/test_hip_ctc_beam_kernel.py share.

ctc_beam_ref(logits [T, C], K, blank, eos, nbest) -> dict:
  nbest      the final beam in rank order, at most `nbest` (tokens tuple, score) pairs
  slack      min over the comparisons whose flip would change the output of  gap - DELTA(scores concerned); the GPU result is compared
             only where slack > 0 (the "min_gap > DELTA" rule).  The comparisons: the K-th against the (K+1)-th candidate of every
             frame, and adjacent scores of the first nbest + 1 entries of the final beam
  min_gap    the smallest such gap itself (for reports)
  min_class_gap  the smallest fp32 logit difference between the P-th and the (P+1)-th emittable class of a frame.  It does NOT enter slack:
             x_t(c) = z_c - lse is strictly monotone in the fp32 logit z_c, both sides order S_t by the same fp32 logits (class ascending
             on equal logits), and that comparison has no rounding in it, so it cannot flip.  Reported so a test can see it
  merges, recreated   extensions that landed on a beam entry; those whose target entered the beam at an earlier frame than the parent's
             current run did (the parent left the beam and was created again while a descendant survived)

DELTA(s) = 2 * (1e-4 + 2e-5 |s|): twice the fp32 log-sum-exp tolerance of tests/test_hip_ctc_prefix_kernel.py, either side of a comparison
may be off by it."""
import math

import numpy as np

NEG_INF = -math.inf


def tol(s):
    return 1e-4 + 2e-5 * abs(s)


def delta(*scores):
    return 2.0 * max(tol(s) for s in scores)


def _lae(a, b):
    m = max(a, b)
    if m == NEG_INF:
        return NEG_INF
    return m + math.log1p(math.exp(min(a, b) - m))


def ctc_beam_ref(logits, K, blank=0, eos=-1, nbest=None):
    z = np.asarray(logits)
    assert z.dtype == np.float32 and z.ndim == 2
    T, C = z.shape
    nbest = K if nbest is None else nbest
    emit = [c for c in range(C) if c != blank and c != eos]
    P = min(K, len(emit))
    z64 = z.astype(np.float64)
    beam = [((), 0.0, NEG_INF, -1)]                       # (prefix, p_b, p_nb, frame the entry's current run began)
    slack, min_gap, min_class_gap, merges, recreated = math.inf, math.inf, math.inf, 0, 0
    for t in range(T):
        row = z64[t]
        mx = row.max()
        x = row - (mx + math.log(np.exp(row - mx).sum()))
        order = sorted(emit, key=lambda c: (-z[t, c], c))  # (x_t descending, class ascending) == (fp32 logit descending, class ascending)
        S = order[:P]
        if len(order) > P and P > 0:
            min_class_gap = min(min_class_gap, float(z[t, order[P - 1]]) - float(z[t, order[P]]))
        index = {e[0]: k for k, e in enumerate(beam)}
        stay = []
        for pre, pb, pnb, born in beam:
            stay.append([_lae(pb, pnb) + x[blank], pnb + x[pre[-1]] if pre else NEG_INF])
        ext = []                                           # (candidate index, parent k, class, p_nb')
        for k, (pre, pb, pnb, born) in enumerate(beam):
            for j, c in enumerate(S):
                v = (pb if pre and c == pre[-1] else _lae(pb, pnb)) + x[c]
                k2 = index.get(pre + (c,))
                if k2 is not None:
                    stay[k2][1] = _lae(stay[k2][1], v)
                    merges += 1
                    recreated += beam[k2][3] < born
                else:
                    ext.append((k * (P + 1) + 1 + j, k, c, v))
        cands = [(_lae(*stay[k]), k * (P + 1), k, -1) for k in range(len(beam))] + [(v, i, k, c) for i, k, c, v in ext]
        cands = sorted((cd for cd in cands if cd[0] != NEG_INF), key=lambda cd: (-cd[0], cd[1]))
        if len(cands) > K:
            a, b = cands[K - 1][0], cands[K][0]
            slack, min_gap = min(slack, a - b - delta(a, b)), min(min_gap, a - b)
        new = []
        for sc, i, k, c in cands[:K]:
            pre, pb, pnb, born = beam[k]
            new.append((pre, stay[k][0], stay[k][1], born) if c < 0 else (pre + (c,), NEG_INF, sc, t))
        beam = new
    final = [(pre, _lae(pb, pnb)) for pre, pb, pnb, _ in beam]
    for (_, a), (_, b) in zip(final[:nbest], final[1:nbest + 1]):
        slack, min_gap = min(slack, a - b - delta(a, b)), min(min_gap, a - b)
    return {"nbest": final[:nbest], "slack": slack, "min_gap": min_gap, "min_class_gap": min_class_gap, "merges": merges,
            "recreated": recreated}


def ctc_beam_ref_batch(logits, lens, K, blank=0, eos=-1, nbest=None):
    """logits [B, Tp, >= C] fp32 (only [:, :, :C] is read: pass the view), lens [B]; frames past lens[b] are not read"""
    return [ctc_beam_ref(np.ascontiguousarray(logits[b, :max(0, min(int(n), logits.shape[1]))]), K, blank, eos, nbest) for b, n in enumerate(lens)]


# ---------------------------------------------------------------- the cases of the GPU kernel test
# name -> dict(B, Tp, C, K list, lens, eos, scale, seed, ld (None = C), ninf (share of emittable logits set to -inf))
# The logits are randn * scale of a seeded numpy generator.  The seeds are chosen on the CPU (test_ctc_beam_ref_cpu.py) so that at least
# 3/4 of each case's utterances have slack > 0; the scales keep a frame's candidates apart: with flat rows the long or wide cases nearly always have
# some frame whose K-th and (K+1)-th candidates are closer than DELTA, and a 64-long N-best list nearly always has two adjacent scores
# that close (the K = 64 case therefore returns 4 of its 64 entries).
def _case(B, Tp, C, Ks, lens, seed, eos="last", scale=1.0, ld=None, ninf=0.0, nbest=None):
    return dict(B=B, Tp=Tp, C=C, Ks=Ks, lens=lens, seed=seed, eos=C - 1 if eos == "last" else eos, scale=scale, ld=ld or C, ninf=ninf, nbest=nbest)


CASES = {
    "basic": _case(3, 40, 12, [1, 4, 8], [1, 40, 23], seed=13),
    "basic_nbest2": _case(3, 40, 12, [8], [1, 40, 23], seed=13, nbest=2),
    "few_classes": _case(4, 24, 5, [8], [24, 7, 16, 0], seed=2),                       # P = C - 2 = 3 < K: fewer than K live entries
    "peaky_merge": _case(4, 30, 4, [3], [30, 30, 30, 30], seed=3, scale=4.0),          # merging and re-creation
    "full_buffer": _case(4, 30, 70, [64], [30, 6, 9, 4], seed=4, scale=6.0, nbest=4),  # 64 * 65 candidates from frame 2 on
    "wide_367": _case(2, 100, 367, [20], [100, 61], seed=9, scale=12.0, ld=369),
    "wide_4096": _case(2, 100, 4096, [20], [100, 37], seed=8, scale=12.0, ld=4099),
    "no_eos": _case(4, 40, 12, [4], [40, 1, 17, 33], seed=8, eos=-1),
    "neg_inf": _case(4, 30, 12, [8], [30, 30, 9, 21], seed=8, ninf=0.4),
}


def make_case(name):
    """-> (case dict, logits fp32 [B, Tp, ld] with NaN in the padding columns and frames, lens int32 [B])"""
    cs = CASES[name]
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
    return cs, z, np.asarray(cs["lens"], np.int32)
