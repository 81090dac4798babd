"""CPU restatement of the CTC prefix beam search with the LSTM LM fused in, masr_ctc_beam_search_nlm (include/masr.h), and the cases
that tests/test_ctc_nlm_beam_ref_cpu.py and tests/test_hip_ctc_nlm_beam_kernel.py share.  A plain helper module like ctc_lm_beam_ref.py.

It is ctc_lm_beam_ref.ctc_lm_beam_ref with the LM terms taken from a callable lm_row(h) -> fp32 [C], the LM's log-softmax row after feeding
[start] + h from the zero state (default: nlm_ref.lm_row(m, h), the bf16-emulating CPU LM).  The acoustic recursion is fp64 over tuples of
tokens; lmacc and the eos term are fp32 in the written order, so with the device's own rows a prefix's lmacc has the kernel's bits.

The LM state moves the way the device moves it: per frame an array of K slots by rank; the entry kept at rank r takes the state of its PARENT's
slot of the frame before -- advanced by its token, or carried over unchanged by a stay.  A state is a function of the tokens fed, so a slot
holds that token tuple and the LM term of (entry k, class c) is lm_row(slot[k])[c].  `mutate` names a deliberately wrong variant (the CPU test
shows that each changes an N-best list):
  "own_slot"   the state is read from the entry's own rank of the frame before instead of its parent's
  "no_carry"   a stay keeps whatever state sits at its new rank (no copy); an extension is advanced from its parent's slot

ctc_nlm_beam_ref(logits [T, C], K, lm_row, lm_w, len_bonus, nbest) -> dict with nbest [(tokens, final, am, lmacc)], slack, min_gap, merges,
recreated as ctc_lm_beam_ref's, and beam_lmacc [(tokens, lmacc)] of every entry of the final beam.
"""
import itertools
import math

import numpy as np

import ctc_beam_ref as cr
import nlm_ref
from ctc_lm_beam_ref import _delta, final32

NEG_INF = -math.inf
_lae = cr._lae
f32 = np.float32
MUTATIONS = ("own_slot", "no_carry")


def default_lm_row(m):
    return lambda h: nlm_ref.lm_row(m, tuple(h))


def inc32(row, c, lm_w, len_bonus):
    """fl(fl(lm_w * lm(c | h)) + len_bonus) from h's row, fp32"""
    return f32(f32(f32(lm_w) * f32(row[c])) + f32(len_bonus))


def lmacc32(lm_row, h, lm_w, len_bonus):
    """lmacc(h) recomputed from the tokens alone, fp32 in the written order"""
    acc = f32(0.0)
    for i, c in enumerate(h):
        acc = f32(acc + inc32(lm_row(tuple(h[:i])), c, lm_w, len_bonus))
    return acc


def eos_term32(lm_row, h, lm_w, eos):
    """fl(lm_w * lm(eos | h)), fp32"""
    return f32(f32(lm_w) * f32(lm_row(tuple(h))[eos]))


def ctc_nlm_beam_ref(logits, K, lm_row, lm_w, len_bonus=0.0, nbest=None, mutate=None):
    z = np.asarray(logits)
    assert z.dtype == np.float32 and z.ndim == 2
    T, C = z.shape
    blank, eos = 0, C - 1
    nbest = K if nbest is None else nbest
    emit = [c for c in range(C) if c != blank and c != eos]
    P = min(K, len(emit))
    z64 = z.astype(np.float64)
    beam = [((), 0.0, NEG_INF, -1, f32(0.0))]             # (prefix, p_b, p_nb, frame the entry's current run began, lmacc)
    slots = [()] * K                                       # the tokens whose state each rank's slot holds
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
                k2 = index.get(pre + (c,))
                if k2 is not None:
                    stay[k2][1] = _lae(stay[k2][1], v)
                    merges += 1
                    recreated += beam[k2][3] < born
                elif v != NEG_INF:                         # (a -inf candidate is never kept: no LM value needed)
                    ext.append((k * (P + 1) + 1 + j, k, c, v, f32(acc + inc32(lm_row(slots[k]), c, lm_w, len_bonus))))
        # (fused score, candidate index, parent, class, am, lmacc)
        cands = [(_lae(*stay[k]) + float(beam[k][4]), k * (P + 1), k, -1, _lae(*stay[k]), beam[k][4]) for k in range(len(beam))]
        cands += [(v + float(nacc), i, k, c, v, nacc) for i, k, c, v, nacc in ext]
        cands = sorted((cd for cd in cands if cd[0] != NEG_INF), key=lambda cd: (-cd[0], cd[1]))
        if len(cands) > K:
            a, b = cands[K - 1], cands[K]
            slack, min_gap = min(slack, a[0] - b[0] - _delta((a[4], a[0]), (b[4], b[0]))), min(min_gap, a[0] - b[0])
        new, nslots = [], list(slots)
        for r, (sc, i, k, c, am, nacc) in enumerate(cands[:K]):
            pre, pb, pnb, born, acc = beam[k]
            new.append((pre, stay[k][0], stay[k][1], born, nacc) if c < 0 else (pre + (c,), NEG_INF, am, t, nacc))
            src = slots[r if mutate == "own_slot" else k]
            if c < 0:
                nslots[r] = slots[r] if mutate == "no_carry" else src
            else:
                nslots[r] = src + (c,)
        beam, slots = new, nslots
    final = []
    for rank, (pre, pb, pnb, _, acc) in enumerate(beam):
        am = _lae(pb, pnb)
        e = f32(f32(lm_w) * f32(lm_row(slots[rank])[eos]))
        final.append((pre, am + float(acc) + float(e), am, acc, rank))
    final.sort(key=lambda f: (-f[1], f[4]))
    for a, b in zip(final[:nbest], final[1:nbest + 1]):
        slack, min_gap = min(slack, a[1] - b[1] - _delta((a[2], a[1]), (b[2], b[1]))), min(min_gap, a[1] - b[1])
    return {"nbest": [f[:4] for f in final[:nbest]], "slack": slack, "min_gap": min_gap, "merges": merges, "recreated": recreated,
            "beam_lmacc": [(e[0], e[4]) for e in beam]}


def ctc_nlm_beam_ref_batch(logits, lens, K, lm_row, lm_w, len_bonus=0.0, nbest=None, mutate=None):
    """logits [B, Tp, >= C] fp32 (pass the [:, :, :C] view), lens [B]; frames past lens[b] are not read"""
    return [ctc_nlm_beam_ref(np.ascontiguousarray(logits[b, :max(0, min(int(n), logits.shape[1]))]), K, lm_row, lm_w, len_bonus, nbest, mutate)
            for b, n in enumerate(lens)]


# ---------------------------------------------------------------- brute force (tiny shapes only)
def brute_force(logits, lm_row, lm_w, len_bonus=0.0):
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
    out = [(h, am + float(lmacc32(lm_row, h, lm_w, len_bonus)) + float(eos_term32(lm_row, h, lm_w, eos)), am) for h, am in tot.items()
           if am != NEG_INF]
    return sorted(out, key=lambda r: -r[1])


# ---------------------------------------------------------------- the cases
# name -> dict(shape: a ctc_beam_ref.CASES name or a case dict of its own, Ks, nlm_seed, lm_w, len_bonus).  The LM is
# nlm_ref.toy_nlm(C, 16, 24, 2, nlm_seed).  Seeds and weights were chosen on the CPU with the emulated LM (test_ctc_nlm_beam_ref_cpu.py asserts
# both conditions): at least 3/4 of each case's utterances have slack > 0 for every K, and the LM changes the best hypothesis of at least one
# utterance.  ctc_beam_ref's own wide_367 (T' 100) does not qualify with this LM (near-ties of 1e-4 at scores of -30 to -200); the shorter
# "wide" replaces it and still has 367 classes, Cp = 384 and projection tiles past the first.
def _nlm_case(shape, nlm_seed, lm_w, len_bonus=0.0, Ks=None):
    return dict(shape=shape, nlm_seed=nlm_seed, lm_w=lm_w, len_bonus=len_bonus, Ks=Ks)


NLM_DIMS = (16, 24, 2)                                                   # E, H, L of the cases' LMs
NLM_CASES = {
    "basic": _nlm_case("basic", 0, 0.8),
    "basic_bonus_pos": _nlm_case("basic", 0, 0.8, len_bonus=0.7),        # one re-created prefix at K 8
    "basic_bonus_neg": _nlm_case("basic", 0, 0.8, len_bonus=-0.3),
    "few_classes": _nlm_case("few_classes", 2, 0.8),                     # an enc_len 0; one re-created prefix
    "peaky_merge": _nlm_case("peaky_merge", 0, 0.8),
    "neg_inf": _nlm_case("neg_inf", 0, 0.8),
    "full_buffer": _nlm_case("full_buffer", 0, 0.8),                     # K 64, nbest 4
    "wide": _nlm_case(cr._case(4, 24, 367, [20], [24, 24, 15, 9], seed=11, scale=12.0, ld=369), 0, 0.3, len_bonus=1.85),
}

_made = {}


def make_nlm_case(name):
    """-> (case dict with the shape fields filled in, logits fp32 [B, Tp, ld] NaN-padded as ctc_beam_ref.make_case pads them, lens int32 [B],
    the LM in nlm_ref's dict form).  Built once per process and shared: callers leave the arrays unchanged."""
    if name not in _made:
        from ctc_lm_beam_ref import _logits
        nc = NLM_CASES[name]
        base = dict(cr.CASES[nc["shape"]]) if isinstance(nc["shape"], str) else dict(nc["shape"])
        z, lens = _logits(base)
        cs = dict(base, lm_w=nc["lm_w"], len_bonus=nc["len_bonus"], nlm_seed=nc["nlm_seed"])
        cs["Ks"] = nc["Ks"] or cs["Ks"]
        _made[name] = (cs, z, lens, nlm_ref.toy_nlm(cs["C"], *NLM_DIMS, nc["nlm_seed"]))
    return _made[name]


_refs = {}


def case_refs(name):
    """{K: ctc_nlm_beam_ref_batch of the case with the emulated LM}, computed once per process"""
    if name not in _refs:
        cs, z, lens, m = make_nlm_case(name)
        row = default_lm_row(m)
        _refs[name] = {K: ctc_nlm_beam_ref_batch(z[..., :cs["C"]], lens, K, row, cs["lm_w"], cs["len_bonus"], cs["nbest"]) for K in cs["Ks"]}
    return _refs[name]
