"""CPU restatement of n-gram LM shallow fusion (include/masr.h masr_recog_beam_lm).  A plain helper module like beam_ref.py:
no fixtures, no tests.

The LM is a dict: {"order": N, "C": C, "grams": [per order n a dict (w_1 .. w_n) -> (logp, bo)]}, natural log, values as np.float32.
lm_logprob follows the written rule: ctx = the last min(N - 1, |h| + 1) tokens of [sos] + h; acc = 0; for k = |ctx| down to 0 with g = the
last k tokens of ctx: (g, c) an n-gram -> acc + logp and stop; else, k >= 1 and g an n-gram -> acc += bo(g).

The toy-LM generator counts n-grams of a seeded random token stream and smooths them by interpolated absolute discounting written as a
backoff model: p(w | g) = (c(g, w) - D) / c(g) + lam(g) p(w | g'), lam(g) = D n_seen(g) / c(g) for seen (g, w), backoff weight lam(g) <= 1,
unigrams add-one smoothed over all C classes.  Every conditional distribution sums to one, and every log value is <= 0.
"""
import math

import numpy as np
import torch

import beam_ref

SOS = 0
LN10 = math.log(10.0)


# ---------------------------------------------------------------- the score rule
def lm_context(lm, h):
    seq = (SOS,) + tuple(h)
    n = min(lm["order"] - 1, len(seq))
    return seq[len(seq) - n:]


def _walk(lm, ctx, c, add, zero):
    acc = zero
    for k in range(len(ctx), -1, -1):
        g = tuple(ctx[len(ctx) - k:])
        hit = lm["grams"][k].get(g + (c,))
        if hit is not None:
            return add(acc, hit[0])
        if k >= 1:
            bo = lm["grams"][k - 1].get(g)
            if bo is not None:
                acc = add(acc, bo[1])
    raise AssertionError("order 1 must be dense")


def lm_logprob_ctx32(lm, ctx, c):
    """fp32 additions in the written order, for an explicit context (oldest first)"""
    return _walk(lm, ctx, c, lambda a, b: np.float32(a + np.float32(b)), np.float32(0.0))


def lm_logprob(lm, h, c):
    """lm(c | h) in fp32, the kernels' order of additions"""
    return lm_logprob_ctx32(lm, lm_context(lm, h), c)


def lm_logprob64(lm, h, c, ctx=None):
    """the same rule in fp64"""
    return _walk(lm, lm_context(lm, h) if ctx is None else ctx, c, lambda a, b: float(a) + float(b), 0.0)


def lm_row32(lm, ctx):
    return np.array([lm_logprob_ctx32(lm, ctx, c) for c in range(lm["C"])], dtype=np.float32)


def from_arrays(a):
    """what masr_amd.lm.read_arpa returns -> the dict form"""
    grams = []
    for n in range(a.order):
        grams.append({tuple(int(w) for w in g): (np.float32(lp), np.float32(bo)) for g, lp, bo in zip(a.grams[n], a.logp[n], a.backoff[n])})
    return {"order": a.order, "C": a.C, "grams": grams}


def to_arrays(lm):
    """the dict form -> (grams, logp, backoff) lists of arrays for NGramLM, n-grams in the dict's order"""
    g = [np.array(list(d.keys()), dtype=np.int32).reshape(-1, n + 1) for n, d in enumerate(lm["grams"])]
    lp = [np.array([v[0] for v in d.values()], dtype=np.float32) for d in lm["grams"]]
    bo = [np.array([v[1] for v in d.values()], dtype=np.float32) for d in lm["grams"]]
    return g, lp, bo


# ---------------------------------------------------------------- the toy LM
def toy_stream(C, seed, n_sent=60, max_len=9, sharp=3.0, active=None):
    """sentences over the units 1 .. C - 2 (active: the first `active` of them only) from a seeded first-order chain with peaked
    transitions (so that n-grams repeat)"""
    rng = np.random.RandomState(seed)
    U = C - 2 if active is None else min(C - 2, active)
    trans = np.exp(sharp * rng.randn(U + 1, U))             # row 0: after <s>
    trans /= trans.sum(axis=1, keepdims=True)
    sents = []
    for _ in range(n_sent):
        n, prev, s = rng.randint(1, max_len + 1), 0, []
        for _ in range(n):
            prev = 1 + int(rng.choice(U, p=trans[prev]))
            s.append(prev)
        sents.append(s)
    return sents


def toy_lm_log10(C, order, seed, D=0.75, **kw):
    """-> per order n a dict (w_1 .. w_n) -> (log10 p, log10 backoff), fp64, built from toy_stream's counts"""
    eos = C - 1
    counts = [dict() for _ in range(order)]
    for s in toy_stream(C, seed, **kw):
        seq = [SOS] + s + [eos]
        for n in range(1, order + 1):
            for i in range(len(seq) - n + 1):
                g = tuple(seq[i:i + n])
                counts[n - 1][g] = counts[n - 1].get(g, 0) + 1
    total = sum(v for (w,), v in counts[0].items() if w != SOS)
    model = [dict() for _ in range(order)]                  # (p, lam) in the linear domain
    for c in range(C):
        model[0][(c,)] = [((0 if c == SOS else counts[0].get((c,), 0)) + 1.0) / (total + C), 1.0]

    def prob(ctx, c):                                       # the backoff rule on the orders built so far
        acc = 1.0
        for k in range(len(ctx), -1, -1):
            g = tuple(ctx[len(ctx) - k:])
            if g + (c,) in model[k]:
                return acc * model[k][g + (c,)][0]
            if k >= 1 and g in model[k - 1]:
                acc *= model[k - 1][g][1]
        raise AssertionError

    for n in range(2, order + 1):
        followers = {}
        for g, v in counts[n - 1].items():
            followers.setdefault(g[:-1], []).append((g[-1], v))
        for ctx, fl in followers.items():
            tot = sum(v for _, v in fl)
            lam = D * len(fl) / tot
            for w, v in fl:
                model[n - 1][ctx + (w,)] = [(v - D) / tot + lam * prob(ctx[1:], w), 1.0]
            model[n - 2][ctx][1] = lam                      # ctx was counted as an (n - 1)-gram: it is in the model
    return [{g: (math.log10(p), math.log10(lam)) for g, (p, lam) in d.items()} for d in model]


def arpa_text(model10, id2unit):
    """ARPA text of toy_lm_log10's model; repr() round-trips the fp64 values"""
    order = len(model10)
    out = ["\\data\\"] + [f"ngram {n + 1}={len(d)}" for n, d in enumerate(model10)] + [""]
    for n, d in enumerate(model10):
        out.append(f"\\{n + 1}-grams:")
        for g, (lp, bo) in d.items():
            words = " ".join(id2unit[w] for w in g)
            out.append(f"{lp!r}\t{words}" + (f"\t{bo!r}" if n + 1 < order else ""))
        out.append("")
    out.append("\\end\\")
    return "\n".join(out) + "\n"


def units(C):
    """the unit strings of a C-class model as load_units gives them: <s>, u1 .. u{C-2}, </s>"""
    return ["<s>"] + [f"u{i}" for i in range(1, C - 1)] + ["</s>"]


def toy_lm(C, order, seed, **kw):
    """the toy model as the device tables hold it: the dict form with float32(float64(log10 x) * ln 10) values"""
    m10 = toy_lm_log10(C, order, seed, **kw)
    grams = [{g: (np.float32(np.float64(lp) * LN10), np.float32(np.float64(bo) * LN10) if n + 1 < order else np.float32(0.0))
              for g, (lp, bo) in d.items()} for n, d in enumerate(m10)]
    return {"order": order, "C": C, "grams": grams}


# ---------------------------------------------------------------- the search
def fused_row(lp_row, lm, h, lm_w):
    """f(c) = fl(lp(c) + fl(lm_w * lm(c | h))) for every class, fp32, two roundings"""
    ctx = lm_context(lm, h)
    lmv = lm_row32(lm, ctx)
    return (lp_row.astype(np.float32) + (np.float32(lm_w) * lmv).astype(np.float32)).astype(np.float32)


def beam_search_lm_one(p, cfg, memory_b, mask_b, K, maxlen, minlen, lm, lm_w):
    """beam_ref.beam_search_one with the fused increment and the row order (f descending, class ascending)"""
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    running = [((), np.float32(0.0))]
    ended = []
    sel_gaps, stop_gaps = [], []
    for t in range(1, maxlen + 1):
        z = beam_ref.last_logits(p, cfg, memory_b, mask_b, [h for h, _ in running])
        lp = beam_ref.log_softmax32(z).numpy()
        cands = []
        for k, (h, ps) in enumerate(running):
            f = fused_row(lp[k], lm, h, lm_w)
            sc = (ps + f).astype(np.float32)
            for c in range(C):
                if c == eos and len(h) < minlen:
                    continue
                cands.append((float(sc[c]), k, float(f[c]), c))
        cands.sort(key=lambda x: (-x[0], x[1], -x[2], x[3]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c) in enumerate(cands[:K]):
            h = running[k][0]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), np.float32(sc)))
                if t == maxlen:
                    ended.append((sc, t, i, h + (c,)))
        running = nxt
        best_end = max((e[0] for e in ended), default=-math.inf)
        if running and ended and t < maxlen:
            stop_gaps.append(abs(best_end - float(running[0][1])))
        if not running or best_end >= float(running[0][1]):
            break
    ended.sort(key=lambda e: (-e[0], e[1], e[2]))
    end_gap = ended[0][0] - ended[1][0] if len(ended) > 1 else math.inf
    return {"tokens": list(ended[0][3]), "score": ended[0][0], "sel_gaps": sel_gaps, "stop_gaps": stop_gaps, "end_gap": end_gap}


@torch.no_grad()
def beam_search_lm(p, cfg, xs, ilens, K, lm, lm_w, min_step_ratio=0.0, max_step_ratio=1.0):
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(beam_search_lm_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], K, maxlen, minlen, lm, lm_w))
    return out


@torch.no_grad()
def greedy_lm(p, cfg, xs, ilens, lm, lm_w, min_step_ratio=0.0, max_step_ratio=1.0):
    """step-by-step arg-max of the fused increment (first maximal class; eos excluded below minlen), stopped at eos or maxlen ->
    [(tokens, score)]"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        C = p["char_trans.weight"].shape[0]
        h, s = (), np.float32(0.0)
        for t in range(1, maxlen + 1):
            z = beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [h])
            f = fused_row(beam_ref.log_softmax32(z).numpy()[0], lm, h, lm_w)
            if len(h) < minlen:
                f = f.copy(); f[C - 1] = -np.inf
            c = int(np.argmax(f))
            s = np.float32(s + f[c])
            if c == C - 1:
                break
            h = h + (c,)
        out.append((list(h), float(s)))
    return out


@torch.no_grad()
def exhaustive_lm(p, cfg, xs, ilens, lm, lm_w, min_step_ratio=0.0, max_step_ratio=1.0):
    """beam_ref.exhaustive with the fused increment (tiny vocabularies only) -> [(tokens, score)]"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    res = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        best = (-math.inf, None)
        frontier = [((), np.float32(0.0))]
        for t in range(1, maxlen + 1):
            lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [h for h, _ in frontier])).numpy()
            nxt = []
            for k, (h, ps) in enumerate(frontier):
                sc = (ps + fused_row(lp[k], lm, h, lm_w)).astype(np.float32)
                for c in range(C):
                    if c == eos:
                        if len(h) >= minlen and float(sc[c]) > best[0]:
                            best = (float(sc[c]), list(h))
                    elif t == maxlen:
                        if float(sc[c]) > best[0]:
                            best = (float(sc[c]), list(h) + [c])
                    else:
                        nxt.append((h + (c,), sc[c]))
            frontier = nxt
        res.append((best[1], best[0]))
    return res
