"""The kernels of n-gram LM shallow fusion alone (lm.hip) through include/masr_test.h: the LM's score rule
(masr_test_lm_score) bit for bit against the fp32-ordered restatement of tests/lm_ref.py, what masr_lm_create refuses, and the beam's
LM step kernel (masr_test_beam_lm_topk) on random logits against numpy."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import lm_ref  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402

DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_LMS = {}


def toy(C_, order, seed=1):
    """(dict form, NGramLM) of the toy model; the big vocabularies draw their stream from few units so that n-grams repeat"""
    key = (C_, order, seed)
    if key not in _LMS:
        kw = dict(n_sent=60, max_len=9)
        if C_ == 367:
            kw = dict(n_sent=500, max_len=12, sharp=1.0)    # > 2000 distinct bigrams
        elif C_ > 367:
            kw = dict(n_sent=200, max_len=12, active=48)
        d = lm_ref.toy_lm(C_, order, seed, **kw)
        _LMS[key] = (d, NGramLM(order, C_, *lm_ref.to_arrays(d)))
    return _LMS[key]


def contexts(d, rng, n_each=12):
    """contexts (oldest first) of every kind: full and seen, shorter than N - 1 (<s> only, <s> + tokens), unseen at every length"""
    order, C_ = d["order"], d["C"]
    w = order - 1
    out = [()] if w == 0 else []
    for k in range(1, w + 1):
        seen = [g for g in d["grams"][k - 1] if C_ - 1 not in g]
        full = [g for g in seen if g[0] != 0] if k == w else []
        short = [g for g in seen if g[0] == 0]              # starts at <s>: a hypothesis of k - 1 tokens
        for pool in (full, short):
            for i in rng.permutation(len(pool))[:n_each]:
                out.append(pool[i])
        if k == w:
            for _ in range(n_each):                         # random units: unseen from length 2 on (seen tails, unseen heads included)
                out.append(tuple(int(t) for t in rng.randint(1, C_ - 1, size=k)))
            for g in full[:n_each]:                         # a seen tail under an unseen head
                out.append((int(rng.randint(1, C_ - 1)),) + g[1:])
        out.append((0,) + tuple(int(t) for t in rng.randint(1, C_ - 1, size=k - 1)))
    return out


@pytest.mark.parametrize("C_", [12, 367])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_lm_score_bit_for_bit(L, order, C_):
    d, lm = toy(C_, order)
    assert lm.counts == [len(g) for g in d["grams"]] and lm.device_bytes > 0
    rng = np.random.RandomState(100 * order + C_)
    ctxs = contexts(d, rng)
    w = order - 1
    if w:
        assert {len(c) for c in ctxs} == set(range(1, w + 1))
        assert any(len(c) == w and c not in d["grams"][w - 1] for c in ctxs) or w == 1      # unseen full contexts
    R = len(ctxs)
    arr = np.full((R, max(w, 1)), -1, dtype=np.int32)
    for r, c in enumerate(ctxs):
        if c:
            arr[r, w - len(c):w] = c
    ctx_d = torch.from_numpy(arr[:, :w].copy()).to(DEV) if w else None
    out = torch.full((R, C_), float("nan"), device=DEV)
    _cabi.check(L.masr_test_lm_score(lm.h, P(ctx_d), R, P(out), S()), "masr_test_lm_score")
    got = out.cpu().numpy()
    want = np.stack([lm_ref.lm_row32(d, c) for c in ctxs])
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))
    assert bad[0].size == 0, (ctxs[bad[0][0]], int(bad[1][0]), got[bad[0][0], bad[1][0]], want[bad[0][0], bad[1][0]])
    if order >= 2:                                          # hits and backoffs both occurred
        hits = sum((c[-1:] + (k,)) in d["grams"][1] for c in ctxs for k in range(C_))
        assert 0 < hits < R * C_
    if C_ == 367 and order >= 2:
        # linear probing was exercised: with > 2000 bigrams in a table of 4096 or 8192 slots some insertion met an occupied slot
        assert lm.counts[1] >= 2000, lm.counts
        assert L.masr_test_lm_max_probe(lm.h) >= 2


def test_lm_score_refuses_bad_contexts(L):
    d, lm = toy(12, 3)
    out = torch.zeros(2, 12, device=DEV)
    for bad in ([[3, -1], [1, 2]], [[1, 12], [1, 2]], [[-2, 1], [1, 2]]):
        ctx = torch.tensor(bad, dtype=torch.int32, device=DEV)
        assert L.masr_test_lm_score(lm.h, P(ctx), 2, P(out), S()) != 0
        assert b"masr_test_lm_score" in L.masr_last_error()


def _create(L, order, C_, grams, logp, backoff):
    g = [np.ascontiguousarray(np.array(a, dtype=np.int32).reshape(-1, n + 1)) for n, a in enumerate(grams)]
    lp = [np.ascontiguousarray(a, dtype=np.float32) for a in logp]
    bo = [np.ascontiguousarray(a, dtype=np.float32) for a in backoff]
    ptr = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])  # noqa: E731
    return L.masr_lm_create(order, C_, (C.c_int64 * len(g))(*[len(a) for a in g]), ptr(g), ptr(lp), ptr(bo))


def test_lm_create_refusals(L):
    C_ = 5
    uni = [[c] for c in range(C_)]
    ulp, ubo = [-1.0] * C_, [-0.5] * C_
    ok = dict(grams=[uni, [[0, 1], [1, 2], [2, 4]]], logp=[ulp, [-0.1, -0.2, -0.3]], backoff=[ubo, [0.0, 0.0, 0.0]])
    h = _create(L, 2, C_, **ok)
    assert h and L.masr_lm_bytes(h) > 0
    L.masr_lm_destroy(h)

    def refused(msg, order=2, C__=C_, **kw):
        args = dict(ok, **kw)
        assert not _create(L, order, C__, **args), msg
        assert msg.encode() in L.masr_last_error(), (msg, L.masr_last_error())

    refused("duplicate n-gram", grams=[uni, [[0, 1], [1, 2], [0, 1]]])
    refused("duplicate n-gram", grams=[[[0], [1], [2], [3], [3]], ok["grams"][1]])
    refused("outside [0, C - 1]", grams=[uni, [[0, 1], [1, 5], [2, 4]]])
    refused("outside [0, C - 1]", grams=[uni, [[0, 1], [-1, 2], [2, 4]]])
    refused("</s> may only be the last", grams=[uni, [[0, 1], [4, 2], [2, 4]]])
    refused("<s> may only be the first", grams=[uni, [[0, 1], [1, 0], [2, 4]]])
    refused("finite and <= 0", logp=[ulp, [-0.1, 0.2, -0.3]])
    refused("finite and <= 0", logp=[ulp, [-0.1, float("nan"), -0.3]])
    refused("finite and <= 0", logp=[ulp, [-0.1, float("-inf"), -0.3]])
    refused("finite and <= 0", backoff=[[-0.5, 0.5, -0.5, -0.5, -0.5], [0.0, 0.0, 0.0]])
    refused("missing unigram", grams=[uni[:4], ok["grams"][1]], logp=[ulp[:4], ok["logp"][1]], backoff=[ubo[:4], ok["backoff"][1]])
    refused("order must be in [1, 4]", order=0)
    refused("order must be in [1, 4]", order=5)
    refused("[2, 65535]", C__=65536)
    with pytest.raises(_cabi.MasrError, match="duplicate"):
        NGramLM(2, C_, [uni, [[0, 1], [0, 1]]], [ulp, [-0.1, -0.2]], [ubo, [0.0, 0.0]])


# ---------------------------------------------------------------- the step kernel
def _hyp(tok_hist, par_hist, r, t):
    h, row = [], r
    for s in range(t - 1, 0, -1):
        h.append(int(tok_hist[s - 1, row]))
        row = int(par_hist[s - 1, row])
    return tuple(reversed(h))


def run_topk(L, C_, order, B, K, t, lm_w, seed):
    d, lm = toy(C_, order)
    rng = np.random.RandomState(seed)
    R = B * K
    ld = (C_ + 127) // 128 * 128 + (128 if C_ % 128 == 0 else 0)      # ld > C always
    z = np.full((R, ld), 100.0, dtype=F32)                  # a pad column that was read would win every list
    z[:, :C_] = (3.0 * rng.randn(R, C_)).astype(F32)
    score = (-20.0 * rng.rand(R)).astype(F32)
    dead = int(rng.randint(R)) if R > 1 else -1
    if dead >= 0:
        score[dead] = -np.inf
    minlen = np.where(rng.rand(B) < 0.5, 0, t + 1).astype(np.int32)     # about half of the utterances may not end yet
    pool = sorted({w for g in d["grams"][min(1, order - 1)] for w in g if 0 < w < C_ - 1})      # units the LM has seen
    tok_hist = np.array(pool, dtype=np.int32)[rng.randint(len(pool), size=(max(t - 1, 1), R))]
    par_hist = (np.arange(R) // K * K)[None, :] + rng.randint(K, size=(max(t - 1, 1), R))
    par_hist = par_hist.astype(np.int32)
    dz, ds, dm = torch.from_numpy(z).to(DEV), torch.from_numpy(score).to(DEV), torch.from_numpy(minlen).to(DEV)
    dt, dp = (torch.from_numpy(tok_hist).to(DEV), torch.from_numpy(par_hist).to(DEV)) if t > 1 else (None, None)
    lt = torch.full((R, K), -7, dtype=torch.int32, device=DEV)
    ls = torch.full((R, K), float("nan"), device=DEV)
    _cabi.check(L.masr_test_beam_lm_topk(lm.h, float(lm_w), B, K, t, P(dm), P(dz), ld, P(ds), P(dt), P(dp), P(lt), P(ls), S()),
                "masr_test_beam_lm_topk")
    lt, ls = lt.cpu().numpy(), ls.cpu().numpy()
    # the reference: lp and the sums in fp64 on the fp32 logits; the LM term is the fp32-ordered restatement's value
    n_pos = n_ok = 0
    rows = {}
    for r in range(R):
        if r == dead:
            assert (lt[r] == -1).all() and np.isneginf(ls[r]).all(), (r, lt[r], ls[r])
            continue
        h = _hyp(tok_hist, par_hist, r, t)
        assert len(h) == t - 1
        ctx = lm_ref.lm_context(d, h)
        if ctx not in rows:
            rows[ctx] = lm_ref.lm_row32(d, ctx).astype(np.float64)
        zr = z[r, :C_].astype(np.float64)
        lp = zr - (zr.max() + math.log(np.exp(zr - zr.max()).sum()))
        f = lp + float(F32(lm_w)) * rows[ctx]
        if minlen[r // K] > t - 1:
            f[C_ - 1] = -np.inf
        order_ref = np.lexsort((np.arange(C_), -f))[:K]
        n_live = min(K, int(np.isfinite(f).sum()))
        assert (lt[r, n_live:] == -1).all() and np.isneginf(ls[r, n_live:]).all()
        fs = f[order_ref]
        for i in range(n_live):
            c = int(lt[r, i])
            assert 0 <= c < C_ and not (c == C_ - 1 and minlen[r // K] > t - 1), (r, i, c)
            want = float(score[r]) + f[c]
            assert abs(float(ls[r, i]) - want) <= 1e-5 + 1e-6 * abs(want), (r, i, c, float(ls[r, i]), want)
            n_pos += 1
            clear = (i == 0 or fs[i - 1] - fs[i] > 1e-4) and (i + 1 >= len(fs) or fs[i] - fs[i + 1] > 1e-4)
            if clear:
                n_ok += 1
                assert c == int(order_ref[i]), (r, i, c, int(order_ref[i]), fs[max(i - 1, 0):i + 2])
        assert len(set(lt[r, :n_live].tolist())) == n_live
        if n_live > 1:                                      # the list is in score order
            assert (np.diff(ls[r, :n_live]) <= 0).all()
    return n_pos, n_ok, len(rows)


GEOM = [(1, 1), (5, 1), (16, 4), (1, 64)]                 # (B, K): 1, 5, 64 and 64 rows


@pytest.mark.parametrize("C_, order", [(12, 3), (12, 1), (12, 4), (367, 3), (367, 2), (4096, 3), (4096, 4)])
def test_beam_lm_topk(L, C_, order):
    steps = (1, 2, order + 1)
    weights = (0.0, 0.5, 2.0)
    cases = []
    if C_ == 12:
        cases = [(B, K, t, w) for (B, K) in GEOM for t in steps for w in weights]
    elif C_ == 367:
        cases = [(B, K, t, weights[(i + j) % 3]) for i, (B, K) in enumerate(GEOM) for j, t in enumerate(steps)]
    else:                                                   # the reference walks 4096 classes per distinct context: a few cases
        cases = [(5, 1, 1, 0.5), (16, 4, order + 1, 2.0), (1, 64, 2, 0.0)]
    n_pos = n_ok = n_ctx = 0
    for i, (B, K, t, w) in enumerate(cases):
        a, b, c = run_topk(L, C_, order, B, K, t, w, seed=1000 * C_ + 10 * i + order)
        n_pos += a; n_ok += b; n_ctx += c
    print(f"C = {C_}, order {order}: {len(cases)} launches, {n_ok} of {n_pos} list positions have neighbours > 1e-4 apart; {n_ctx} distinct contexts")
    assert n_ok >= 0.9 * n_pos, (n_ok, n_pos)
