"""The beam's row stage with LM logits alone (beam.hip beam_rows_kernel<LM logits, top-K | pre-beam>) through
masr_test_beam_nlm_rows of include/masr_test.h: caller-given decoder logits and LM logit rows, no model and no LSTM.  The twin of
test_hip_joint_lm_kernels.py's test_fused_prebeam and test_topk_and_prebeam_compose_alike:
  pre-beam       against an fp64 restatement: pre_lp and pre_lm within 1e-5 + 1e-6 |x|; a position whose neighbours in
                 g = lp + lm_w * lm are more than 1e-4 apart holds the restatement's class, and >= 0.9 of the positions are such
  compose-alike  top-K and pre-beam rank one row by the same f(c) = fl(lp(c) + fl(lm_w * lm(c))): list_score equals fl(pre_lp + pre_lm) bit for
                 bit at lm_w 0.3 and 0.7 (inexact products: a fused multiply-add on the weight shows), the common classes in one order
Decoder rows, scores (one dead row) and minlen are drawn by test_hip_joint_lm_kernels.prebeam_inputs; the LM rows are 2 * randn with column 0
(sos / blank, never a token) at -30 and pad columns that would win every list if they were read."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
from test_hip_joint_lm_kernels import prebeam_inputs  # noqa: E402

DEV = "cuda:0"
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def inputs(C_, B, K, t, seed, minlen_on):
    """prebeam_inputs' decoder rows, scores, dead row and minlen (its n-gram LM and histories are not used) + the LM logit rows [R][ld]"""
    _, _, z, score, dead, minlen, _, _ = prebeam_inputs(C_, 1, B, K, t, seed, minlen_on)
    rng = np.random.RandomState(seed + 50000)
    y = np.full(z.shape, 100.0, dtype=F32)
    y[:, :C_] = (2.0 * rng.randn(z.shape[0], C_)).astype(F32)
    y[:, 0] = -30.0
    return z, y, score, dead, minlen


def launch(L, z, y, score, minlen, lm_w, B, K, C_, t, pre):
    R, Pw, ld = B * K, max(1, 3 * K // 2), z.shape[1]
    dz, dy, ds, dm = (torch.from_numpy(a).to(DEV) for a in (z, y, score, minlen))
    if pre:
        out = (torch.full((R, Pw), -7, dtype=torch.int32, device=DEV), torch.full((R, Pw), float("nan"), device=DEV),
               torch.full((R, Pw), float("nan"), device=DEV))
        args = (None, None, *map(P, out))
    else:
        out = (torch.full((R, K), -7, dtype=torch.int32, device=DEV), torch.full((R, K), float("nan"), device=DEV))
        args = (*map(P, out), None, None, None)
    _cabi.check(L.masr_test_beam_nlm_rows(P(dy), ld, float(lm_w), B, K, C_, t, P(dm), P(dz), ld, P(ds), *args, S()), "masr_test_beam_nlm_rows")
    return tuple(o.cpu().numpy() for o in out)


def lsm64(row):
    row = row.astype(np.float64)
    return row - (row.max() + math.log(np.exp(row - row.max()).sum()))


def run_prebeam(L, C_, B, K, t, lm_w, seed, minlen_on):
    z, y, score, dead, minlen = inputs(C_, B, K, t, seed, minlen_on)
    R, Pw, eos = B * K, max(1, 3 * K // 2), C_ - 1
    pt, pl, pm = launch(L, z, y, score, minlen, lm_w, B, K, C_, t, pre=True)
    n_pos = n_ok = 0
    for r in range(R):
        if r == dead:                                       # untouched: the prefix kernel writes a dead row's empty list
            assert (pt[r] == -7).all() and np.isnan(pl[r]).all() and np.isnan(pm[r]).all(), (r, pt[r])
            continue
        lp = lsm64(z[r, :C_])
        lm = float(F32(lm_w)) * lsm64(y[r, :C_])
        g = lp + lm
        g[0] = -np.inf                                      # blank never
        no_eos = minlen[r // K] > t - 1
        if no_eos:
            g[eos] = -np.inf
        order_ref = np.lexsort((np.arange(C_), -g))[:Pw]
        n_live = min(Pw, int(np.isfinite(g).sum()))
        assert (pt[r, n_live:] == -1).all() and np.isneginf(pl[r, n_live:]).all() and (pm[r, n_live:] == 0).all(), (r, pt[r])
        gs = g[order_ref]
        for i in range(n_live):
            c = int(pt[r, i])
            assert 0 < c < C_ and not (c == eos and no_eos), (r, i, c)
            assert abs(float(pl[r, i]) - lp[c]) <= 1e-5 + 1e-6 * abs(lp[c]), (r, i, c, float(pl[r, i]), lp[c])
            assert abs(float(pm[r, i]) - lm[c]) <= 1e-5 + 1e-6 * abs(lm[c]), (r, i, c, float(pm[r, i]), lm[c])
            n_pos += 1
            clear = (i == 0 or gs[i - 1] - gs[i] > 1e-4) and (i + 1 >= len(gs) or gs[i] - gs[i + 1] > 1e-4)
            if clear:
                n_ok += 1
                assert c == int(order_ref[i]), (r, i, c, int(order_ref[i]), gs[max(i - 1, 0):i + 2])
        assert len(set(pt[r, :n_live].tolist())) == n_live
    return n_pos, n_ok


GEOM = [(5, 1), (3, 4), (2, 64)]                             # (B, K): P = 1, 6, 96
WEIGHTS = (0.0, 0.5, 2.0)


@pytest.mark.parametrize("C_", [12, 367])
def test_prebeam_with_lm_logits(L, C_):
    n_pos = n_ok = 0
    for i, (B, K) in enumerate(GEOM):
        for t in (1, 2):
            for j, lm_w in enumerate(WEIGHTS):              # both minlen cases per geometry, step and (over the geometries) weight
                a, b = run_prebeam(L, C_, B, K, t, lm_w, seed=1000 * C_ + 100 * i + 10 * t + j, minlen_on=(i + t + j) % 2 == 0)
                n_pos += a; n_ok += b
    print(f"C = {C_}: {n_ok} of {n_pos} pre-beam positions have neighbours > 1e-4 apart")
    assert n_ok >= 0.9 * n_pos, (n_ok, n_pos)


@pytest.mark.parametrize("C_, B, K, t", [(12, 3, 4, 1), (367, 2, 64, 2)])
def test_topk_with_lm_logits(L, C_, B, K, t):
    """the top-K form against the same fp64 restatement: list_score within 1e-5 + 1e-6 |x| of score + lp + lm_w * lm, the class of a clear
    position, eos skipped below minlen, blank admitted, -1 / -inf past the end and in a dead row"""
    lm_w = 0.5
    z, y, score, dead, minlen = inputs(C_, B, K, t, seed=3000 + C_, minlen_on=True)
    lt, ls = launch(L, z, y, score, minlen, lm_w, B, K, C_, t, pre=False)
    eos, n_pos, n_ok = C_ - 1, 0, 0
    for r in range(B * K):
        if r == dead:
            assert (lt[r] == -1).all() and np.isneginf(ls[r]).all()
            continue
        f = lsm64(z[r, :C_]) + lm_w * lsm64(y[r, :C_])
        no_eos = minlen[r // K] > t - 1
        if no_eos:
            f[eos] = -np.inf
        order_ref = np.lexsort((np.arange(C_), -f))[:K]
        n_live = min(K, int(np.isfinite(f).sum()))
        assert (lt[r, n_live:] == -1).all() and np.isneginf(ls[r, n_live:]).all()
        fs = f[order_ref]
        for i in range(n_live):
            c = int(lt[r, i])
            want = float(score[r]) + f[c]
            assert 0 <= c < C_ and not (c == eos and no_eos)
            assert abs(float(ls[r, i]) - want) <= 1e-5 + 1e-6 * abs(want), (r, i, c, float(ls[r, i]), want)
            n_pos += 1
            if (i == 0 or fs[i - 1] - fs[i] > 1e-4) and (i + 1 >= len(fs) or fs[i] - fs[i + 1] > 1e-4):
                n_ok += 1
                assert c == int(order_ref[i]), (r, i, c, int(order_ref[i]))
    assert n_ok >= 0.9 * n_pos, (n_ok, n_pos)


@pytest.mark.parametrize("lm_w", [0.3, 0.7])                 # inexact products: at 0.5 or 2.0 a multiply-add and two roundings agree
@pytest.mark.parametrize("C_, B, K, t", [(367, 2, 64, 2), (12, 3, 4, 2)])     # P = 96, 128 rows in two utterances; P = 6
def test_topk_and_prebeam_compose_alike(L, C_, B, K, t, lm_w):
    """On the same inputs, with score +0 (list_score is then f itself) and minlen 0, every non-blank class of a row's K-list stands in its
    P-list (P >= K + 1 and only blank is removed), list_score equals fl(pre_lp + pre_lm) bit for bit, and the common classes keep their order."""
    z, y, score, dead, minlen = inputs(C_, B, K, t, seed=7000 + C_ + K, minlen_on=False)
    R, Pw = B * K, 3 * K // 2
    assert dead >= 0 and Pw >= K + 1
    minlen[:] = 0
    score[:] = 0.0
    score[dead] = -np.inf
    lt, ls = launch(L, z, y, score, minlen, lm_w, B, K, C_, t, pre=False)
    pt, pl, pm = launch(L, z, y, score, minlen, lm_w, B, K, C_, t, pre=True)
    n_cmp, missing, differ, disorder = 0, [], [], []
    for r in range(R):
        if r == dead:
            continue
        place = {int(c): i for i, c in enumerate(pt[r]) if c > 0}
        common = [(i, int(c)) for i, c in enumerate(lt[r]) if c > 0]
        assert len(common) >= min(K, C_ - 1) - 1, (r, lt[r])     # at most blank leaves the K-list
        for i, c in common:
            if c not in place:
                missing.append((r, i, c))
                continue
            n_cmp += 1
            f = F32(pl[r, place[c]]) + F32(pm[r, place[c]])
            if bits(ls[r, i]) != bits(f):
                differ.append((r, i, c, float(ls[r, i]), float(f)))
        seq = [place[c] for _, c in common if c in place]
        if seq != sorted(seq):
            disorder.append((r, seq))
    print(f"C = {C_}, K = {K}, lm_w = {lm_w}: {n_cmp} positions compared, {len(differ)} differ, {len(missing)} missing, {len(disorder)} rows out of order")
    assert n_cmp >= (R - 1) * (min(K, C_ - 1) - 1), n_cmp
    assert not missing, missing[:5]
    assert not differ, (len(differ), n_cmp, differ[:5])
    assert not disorder, disorder[:3]


def test_refusals(L):
    z, y, score, dead, minlen = inputs(12, 3, 4, 1, 1, False)
    dz, dy, ds, dm = (torch.from_numpy(a).to(DEV) for a in (z, y, score, minlen))
    lt = torch.zeros(12, 4, dtype=torch.int32, device=DEV)
    ls = torch.zeros(12, 4, device=DEV)
    for args, msg in (((None, 128, 0.5, 3, 4, 12, 1, P(dm), P(dz), 128, P(ds), P(lt), P(ls), None, None, None), b"null pointer"),
                      ((P(dy), 128, 0.5, 3, 4, 12, 1, P(dm), P(dz), 128, P(ds), None, P(ls), None, None, None), b"null pointer"),
                      ((P(dy), 128, 0.5, 3, 4, 12, 1, P(dm), P(dz), 128, P(ds), None, None, P(lt), None, None), b"null pointer"),
                      ((P(dy), 8, 0.5, 3, 4, 12, 1, P(dm), P(dz), 128, P(ds), P(lt), P(ls), None, None, None), b"ld_lm >= C"),
                      ((P(dy), 128, 0.5, 3, 65, 12, 1, P(dm), P(dz), 128, P(ds), P(lt), P(ls), None, None, None), b"beam size must be in [1, 64]"),
                      ((P(dy), 128, 0.5, 3, 4, 12, 1, P(dm), P(dz), 8, P(ds), P(lt), P(ls), None, None, None), b"ld >= C")):
        assert L.masr_test_beam_nlm_rows(*args, S()) == -1 and msg in L.masr_last_error(), (msg, L.masr_last_error())
