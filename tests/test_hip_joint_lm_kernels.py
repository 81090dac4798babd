"""The step kernels of the joint beam with LM, bonus and N-best alone through include/masr_test.h:
  masr_test_joint_lm_prebeam   the fused pre-beam on random logits against numpy (as test_hip_lm_kernels.py checks beam_lm_topk), pre_lm bit
                               for bit fl(lm_w * lm32); and against masr_test_beam_lm_topk on the same inputs: one fused increment, bit for bit
  masr_test_ctc_prefix_lm      the prefix kernel with the LM term and the bonus: list_psi and the states to the tolerances of
                               test_hip_ctc_prefix_kernel.py, list_score bit for bit from the returned list_psi and the inputs in the written
                               order (a fused multiply-add shows here), and masr_test_ctc_prefix's output at pre_lm = 0, bonus = 0
  masr_test_beam_select_nbest  the select with the N-best merge and the bound stop rule: integer and compare work only, so the list, the
                               finished flags and the histories equal a Python restatement exactly"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import joint_beam_ref as jr  # noqa: E402
import joint_lm_beam_ref as jl  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from test_hip_ctc_prefix_kernel import _close, _lp  # noqa: E402
from test_hip_ctc_prefix_kernel import run_kernel as run_plain_prefix  # noqa: E402
from test_hip_lm_kernels import _hyp, toy  # noqa: E402

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


# ---------------------------------------------------------------- the fused pre-beam
def prebeam_inputs(C_, order, B, K, t, seed, minlen_on):
    """random logits (pad columns that would win every list), scores with one dead row, minlen, and histories over the LM's own tokens"""
    d, lm = toy(C_, order)
    rng = np.random.RandomState(seed)
    R, Pw, eos = B * K, max(1, 3 * K // 2), C_ - 1
    ld = (C_ + 127) // 128 * 128
    z = np.full((R, ld), 100.0, dtype=F32)                  # a pad column that was read would win every list
    z[:, :C_] = (3.0 * rng.randn(R, C_)).astype(F32)
    score = (-20.0 * rng.rand(R)).astype(F32)
    dead = int(rng.randint(R)) if R > 1 else -1
    if dead >= 0:
        score[dead] = -np.inf
    minlen = np.full(B, t + 1 if minlen_on else 0, dtype=np.int32)
    if B > 1:
        minlen[0] = 0 if minlen_on else t + 1                  # one utterance the other way
    pool = sorted({w for g in d["grams"][min(1, order - 1)] for w in g if 0 < w < C_ - 1})
    tok_hist = np.array(pool, dtype=np.int32)[rng.randint(len(pool), size=(max(t - 1, 1), R))]
    par_hist = ((np.arange(R) // K * K)[None, :] + rng.randint(K, size=(max(t - 1, 1), R))).astype(np.int32)
    return d, lm, z, score, dead, minlen, tok_hist, par_hist


def run_prebeam(L, C_, order, B, K, t, lm_w, seed, minlen_on):
    d, lm, z, score, dead, minlen, tok_hist, par_hist = prebeam_inputs(C_, order, B, K, t, seed, minlen_on)
    R, Pw, eos = B * K, max(1, 3 * K // 2), C_ - 1
    ld = z.shape[1]
    dz, ds, dm = torch.from_numpy(z).to(DEV), torch.from_numpy(score).to(DEV), torch.from_numpy(minlen).to(DEV)
    dt, dp = (torch.from_numpy(tok_hist).to(DEV), torch.from_numpy(par_hist).to(DEV)) if t > 1 else (None, None)
    pt = torch.full((R, Pw), -7, dtype=torch.int32, device=DEV)
    pl = torch.full((R, Pw), float("nan"), device=DEV)
    pm = torch.full((R, Pw), float("nan"), device=DEV)
    _cabi.check(L.masr_test_joint_lm_prebeam(lm.h, float(lm_w), B, K, t, P(dm), P(dz), ld, P(ds), P(dt), P(dp), P(pt), P(pl), P(pm), S()),
                "masr_test_joint_lm_prebeam")
    pt, pl, pm = pt.cpu().numpy(), pl.cpu().numpy(), pm.cpu().numpy()
    n_pos = n_ok = 0
    rows = {}
    for r in range(R):
        if r == dead:                                       # untouched: the prefix kernel writes a dead row's empty list
            assert (pt[r] == -7).all() and np.isnan(pl[r]).all() and np.isnan(pm[r]).all(), (r, pt[r])
            continue
        h = _hyp(tok_hist, par_hist, r, t)
        ctx = lm_ref.lm_context(d, h)
        if ctx not in rows:
            rows[ctx] = lm_ref.lm_row32(d, ctx)
        lm32 = rows[ctx]
        zr = z[r, :C_].astype(np.float64)
        lp = zr - (zr.max() + math.log(np.exp(zr - zr.max()).sum()))
        g = lp + float(F32(lm_w)) * lm32.astype(np.float64)
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
            assert bits(pm[r, i]) == bits(F32(F32(lm_w) * lm32[c])), (r, i, c, pm[r, i], lm32[c])
            n_pos += 1
            clear = (i == 0 or gs[i - 1] - gs[i] > 1e-4) and (i + 1 >= len(gs) or gs[i] - gs[i + 1] > 1e-4)
            if clear:
                n_ok += 1
                assert c == int(order_ref[i]), (r, i, c, int(order_ref[i]), gs[max(i - 1, 0):i + 2])
        assert len(set(pt[r, :n_live].tolist())) == n_live
    return n_pos, n_ok


@pytest.mark.parametrize("C_", [12, 367])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_fused_prebeam(L, order, C_):
    d, lm = toy(C_, order)
    if C_ == 367 and order >= 2:
        assert L.masr_test_lm_max_probe(lm.h) >= 2               # linear probing is exercised
    geom = [(5, 1), (3, 4), (2, 64)]                         # (B, K): P = 1, 6, 96
    steps = (1, 2, order + 1)
    weights = (0.0, 0.5, 2.0)
    n_pos = n_ok = 0
    for i, (B, K) in enumerate(geom):
        for j, t in enumerate(steps):
            a, b = run_prebeam(L, C_, order, B, K, t, weights[(i + j) % 3], seed=1000 * C_ + 100 * order + 10 * i + j, minlen_on=(i + j) % 2 == 0)
            n_pos += a; n_ok += b
    print(f"C = {C_}, order {order}: {n_ok} of {n_pos} pre-beam positions have neighbours > 1e-4 apart")
    assert n_ok >= 0.9 * n_pos, (n_ok, n_pos)


@pytest.mark.parametrize("lm_w", [0.3, 0.7])                 # inexact products: at 0.5 or 2.0 a multiply-add and two roundings agree
@pytest.mark.parametrize("C_, order, B, K, t", [(367, 3, 2, 64, 3), (12, 3, 3, 4, 2)])     # P = 96, 128 rows in two utterances; P = 6
def test_topk_and_prebeam_compose_alike(L, C_, order, B, K, t, lm_w):
    """The LM beam's top-K and the joint LM beam's pre-beam rank one row by the same f(c) = fl(lp(c) + fl(lm_w * lm(c | h))): on the same
    inputs, with score +0 (list_score is then f itself) and minlen 0, every non-blank class of a row's K-list stands in its P-list
    (P >= K + 1 and only blank is removed), list_score equals fl(pre_lp + pre_lm) bit for bit, and the common classes keep their order."""
    d, lm, z, score, dead, minlen, tok_hist, par_hist = prebeam_inputs(C_, order, B, K, t, seed=7000 + C_ + K, minlen_on=False)
    R, Pw, ld = B * K, 3 * K // 2, z.shape[1]
    assert dead >= 0 and Pw >= K + 1
    minlen[:] = 0
    score[:] = 0.0
    score[dead] = -np.inf
    dz, ds, dm = torch.from_numpy(z).to(DEV), torch.from_numpy(score).to(DEV), torch.from_numpy(minlen).to(DEV)
    dt, dp = torch.from_numpy(tok_hist).to(DEV), torch.from_numpy(par_hist).to(DEV)
    lt = torch.full((R, K), -7, dtype=torch.int32, device=DEV)
    ls = torch.full((R, K), float("nan"), device=DEV)
    pt = torch.full((R, Pw), -7, dtype=torch.int32, device=DEV)
    pl = torch.full((R, Pw), float("nan"), device=DEV)
    pm = torch.full((R, Pw), float("nan"), device=DEV)
    _cabi.check(L.masr_test_beam_lm_topk(lm.h, float(lm_w), B, K, t, P(dm), P(dz), ld, P(ds), P(dt), P(dp), P(lt), P(ls), S()), "masr_test_beam_lm_topk")
    _cabi.check(L.masr_test_joint_lm_prebeam(lm.h, float(lm_w), B, K, t, P(dm), P(dz), ld, P(ds), P(dt), P(dp), P(pt), P(pl), P(pm), S()),
                "masr_test_joint_lm_prebeam")
    lt, ls, pt, pl, pm = lt.cpu().numpy(), ls.cpu().numpy(), pt.cpu().numpy(), pl.cpu().numpy(), pm.cpu().numpy()
    n_cmp, missing, differ, disorder = 0, [], [], []
    for r in range(R):
        if r == dead:
            continue
        place = {int(c): i for i, c in enumerate(pt[r]) if c > 0}
        common = [(i, int(c)) for i, c in enumerate(lt[r]) if c > 0]
        assert len(common) >= K - 1, (r, lt[r])             # at most blank leaves the K-list
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
    assert n_cmp >= (R - 1) * (K - 1), n_cmp
    assert not missing, missing[:5]
    assert not differ, (len(differ), n_cmp, differ[:5])
    assert not disorder, disorder[:3]


# ---------------------------------------------------------------- the prefix kernel with the LM term and the bonus
def run_prefix_lm(L, x, h, cands, att_lp, pre_lm, att_w, ctc_w, bonus, score):
    """test_hip_ctc_prefix_kernel.run_kernel through masr_test_ctc_prefix_lm; the list buffers start dirty"""
    T, Cn = x.shape
    n = len(cands)
    lp_d = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    if h:
        psi_par, (rn, rb) = jr.prefix_score(x, list(h))
        parent = torch.from_numpy(np.stack([rn, rb], axis=1).astype(F32)).to(DEV)
        last = h[-1]
    else:
        psi_par, parent, last = F32(0), None, -1
    cand_d = torch.tensor(cands, dtype=torch.int32, device=DEV)
    alp_d = torch.tensor(att_lp, dtype=torch.float32, device=DEV)
    plm_d = torch.tensor(pre_lm, dtype=torch.float32, device=DEV)
    lt = torch.full((n,), 1, dtype=torch.int32, device=DEV)
    ls = torch.full((n,), 100.0, dtype=torch.float32, device=DEV)
    lps = torch.full((n,), 100.0, dtype=torch.float32, device=DEV)
    lsl = torch.full((n,), 0, dtype=torch.int32, device=DEV)
    out = torch.zeros(T, n, 2, dtype=torch.float32, device=DEV)
    _cabi.check(L.masr_test_ctc_prefix_lm(P(lp_d), Cn, T, last, P(parent), float(psi_par), float(score), P(cand_d), P(alp_d), P(plm_d), n,
                                          float(att_w), float(ctc_w), float(bonus), P(lt), P(ls), P(lps), P(lsl), P(out), S()),
                "masr_test_ctc_prefix_lm")
    return lt.cpu().tolist(), ls.cpu().numpy(), lps.cpu().numpy(), lsl.cpu().tolist(), out.cpu().numpy(), psi_par


PREFIX_CASES = [
    # (T, C, parent, candidates): eos = C - 1, -1 = no candidate
    (7, 6, (), [3, 1, 5, 4, 2, -1]),                          # the empty parent, eos among the candidates
    (7, 6, (1, 2, 1, 2, 1, 2), [2, 3, 5, 1, 4]),              # the repeated token 2 has psi = -inf (no blank frame left) and sits in front
    (7, 6, (1, 2, 1, 2, 1, 2, 1), [2, 3, 5, 4]),              # no frame left: only eos is finite
    (300, 10, (4, 4, 7, 1, 8), [8, 1, 2, 3, 5, 6, 9, 4, 7]),  # 300 frames cross the 256-frame chunk; 8 repeats, 9 = eos
    (300, 10, (), [8, 1, 2, 3, 5, 6, 9, 4, 7]),
]


@pytest.mark.parametrize("T, Cn, h, cands", PREFIX_CASES)
@pytest.mark.parametrize("bonus", [0.75, -0.5])
def test_prefix_kernel_with_lm_and_bonus(L, T, Cn, h, cands, bonus):
    x = _lp(T, Cn, T + len(h), scale=2.0 if T < 100 else 3.0)
    eos = Cn - 1
    g = np.random.default_rng(T + len(cands))
    att_lp = (-np.abs(g.standard_normal(len(cands))) * 3).astype(F32)
    pre_lm = (-np.abs(g.standard_normal(len(cands))) * 2).astype(F32)
    # irrational-looking weights: the products are inexact, so fma(att_w, lp, s) would differ from fl(s + fl(att_w * lp))
    att_w, ctc_w, score = F32(0.37), F32(0.63), F32(-3.1415927)
    lt, ls, lps, lsl, out, psi_par = run_prefix_lm(L, x, h, cands, att_lp, pre_lm, att_w, ctc_w, bonus, score)
    # the restatement: which candidates are finite, their order, psi and the states
    state = jr.prefix_score(x, list(h))[1] if h else jr.ctc_empty(x)
    chains = [c for c in cands if c > 0 and c != eos]
    sts, ps = jr.ctc_extend(x, state, tuple(h), chains) if chains else ([], [])
    by_c = {c: (sts[i], ps[i]) for i, c in enumerate(chains)}
    want = []
    for i, c in enumerate(cands):
        if c < 0:
            continue
        psi = jr.ctc_eos(state) if c == eos else by_c[c][1]
        if psi != jr.NEG:
            want.append((i, c, float(psi)))
    nv = len(want)
    assert sorted(lsl[:nv]) == [w[0] for w in want], (lsl, want)
    assert lt[nv:] == [-1] * (len(cands) - nv) and np.isneginf(ls[nv:]).all(), (lt, ls)     # padding, no stale entry
    by_slot = {w[0]: w for w in want}
    for i in range(nv):
        slot = lsl[i]
        assert lt[i] == by_slot[slot][1]
        _close([lps[i]], [by_slot[slot][2]], f"psi of slot {slot}")
        b = F32(0) if lt[i] == eos else F32(bonus)
        js = jl.score(score, att_lp[slot], att_w, ctc_w, F32(lps[i]), F32(psi_par), pre_lm[slot], b)
        assert bits(ls[i]) == bits(js), (i, slot, float(ls[i]), float(js))
    keys = [(-float(ls[i]), lsl[i]) for i in range(nv)]
    assert keys == sorted(keys)                              # score descending, then the pre-beam position
    for i, c in enumerate(cands):
        if c in by_c:
            _close(out[:, i, 0], by_c[c][0][0], f"r^n of candidate {i}")
            _close(out[:, i, 1], by_c[c][0][1], f"r^b of candidate {i}")


@pytest.mark.parametrize("T, Cn, h, cands", PREFIX_CASES)
def test_prefix_kernel_without_lm_is_the_joint_beams(L, T, Cn, h, cands):
    x = _lp(T, Cn, T + len(h), scale=2.0 if T < 100 else 3.0)
    g = np.random.default_rng(T)
    att_lp = (-np.abs(g.standard_normal(len(cands))) * 3).astype(F32).tolist()
    a = run_prefix_lm(L, x, h, cands, att_lp, [0.0] * len(cands), 0.37, 0.63, 0.0, -3.1415927)
    b = run_plain_prefix(x, h, cands, att_lp, 0.37, 0.63, -3.1415927)
    nv = sum(t >= 0 for t in b[0])
    assert a[0] == b[0] and a[3][:nv] == b[3][:nv]
    assert (bits(a[1]) == bits(b[1])).all() and (bits(a[2][:nv]) == bits(b[2][:nv])).all() and (bits(a[4]) == bits(b[4])).all()


# ---------------------------------------------------------------- the select with the N-best list
def select_ref(B, K, N, Cn, t, maxlen, bonus, lt, ls, lpsi, lslot, st):
    """one step on the state st (dict of numpy arrays, changed in place): the contract of DESIGN 5.7 on caller-given sorted row lists"""
    Pw, eos = lt.shape[1], Cn - 1
    for u in range(B):
        if st["fin"][u]:
            continue
        r0 = u * K
        cands = []
        for k in range(K):
            for h in range(Pw):
                if lt[r0 + k, h] < 0 or ls[r0 + k, h] == -np.inf:
                    break
                cands.append((ls[r0 + k, h], k, h))
        cands.sort(key=lambda e: (-float(e[0]), e[1], e[2]))
        cands = cands[:K]
        old = [(st["nb_score"][u, i], st["nb_len"][u, i], st["nb_row"][u, i]) for i in range(N) if st["nb_len"][u, i] >= 0]
        new, j, run_best = [], 0, None
        for sc, k, h in cands:
            r = r0 + k
            if lt[r, h] == eos:
                new.append((sc, t - 1, r))
                continue
            row = r0 + j
            j += 1
            st["tok"][row], st["par"][row], st["score"][row] = lt[r, h], r, sc
            st["psi"][row], st["src"][row] = lpsi[r, h], r * Pw + lslot[r, h]
            run_best = sc if run_best is None else run_best
            if t >= maxlen[u]:
                new.append((sc, t, row))
        for k in range(j, K):
            st["tok"][r0 + k], st["par"][r0 + k], st["score"][r0 + k] = 0, r0 + k, -np.inf
        merged = sorted([(e, 0, i) for i, e in enumerate(old)] + [(e, 1, i) for i, e in enumerate(new)],
                        key=lambda m: (-float(m[0][0]), m[1], m[2]))[:N]       # an old entry ended earlier: it wins a tie
        for i, (e, _, _) in enumerate(merged):
            st["nb_score"][u, i], st["nb_len"][u, i], st["nb_row"][u, i] = e
        done = j == 0 or t >= maxlen[u]
        if not done and len(merged) == N:
            bound = F32(F32(run_best) + F32(F32(maxlen[u] - t) * F32(max(bonus, 0.0))))
            done = bool(merged[N - 1][0][0] >= bound)
        if done:
            st["fin"][u] = 1


def random_lists(rng, B, K, Cn, live_rows, p_eos, fill):
    """sorted row lists [B*K][P] with ties (scores on a grid of 0.25); rows >= live_rows[u] of an utterance are empty; `fill` of each live
    row's positions are valid"""
    R, Pw = B * K, max(1, 3 * K // 2)
    lt = np.full((R, Pw), -1, np.int32)
    ls = np.full((R, Pw), -np.inf, F32)
    lpsi = rng.standard_normal((R, Pw)).astype(F32)
    lslot = np.stack([rng.permutation(Pw) for _ in range(R)]).astype(np.int32)
    for r in range(R):
        if r % K >= live_rows[r // K]:
            continue
        n = max(1, int(round(fill * Pw)))
        sc = np.sort((-0.25 * rng.randint(0, 24, size=n)).astype(F32))[::-1]
        tok = rng.randint(1, Cn - 1, size=n)
        tok[rng.rand(n) < p_eos] = Cn - 1
        lt[r, :n], ls[r, :n] = tok, sc
    return lt, ls, lpsi, lslot


@pytest.mark.parametrize("K", [1, 4, 20, 64])
@pytest.mark.parametrize("bonus", [0.5, -0.5])
def test_select_nbest(L, K, bonus):
    Cn, B = 9, 6
    for N in sorted({1, min(2, K), K}):
        rng = np.random.RandomState(100 * K + 10 * N + (bonus > 0))
        R = B * K
        t0 = 3
        # utterance 0 is finished already, 1 reaches maxlen at the second step, 2's beam shrinks, the others run on
        maxlen = np.array([9, t0 + 1, 9, 30, 30, 5], np.int32)
        st = {"fin": np.array([1, 0, 0, 0, 0, 0], np.int32), "tok": np.full(R, -5, np.int32), "par": np.full(R, -5, np.int32),
              "score": np.full(R, 7.0, F32), "psi": np.full(R, 7.0, F32), "src": np.full(R, -5, np.int32),
              "nb_score": np.full((B, N), -np.inf, F32), "nb_len": np.full((B, N), -1, np.int32),
              "nb_row": (np.arange(B) * K)[:, None].repeat(N, 1).astype(np.int32)}
        n0 = max(1, N // 2)                                 # utterance 3 starts with a half-filled list whose scores tie with new ones
        st["nb_score"][3, :n0] = np.sort((-0.25 * rng.randint(0, 8, size=n0)).astype(F32))[::-1]
        st["nb_len"][3, :n0] = 2
        st["nb_row"][3, :n0] = 3 * K + rng.randint(K, size=n0)
        fins = []
        for step in range(4):                               # several steps of ended candidates into one list
            t = t0 + step
            live = [K, K, max(1, K // 3) if step else K, K, K, K]
            lt, ls, lpsi, lslot = random_lists(rng, B, K, Cn, live, p_eos=0.3 if step < 3 else 0.9, fill=1.0 if step != 2 else 0.2)
            dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in st.items()}
            d_in = [torch.from_numpy(a).to(DEV) for a in (lt, ls, lpsi, lslot)]
            d_max = torch.from_numpy(maxlen).to(DEV)
            step_out = torch.zeros(2, dtype=torch.int32, device=DEV)
            _cabi.check(L.masr_test_beam_select_nbest(B, K, N, Cn, t, P(d_max), float(bonus), P(d_in[0]), P(d_in[1]), P(d_in[2]), P(d_in[3]),
                                                      P(dev["score"]), P(dev["psi"]), P(dev["src"]), P(dev["fin"]), P(dev["nb_score"]),
                                                      P(dev["nb_len"]), P(dev["nb_row"]), P(dev["tok"]), P(dev["par"]), P(step_out), S()),
                        "masr_test_beam_select_nbest")
            select_ref(B, K, N, Cn, t, maxlen, bonus, lt, ls, lpsi, lslot, st)
            assert step_out.cpu().tolist() == [t + 1, 0]
            for k, v in st.items():
                got = dev[k].cpu().numpy()
                same = (bits(got) == bits(v)).all() if v.dtype == F32 else (got == v).all()
                assert same, (K, N, bonus, step, k, got, v)
            fins.append(st["fin"].copy())
        assert st["fin"][1] == 1 and st["fin"][0] == 1       # the maxlen step ended utterance 1
        assert (st["nb_len"][0] == -1).all()                 # a finished utterance is not touched
        assert (st["nb_len"][1:] >= 0).any()
        print(f"K = {K}, N = {N}, bonus {bonus}: finished after each step {[int(f.sum()) for f in fins]} of {B}")
