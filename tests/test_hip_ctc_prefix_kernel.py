"""The joint beam's CTC prefix-score kernel alone (include/masr_test.h masr_test_ctc_prefix: beam_ctc_prefix_kernel on one hypothesis
row) against the literal restatement of tests/joint_beam_ref.py, on random log-probs: no encoder in between, so the tolerances are those of
fp32 log-sum-exp chains.  Covers the empty parent, repeated tokens, eos, padding, -inf candidates ahead of finite ones in a row whose list
buffer holds stale entries, and utterances longer than one 256-frame LDS chunk."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import joint_beam_ref as jr  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402

F32 = np.float32


def _lp(T, Cn, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, Cn, generator=g) * scale, dim=-1).numpy().astype(F32)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, got, want)
    f = np.isfinite(want)
    assert np.isfinite(got[f]).all(), what
    err = np.abs(got[f] - want[f])
    assert (err <= 1e-4 + 2e-5 * np.abs(want[f])).all(), (what, float(err.max()) if err.size else 0.0)


def run_kernel(x, h, cands, att_lp, att_w, ctc_w, score=-3.0):
    """x [T][C] log-probs, parent h (tuple), candidates -> (list_tok, list_score, list_psi, list_slot, states [T][n][2]); the list buffers
    start dirty (token 1, score +100) so that any position the kernel leaves unwritten shows"""
    T, Cn = x.shape
    n = len(cands)
    dev = "cuda:0"
    lp_d = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    if h:
        psi_par, (rn, rb) = jr.prefix_score(x, list(h))
        parent = torch.from_numpy(np.stack([rn, rb], axis=1).astype(F32)).to(dev)
        last = h[-1]
    else:
        psi_par, parent, last = F32(0), None, -1
    cand_d = torch.tensor(cands, dtype=torch.int32, device=dev)
    alp_d = torch.tensor(att_lp, dtype=torch.float32, device=dev)
    lt = torch.full((n,), 1, dtype=torch.int32, device=dev)
    ls = torch.full((n,), 100.0, dtype=torch.float32, device=dev)
    lps = torch.full((n,), 100.0, dtype=torch.float32, device=dev)
    lsl = torch.full((n,), 0, dtype=torch.int32, device=dev)
    out = torch.zeros(T, n, 2, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    l = lib()
    rc = l.masr_test_ctc_prefix(p(lp_d), Cn, T, last, p(parent), float(psi_par), float(score), p(cand_d), p(alp_d), n, float(att_w),
                                float(ctc_w), p(lt), p(ls), p(lps), p(lsl), p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    return lt.cpu().tolist(), ls.cpu().numpy(), lps.cpu().numpy(), lsl.cpu().tolist(), out.cpu().numpy(), psi_par


def expect(x, h, cands, att_lp, att_w, ctc_w, score, psi_par):
    eos = x.shape[1] - 1
    state = jr.prefix_score(x, list(h))[1] if h else jr.ctc_empty(x)
    chains = [c for c in cands if c > 0 and c != eos]
    sts, ps = jr.ctc_extend(x, state, tuple(h), chains) if chains else ([], [])
    by_c = {c: (sts[i], ps[i]) for i, c in enumerate(chains)}
    rows = []
    for i, c in enumerate(cands):
        if c < 0:
            continue
        st, psi = (None, jr.ctc_eos(state)) if c == eos else by_c[c]
        if psi == jr.NEG:
            continue
        js = jr.joint_score(F32(score), F32(att_lp[i]), F32(att_w), F32(ctc_w), psi, F32(psi_par))
        if js != jr.NEG:
            rows.append((float(js), i, c, float(psi)))
    rows.sort(key=lambda r: (-r[0], r[1]))
    return rows, by_c


def check(x, h, cands, att_w=0.5, ctc_w=0.5, seed=0, score=-3.0):
    g = np.random.default_rng(seed)
    att_lp = (-np.abs(g.standard_normal(len(cands))) * 3).astype(F32).tolist()
    lt, ls, lps, lsl, out, psi_par = run_kernel(x, h, cands, att_lp, att_w, ctc_w, score)
    rows, by_c = expect(x, h, cands, att_lp, att_w, ctc_w, score, psi_par)
    nv = len(rows)
    assert lt[:nv] == [r[2] for r in rows], (lt, rows)
    assert lsl[:nv] == [r[1] for r in rows], (lsl, rows)
    _close(ls[:nv], [r[0] for r in rows], "joint score")
    _close(lps[:nv], [r[3] for r in rows], "psi")
    assert lt[nv:] == [-1] * (len(cands) - nv), lt             # padding behind the finite ones, no stale entry
    assert np.isneginf(ls[nv:]).all(), ls
    for i, c in enumerate(cands):                              # every chain's (r^n, r^b) at every frame
        if c in by_c:
            _close(out[:, i, 0], by_c[c][0][0], f"r^n of candidate {i}")
            _close(out[:, i, 1], by_c[c][0][1], f"r^b of candidate {i}")
    return nv


def test_prefix_kernel_empty_parent():
    x = _lp(40, 8, 1)
    assert check(x, (), [3, 1, 7, 5, 2, -1], seed=1) == 5        # eos = 7; -1 = no candidate


def test_prefix_kernel_repeated_token_and_eos():
    x = _lp(50, 8, 2)
    assert check(x, (2, 5, 5, 3), [3, 6, 7, 1, 5, 4, 2], seed=2) == 7     # 3 repeats the parent's last token


def test_prefix_kernel_minus_inf_candidate_ahead_of_finite_ones():
    """parent (1, 2, 1, 2) over T = 5 frames: r^b_t = -inf for t < 4, so extending by its last token 2 has psi = -inf while every other
    extension is finite.  The -inf candidate sits at index 0; its row's list must hold the four finite ones, then -1 / -inf."""
    x = _lp(5, 6, 3)
    assert check(x, (1, 2, 1, 2), [2, 3, 1, 5, 4], seed=3) == 4
    assert check(x, (1, 2, 1, 2), [3, 2, 4, 1], seed=4) == 3
    x = _lp(4, 6, 4)                                           # no frame left after the parent: only eos is finite
    assert check(x, (1, 2, 1, 2), [2, 3, 5, 1, 4], seed=5) == 1


@pytest.mark.parametrize("T", [255, 256, 257, 513, 700])
def test_prefix_kernel_across_lds_chunks(T):
    x = _lp(T, 10, T, scale=3.0)
    h = (4, 4, 7, 1, 8)
    cands = [8, 1, 2, 3, 5, 6, 9, 4, 7]                         # 8 repeats; 9 = eos
    assert check(x, h, cands, 0.3, 0.7, seed=T) == 9
    assert check(x, (), cands, 0.3, 0.7, seed=T + 1) == 9


def test_prefix_kernel_wide_row():
    x = _lp(90, 100, 6)                                        # P = 96 candidates (K = 64)
    cands = list(range(1, 97))
    assert check(x, (5, 17), cands, seed=6) == 96
