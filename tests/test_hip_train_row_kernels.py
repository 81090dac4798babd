"""The training step's row kernels one by one (include/masr_test.h) against the plain restatements of tests/train_rowops_ref.py: the
label-smoothed loss head (loss, accuracy count, bf16 dlogits), the full-sequence greedy arg-max, the embedding forward and backward, the
cast + dropout in front of the VGG's backward and the un-permutation of vgg2enc's weight gradient.  Operands are generated on the device
from seeded generators, the references are fp64 (or the same one or two fp32 operations) on exactly the values the kernel reads, the
dropout masks come from masr_test_dropout_mask, and every region a launch must not touch is filled with NaN and compared bit for bit
afterwards.  Every tolerance is derived next to its assert; the worst err / bound of each class is printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
import train_rowops_ref as R  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")
F32 = np.float32
FMAX = float(np.finfo(F32).max)
U24 = R.U24
WORST = {}                                                     # tolerance class -> worst err / bound seen


@pytest.fixture(scope="module")
def lib():
    yield _cabi.lib()
    print("\nworst err / bound per tolerance class:", {k: round(v, 4) for k, v in WORST.items()})


def P(t, off_bytes=0):
    return C.c_void_p(t.data_ptr() + off_bytes) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    """bitwise equality (NaN sentinels included)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    view = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}[a.dtype]
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def within(err, bound, cls, what):
    """err <= bound everywhere (no element left out); records the worst ratio of the class"""
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    assert (err <= bound).all(), (cls, what, "worst err / bound", ratio, "elements over", int((err > bound).sum()))


def keep_mask(lib, seed, site, n, p):
    keep = torch.empty(n, device=DEV)
    _cabi.check(lib.masr_test_dropout_mask(seed, site, n, p, P(keep), S()), "dropout_mask")
    return keep


# ---------------------------------------------------------------- the loss head (rowops.hip ls_ce_kernel + ls_ce_reduce)
def run_ls_ce(lib, z, gold, C_, ld, eps, grad_w, n_total, by_ptr, what, no_loss_rows=()):
    """z fp32 [rows][C_] and gold int32 [rows] on the device -> the launch on a [rows][ld] copy with NaN pads; checks everything it writes"""
    rows = z.shape[0]
    zd = torch.full((rows, ld), NAN, device=DEV)               # pad columns: NaN, never to be read
    zd[:, :C_] = z
    inv = float(F32(1.0) / F32(n_total))
    inv_d = torch.tensor([inv], device=DEV) if by_ptr else None
    dl = torch.full((rows + 2, ld), NAN, device=DEV, dtype=torch.bfloat16)     # two sentinel rows behind `rows`
    dl0 = dl.clone()
    row_loss = torch.full((rows + 2,), NAN, device=DEV)
    row_corr = torch.full((rows + 2,), -7, device=DEV, dtype=torch.int32)
    stats = torch.full((5,), NAN, device=DEV)
    # through the pointer the by-value argument is poisoned: the pointer must win (how a replayed step graph runs the kernel)
    _cabi.check(lib.masr_test_ls_ce(P(zd), ld, P(gold), rows, C_, eps, NAN if by_ptr else inv, P(inv_d), grad_w, P(dl), P(row_loss),
                                  P(row_corr), P(stats), S()), "ls_ce")
    torch.cuda.synchronize()
    ref = R.ls_ce(z, gold, eps, inv, grad_w)
    valid = ref["valid"]
    # -- untouched regions, exact zeros
    assert same_bits(dl[rows:], dl0[rows:]), ("dlogits rows >= rows written", what)
    assert torch.isnan(row_loss[rows:]).all() and (row_corr[rows:] == -7).all() and torch.isnan(stats[3:]).all(), what
    dlc = dl[:rows].cpu()
    assert (dlc[:, C_:].view(torch.int16) == 0).all(), ("pad columns C .. ld are not +0", what)
    assert (dlc[~valid].view(torch.int16) == 0).all(), ("rows with gold -1 are not +0", what)
    # -- counts: exact (logits on a grid: the arg-max is unique or an exact tie)
    assert torch.equal(row_corr[:rows].cpu(), ref["correct"]), ("row_correct", what, torch.nonzero(row_corr[:rows].cpu() != ref["correct"])[:8].tolist())
    st = stats[:3].cpu().double()
    assert float(st[1]) == float(ref["correct"].sum()), ("stats[1]", what)
    assert float(st[2]) == float(n_total), ("stats[2] != n_total", what, float(st[2]))
    # -- row_loss: fp32 sums over C.  |z| enters through sz (C terms, weight off), exp(z - mx) through se (C terms, relative -> absolute after
    # the log: weight qsum ~ 1), and lse / z_g / off sz / off C lse are each rounded a few times (8 covers the products, the differences and
    # the 1-2 ulp of __logf): the sequential bound n 2^-24 sum |terms|
    z64 = z.double().cpu()
    z64 = torch.where(torch.isfinite(z64), z64, torch.zeros_like(z64))         # (a -inf logit is no term of a finite loss)
    on, off, qsum, _ = R.ls_consts(eps, C_, inv, grad_w, torch.float64)
    lse = ref["lse"]
    zg = z64.gather(1, gold.cpu().long().clamp_min(0)[:, None])[:, 0]
    bound = U24 * (C_ * off * z64.abs().sum(1) + C_ * qsum
                   + 8.0 * (lse.abs() + zg.abs() + off * z64.sum(1).abs() + off * C_ * lse.abs() + 1.0))
    got = row_loss[:rows].cpu().double()
    fin = torch.isfinite(ref["row_loss"])
    cmp = torch.ones(rows, dtype=torch.bool)
    cmp[list(no_loss_rows)] = False                            # (used in one place only: test_ls_ce_non_finite_logits says where and why)
    within((got - ref["row_loss"]).abs()[fin & cmp], bound[fin & cmp], "row_loss", what)
    assert torch.equal(got[~fin & cmp], ref["row_loss"][~fin & cmp]), ("row_loss of the rows whose reference is infinite", what)
    # -- stats[0]: the fp32 sum of the rows' losses (rows terms) times inv_ntotal; it must not carry grad_w
    if fin.all():
        s_ref = float(ref["row_loss"].sum()) * inv
        s_bound = inv * (float(bound[valid].sum()) + (rows + 1) * U24 * float(ref["row_loss"].abs().sum()))
        within(torch.tensor([abs(float(st[0]) - s_ref)]), torch.tensor([s_bound + 1e-300]), "stats[0]", what)
    elif cmp.all():
        assert float(st[0]) == float(ref["row_loss"].sum()), what
    # -- dlogits against the fp64 value v: one bf16 ulp of v + the flush threshold + GPU_EXP_ALLOWANCE (4) x the factor by which the CPU's fp32
    # evaluation of THIS case (same logits, gold, eps, inv_ntotal, grad_w) strays from fp64, in units of |gscale| p (|z - lse| + 1) 2^-24
    # (train_rowops_ref.py dlogits_fp32_factor / dlogits_bound have the derivation; nothing is rounded up)
    ref["got"] = dlc[:, :C_].double()
    ref["bound"] = R.dlogits_bound(ref, R.dlogits_fp32_factor(z, gold, eps, inv, grad_w))
    within((ref["got"] - ref["dlogits"]).abs(), ref["bound"], "dlogits", what)
    return ref


@pytest.mark.parametrize("rows,C_,ld", R.LS_SHAPES)
def test_ls_ce(lib, rows, C_, ld):
    combos = [(e, w) for e in R.LS_EPS for w in R.LS_GRAD_W]
    for si, scale in enumerate(R.LS_SCALES):
        z, gold = R.ls_inputs(rows, C_, scale, gen(1000 * si + rows + C_), DEV)
        n_total = max(1, int((gold >= 0).sum()))
        for eps, grad_w in combos:
            for by_ptr in (False, True):                    # inv_ntotal by value and through the device pointer
                run_ls_ce(lib, z, gold, C_, ld, eps, grad_w, n_total, by_ptr, (rows, C_, ld, scale, eps, grad_w, by_ptr))


def test_ls_ce_inputs_reach_their_cases():
    """a property of the inputs (on the restatement): right and wrong ties, gold -1 / 0 / C - 1, a constant row, saturated soft-max"""
    z, gold = R.ls_inputs(640, 367, 3000.0, torch.Generator().manual_seed(1))
    ref = R.ls_ce(z, gold, 0.2, 1.0 / 560)
    assert (gold == -1).sum() == 80 and (gold == 0).sum() >= 80 and (gold == 366).sum() >= 80
    assert ref["correct"][5::16].sum() == 0 and ref["correct"][13::16].all() and ref["correct"][7::8].all()
    assert ref["correct"][4::16].all() and not ref["correct"][12::16].any()        # the constant row: arg-max 0
    assert (ref["p"].max(dim=1).values[0::8] > 0.999).float().mean() > 0.9        # saturated
    assert (ref["p"] == 0).any()                                                    # exp underflows even in fp64


@pytest.mark.parametrize("eps", R.LS_EPS)
def test_ls_ce_all_rows_ignored(lib, eps):
    """every gold -1: loss 0, dlogits all zero, n_correct 0"""
    for rows, C_, ld in ((5, 64, 64), (37, 31, 128)):
        z, _ = R.ls_inputs(rows, C_, 1.0, gen(5), DEV)
        gold = torch.full((rows,), -1, device=DEV, dtype=torch.int32)
        zd = z.contiguous() if ld == C_ else torch.cat([z, torch.full((rows, ld - C_), NAN, device=DEV)], dim=1).contiguous()
        dl = torch.full((rows, ld), NAN, device=DEV, dtype=torch.bfloat16)
        row_loss, row_corr, stats = torch.full((rows,), NAN, device=DEV), torch.full((rows,), -7, device=DEV, dtype=torch.int32), torch.full((3,), NAN, device=DEV)
        _cabi.check(lib.masr_test_ls_ce(P(zd), ld, P(gold), rows, C_, eps, float(F32(1.0) / F32(7.0)), None, 0.7, P(dl), P(row_loss), P(row_corr),
                                      P(stats), S()), "ls_ce")
        torch.cuda.synchronize()
        assert (dl.view(torch.int16) == 0).all() and (row_loss.view(torch.int32) == 0).all() and (row_corr == 0).all()
        assert stats.tolist() == [0.0, 0.0, 7.0]


def test_ls_ce_small_vocabulary_gradient_sums_to_zero(lib):
    """the true gradient of a valid row sums to zero over the classes (qsum sum p - sum q = 0); with qsum taken as 1 every element moves by
    (eps / C) p gscale -- 10 % of p at C = 2, 2.5 % at C = 8 with eps = 0.2, far above a bf16 ulp.  The element-wise check of run_ls_ce
    carries this; here the sum itself: |sum_c d_c| <= sum_c (bf16 rounding 2^-9 |d_c| + the bound's other terms)"""
    for rows, C_ in ((64, 2), (64, 8)):
        g = gen(40 + C_)
        z = torch.round(torch.randn(rows, C_, device=DEV, generator=g) * 8.0) / 8.0
        gold = torch.randint(0, C_, (rows,), device=DEV, generator=g).int()
        ref = run_ls_ce(lib, z, gold, C_, 128, 0.2, 1.0, rows, False, ("qsum", rows, C_))
        d = ref["got"]
        assert (d.sum(1).abs() <= ref["bound"].sum(1)).all(), (C_, float(d.sum(1).abs().max()))
        # what the mutated kernel would give: off by (eps / C) p gscale in every element -- outside the bound in most of them
        shift = (float(F32(0.2)) / C_) * ref["p"] * ref["gscale"]
        assert (shift > 2.0 * ref["bound"]).float().mean() > 0.5


def test_ls_ce_non_finite_logits(lib):
    """-inf in a class other than gold: with eps == 0 the plain cross entropy and its gradient are finite, with eps > 0 the loss is +inf
    (q > 0 on a class of probability 0); a row whose only value above -inf is -FLT_MAX has that class as its arg-max"""
    C_, ld = 70, 128
    g = gen(77)
    z = torch.round(torch.randn(8, C_, device=DEV, generator=g) * 8.0) / 8.0
    gold = torch.tensor([3, 69, 5, 0, 66, 2, 7, -1], device=DEV, dtype=torch.int32)
    z[0, 10] = -INF
    z[1, 0] = -INF; z[1, 65] = -INF                         # (in the second stride of lanes 0 and 1)
    z[2] = -INF; z[2, 5] = -FMAX                            # the only value above -inf: arg-max 5 = gold, loss 0
    z[4] = -INF; z[4, 66] = -FMAX
    z[5] = -INF; z[5, 2] = -3.40e38; z[5, 40] = -3.401e38   # both below the old seed -3.4e38
    # eps > 0 needs C * lse, which is outside the fp32 range for |lse| ~ FLT_MAX (an fp32 evaluation of the formula gives inf - inf there):
    # the loss of such rows is compared at eps == 0 only (exactly 0), their arg-max and gradient at every eps; at eps > 0 the same rows with
    # -1e30 in place of -FLT_MAX carry the +inf check
    zm = z.clone()
    zm[2, 5] = -1e30; zm[4, 66] = -1e30; zm[5, 2] = -1e30; zm[5, 40] = -1.001e30
    want_correct = [int(z[0].argmax() == 3), int(z[1].argmax() == 69), 1, int(z[3].argmax() == 0), 1, 1, int(z[6].argmax() == 7), 0]
    for eps in R.LS_EPS:
        for by_ptr in (False, True):
            ref = run_ls_ce(lib, z, gold, C_, ld, eps, 1.0, 7, by_ptr, ("non-finite", eps, by_ptr), no_loss_rows=() if eps == 0 else (2, 4, 5))
            assert ref["correct"].tolist() == want_correct
            assert torch.isfinite(ref["dlogits"]).all()
            if eps == 0:
                assert torch.isfinite(ref["row_loss"]).all() and ref["row_loss"][[2, 4]].tolist() == [0.0, 0.0]
            else:
                ref = run_ls_ce(lib, zm, gold, C_, ld, eps, 1.0, 7, by_ptr, ("non-finite, -1e30", eps, by_ptr))
                assert ref["correct"].tolist() == want_correct
                assert torch.isinf(ref["row_loss"]).tolist() == [True, True, True, False, True, True, False, False]


def test_ls_ce_errors(lib):
    """refused on the host before anything is launched: the outputs keep their sentinels"""
    z = torch.zeros(4, 16, device=DEV)
    dl = torch.full((4, 16), NAN, device=DEV, dtype=torch.bfloat16)
    dl0 = dl.clone()
    rl, rc, st = torch.full((4,), NAN, device=DEV), torch.full((4,), -7, device=DEV, dtype=torch.int32), torch.full((3,), NAN, device=DEV)

    def call(gold, rows=4, C_=12, ld=16):
        gd = torch.tensor(gold, device=DEV, dtype=torch.int32)
        return lib.masr_test_ls_ce(P(z), ld, P(gd), rows, C_, 0.1, 0.25, None, 1.0, P(dl), P(rl), P(rc), P(st), S())

    assert call([0, 11, -1, 3], ld=8) != 0                    # ld < C
    assert call([0, 11, -1, 3], rows=0) != 0
    assert call([0, 12, -1, 3]) != 0                          # gold == C
    assert call([0, 11, -2, 3]) != 0                          # below -1
    assert lib.masr_last_error()
    torch.cuda.synchronize()
    assert same_bits(dl, dl0) and torch.isnan(rl).all() and (rc == -7).all() and torch.isnan(st).all()
    assert call([0, 11, -1, 3]) == 0                          # (the valid form)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- arg-max of the full-sequence greedy decode (rowops.hip recog_argmax_kernel)
def _argmax_rows(n, Cn, rng):
    """rows on the grid of multiples of 1/4 with the kinds r % 10: 0 plain, 1 equal maxima in one lane's strides (c, c + 64), 2 in different
    lanes, 3 every class tied, 4 +inf twice, 5 all -inf, 6 all NaN, 7 NaN mixed in (one ahead of the maximum), 8 the only value above -inf
    is -FLT_MAX, 9 the maximum in the last column"""
    z = (np.round(rng.standard_normal((n, Cn)) * 12.0) / 4.0).astype(F32)
    for r in range(n):
        k, row = r % 10, z[r]
        if k == 1 and Cn > 64:
            c = int(rng.integers(0, Cn - 64)); row[c] = row[c + 64] = 90.0
        elif k == 2 and Cn > 1:
            c = int(rng.integers(0, min(Cn, 64) - 1)); row[c] = row[min(Cn - 1, c + 1 + int(rng.integers(0, 20)))] = 90.0
        elif k == 3:
            row[:] = row[0]
        elif k == 4:
            row[int(rng.integers(0, Cn))] = np.inf; row[int(rng.integers(0, Cn))] = np.inf
        elif k == 5:
            row[:] = -np.inf
        elif k == 6:
            row[:] = np.nan
        elif k == 7:
            row[rng.random(Cn) < 0.3] = np.nan; row[0] = np.nan
        elif k == 8:
            row[:] = -np.inf; row[int(rng.integers(0, Cn))] = -FMAX
        elif k == 9:
            row[Cn - 1] = 95.0
    return z


@pytest.mark.parametrize("B,Lq,Cn,ld", ((3, 5, 367, 384), (1, 1, 12, 16), (7, 3, 31, 64), (4, 5, 64, 64), (2, 9, 5002, 5120), (16, 2, 65, 128),
                                        (1, 10, 2, 8), (5, 2, 129, 136)))
def test_recog_argmax(lib, B, Lq, Cn, ld):
    """out [L][B], out[l][b] = first maximal index of row b L + l; +inf in the pad columns rather than a NaN sentinel: a `v > mx` scan that
    read past C would let +inf win, whereas a NaN never wins and the read would go unseen; the same logits
    through the decode step's arg-max (decode.hip recog_argmax_step_kernel) must give the same indices"""
    n = B * Lq
    z = _argmax_rows(n, Cn, np.random.default_rng(B * 100 + Cn))
    zd = torch.full((n, ld), INF, device=DEV)
    zd[:, :Cn] = torch.from_numpy(z).to(DEV)
    out = torch.full((Lq + 1, B), -7, device=DEV, dtype=torch.int32)
    _cabi.check(lib.masr_test_recog_argmax(P(zd), ld, P(out), B, Lq, Cn, S()), "recog_argmax")
    step = torch.tensor([1, 0], device=DEV, dtype=torch.int32)
    out_step = torch.full((n,), -7, device=DEV, dtype=torch.int32)
    _cabi.check(lib.masr_test_recog_argmax_step(P(step), P(zd), ld, P(out_step), n, Cn, S()), "recog_argmax_step")
    torch.cuda.synchronize()
    want = np.array([R.argmax_first(z[r]) for r in range(n)], np.int32)
    got = out.cpu().numpy()
    assert (got[Lq] == -7).all(), "row L of the output written"
    assert np.array_equal(got[:Lq], want.reshape(B, Lq).T), (B, Lq, Cn, [(r, int(got[r % Lq, r // Lq]), int(want[r])) for r in range(n)
                                                                           if got[r % Lq, r // Lq] != want[r]][:8])
    assert np.array_equal(out_step.cpu().numpy(), want), "the decode step's arg-max disagrees"


def test_recog_argmax_errors(lib):
    z = torch.zeros(4, 16, device=DEV)
    out = torch.full((4,), -7, device=DEV, dtype=torch.int32)
    assert lib.masr_test_recog_argmax(P(z), 8, P(out), 2, 2, 12, S()) != 0         # ld < C
    assert lib.masr_test_recog_argmax(P(z), 16, P(out), 0, 2, 12, S()) != 0
    assert lib.masr_test_recog_argmax(P(z), 16, None, 2, 2, 12, S()) != 0
    torch.cuda.synchronize()
    assert (out == -7).all()


# ---------------------------------------------------------------- embedding forward (rowops.hip embed_fwd_kernel)
@pytest.mark.parametrize("B,Lq,E,V", ((16, 41, 512, 367), (3, 7, 64, 31), (1, 1, 1024, 5002), (5, 130, 384, 367)))
def test_embed_fwd(lib, B, Lq, E, V):
    """y32 = fl(fl(table[tok] + pe[l]) * keep) bit for bit (two fp32 operations, done in that order by the reference), y16 = one rounding of
    it.  The positional row is l, not b L + l: the rows of pe differ by 100, far more than the table's spread, and pe has NaN from row L on
    (B L rows are allocated); table rows that no token points at hold NaN"""
    g = gen(B * 1000 + E)
    n = B * Lq * E
    used = torch.unique(torch.cat([torch.tensor([0, V - 1], device=DEV), torch.randint(0, V, (min(V, 40),), device=DEV, generator=g)]))
    tok = used[torch.randint(0, len(used), (B, Lq), device=DEV, generator=g)].int()
    tok[0, 0] = 0; tok[-1, -1] = V - 1
    table = torch.full((V, E), NAN, device=DEV)
    table[used] = torch.randn(len(used), E, device=DEV, generator=g)
    pe = torch.full((B * Lq, E), NAN, device=DEV)
    pe[:Lq] = torch.randn(Lq, E, device=DEV, generator=g) + 100.0 * torch.arange(1, Lq + 1, device=DEV)[:, None]
    for drop_p in (0.0, 0.1):
        for by_ptr in (False, True):
            seed, site = 4321 + B, 9
            y32 = torch.full((n + 5,), NAN, device=DEV)
            y16 = torch.full((n + 5,), NAN, device=DEV, dtype=torch.bfloat16)
            seed_d = torch.tensor([seed], device=DEV, dtype=torch.int64).int() if by_ptr else None
            _cabi.check(lib.masr_test_embed_fwd(P(tok), P(table), P(pe), P(y32), P(y16), B, Lq, E, V, drop_p, seed + 1 if by_ptr else seed,
                                              site, P(seed_d), S()), "embed_fwd")
            keep = keep_mask(lib, seed, site, n, drop_p).view(B, Lq, E) if drop_p > 0 else None
            torch.cuda.synchronize()
            ref = R.embed_fwd(tok.cpu(), table.cpu(), pe.cpu(), keep.cpu() if keep is not None else None).reshape(-1)
            what = (B, Lq, E, V, drop_p, by_ptr)
            assert torch.isfinite(ref).all()
            assert torch.isnan(y32[n:]).all() and torch.isnan(y16[n:]).all(), ("written behind the output", what)
            assert same_bits(y32[:n].cpu(), ref), ("y32", what, int((y32[:n].cpu() != ref).sum()))
            assert same_bits(y16[:n].cpu(), ref.bfloat16()), ("y16 != bf16(y32)", what)
            if keep is not None:
                assert 0.05 < float((ref == 0).float().mean()) < 0.15 or n < 4096


def test_embed_errors(lib):
    tok = torch.tensor([[0, 5, 30]], device=DEV, dtype=torch.int32)
    table = torch.zeros(31, 64, device=DEV)
    pe = torch.zeros(3, 64, device=DEV)
    y32 = torch.full((3 * 64,), NAN, device=DEV)
    y16 = torch.full((3 * 64,), NAN, device=DEV, dtype=torch.bfloat16)
    dt = torch.full((31, 64), NAN, device=DEV)
    dy = torch.zeros(3, 64, device=DEV)
    assert lib.masr_test_embed_fwd(P(tok), P(table), P(pe), P(y32), P(y16), 1, 3, 64, 30, 0.0, 1, 1, None, S()) != 0      # token 30 with V = 30
    assert lib.masr_test_embed_bwd(P(tok), 3, P(dy), P(dt), 30, 64, 0, 0.0, 1, 1, None, S()) != 0
    assert lib.masr_test_embed_bwd(P(tok), 3, P(dy), P(dt), 31, 96, 0, 0.0, 1, 1, None, S()) != 0                         # E % 64
    tok[0, 1] = -1
    assert lib.masr_test_embed_fwd(P(tok), P(table), P(pe), P(y32), P(y16), 1, 3, 64, 31, 0.0, 1, 1, None, S()) != 0
    assert lib.masr_test_embed_bwd(P(tok), 3, P(dy), P(dt), 31, 64, 0, 0.0, 1, 1, None, S()) != 0
    assert lib.masr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y32).all() and torch.isnan(y16).all() and torch.isnan(dt).all()


# ---------------------------------------------------------------- embedding backward (folds.h embed_bwd_body + the host's token sort)
HITS = (1, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 2500)       # wave w takes hits w, w + 4, ..: eight loads per pass; 1024-hit chunks


def _bwd_tokens(V, g):
    """tokens with the hit counts of HITS on chosen rows (0 and V - 1 among them), ~300 more spread over a few others, every other row
    without a hit; positions shuffled"""
    ids = [0, V - 1, 1, 17, V // 2, 64, 65, V - 2, 200, 3, 100]
    toks = [torch.full((h,), v, dtype=torch.int64) for v, h in zip(ids, HITS)]
    toks.append(torch.tensor([120, 121, 122, 300])[torch.arange(300) % 4])
    tok = torch.cat(toks).to(DEV)
    return tok[torch.randperm(len(tok), device=DEV, generator=g)].int(), dict(zip(ids, HITS))


@pytest.mark.parametrize("V,E", ((367, 512), (5002, 64), (367, 384), (5002, 1024), (367, 64)))
def test_embed_bwd(lib, V, E):
    g = gen(V + E)
    tok, hits = _bwd_tokens(V, g)
    n = len(tok)
    dy = torch.randn(n, E, device=DEV, generator=g)
    cnt = torch.bincount(tok.long().cpu(), minlength=V).double()[:, None]
    assert all(int(cnt[v]) == h for v, h in hits.items()) and int((cnt == 0).sum()) > V - 20
    base = torch.randn(V + 1, E, device=DEV, generator=g)                           # accumulate = 1 adds to this; row V: the sentinel behind
    for drop_p in (0.0, 0.1):
        seed, site = 99 + E, 12
        keep = keep_mask(lib, seed, site, n * E, drop_p).view(n, E).cpu() if drop_p > 0 else None    # element row * E + col
        ref, mag = R.embed_bwd(tok.cpu(), dy.cpu(), V, keep)
        for accumulate in (0, 1):
            for by_ptr in (False, True):
                what = (V, E, drop_p, accumulate, by_ptr)
                outs = []
                for rep in range(2):                                                # twice: the same bits
                    dt = base.clone() if accumulate else torch.full((V + 1, E), NAN, device=DEV)
                    dt[V] = NAN
                    seed_d = torch.tensor([seed], device=DEV, dtype=torch.int32) if by_ptr else None
                    _cabi.check(lib.masr_test_embed_bwd(P(tok), n, P(dy), P(dt), V, E, accumulate, drop_p, seed + 1 if by_ptr else seed, site,
                                                      P(seed_d), S()), "embed_bwd")
                    torch.cuda.synchronize()
                    outs.append(dt)
                dt = outs[0]
                assert same_bits(outs[0], outs[1]), ("two launches differ", what)
                assert torch.isnan(dt[V]).all(), ("row V written", what)
                got = dt[:V].cpu()
                nohit = (cnt[:, 0] == 0)
                if accumulate:
                    assert same_bits(got[nohit], base[:V].cpu()[nohit]), ("rows without hits changed", what)
                else:
                    assert (got[nohit].view(torch.int32) == 0).all(), ("rows without hits are not +0", what)
                # an fp32 sum of n_v terms, each one fp32 product with the keep-scale: |got - ref| <= n_v 2^-24 sum |terms| (n_v - 1 additions
                # + the product); accumulate: + the rounding of the one addition to the table
                want = ref + (base[:V].cpu().double() if accumulate else 0.0)
                bound = cnt * U24 * mag + (U24 * want.abs() if accumulate else 0.0)
                within((got.double() - want).abs()[~nohit], bound[~nohit].clamp_min(1e-300), "embed_bwd", what)
                if drop_p == 0.0 and not accumulate and not by_ptr:
                    # the documented order of the additions (positions ascending inside a token: the host's stable sort), bit for bit
                    k32 = R.embed_bwd_kernel_order(tok.cpu(), dy.cpu(), V)
                    assert same_bits(got, k32), ("not the documented summation order", what, torch.nonzero((got != k32).any(1)).flatten()[:8].tolist())


# ---------------------------------------------------------------- cast + dropout (rowops.hip cast_dropout_kernel)
@pytest.mark.parametrize("n", (4, 5, 6, 7, 1023, 4000 * 512, 4000 * 512 + 3))
def test_cast_dropout(lib, n):
    """drop_p 0: plain bf16(x); else bf16(x * keep_i) -- one fp32 product, one rounding: bits.  The three elements behind n keep their sentinel"""
    g = gen(n)
    x = torch.randn(n + 3, device=DEV, generator=g)
    for drop_p in (0.0, 0.1, 0.25):
        for by_ptr in (False, True):
            seed, site = 777, 125
            y = torch.full((n + 3,), NAN, device=DEV, dtype=torch.bfloat16)
            seed_d = torch.tensor([seed], device=DEV, dtype=torch.int32) if by_ptr else None
            _cabi.check(lib.masr_test_cast_dropout(P(x), P(y), n, drop_p, seed + 1 if by_ptr else seed, site, P(seed_d), S()), "cast_dropout")
            keep = keep_mask(lib, seed, site, n, drop_p) if drop_p > 0 else None
            torch.cuda.synchronize()
            ref = R.cast_dropout(x[:n].cpu(), keep.cpu() if keep is not None else None)
            what = (n, drop_p, by_ptr)
            assert torch.isnan(y[n:]).all(), ("written behind n", what)
            assert same_bits(y[:n].cpu(), ref), (what, int((y[:n].cpu().float() != ref.float()).sum()))
            if keep is not None and n > 1000:
                assert abs(float((keep == 0).float().mean()) - drop_p) < 0.05


# ---------------------------------------------------------------- un-permutation of vgg2enc's weight gradient (folds.h vgg2enc_unpermute_body)
@pytest.mark.parametrize("E,Cc,Dp", ((512, 128, 20), (512, 128, 21), (64, 128, 1), (128, 4, 3)))
def test_vgg2enc_grad_unpermute(lib, E, Cc, Dp):
    """a pure gather: bits.  Distinct values per element (an arange, exact in fp32 below 2^24), so no swapped index pair can cancel"""
    n = E * Cc * Dp
    assert n < 2 ** 24
    gsrc = torch.arange(n, device=DEV, dtype=torch.float32)
    dw = torch.full((n + 4,), NAN, device=DEV)
    _cabi.check(lib.masr_test_vgg2enc_grad_unpermute(P(gsrc), P(dw), E, Cc, Dp, S()), "unpermute")
    torch.cuda.synchronize()
    assert torch.isnan(dw[n:]).all()
    assert same_bits(dw[:n].cpu(), R.vgg2enc_unpermute(gsrc.cpu(), E, Cc, Dp).reshape(-1))
    assert lib.masr_test_vgg2enc_grad_unpermute(P(gsrc), P(dw), E, 0, Dp, S()) != 0
