"""The CPU restatements of the training step's row kernels (tests/train_rowops_ref.py) against independent facts: the label-smoothed loss
against the reference's own formula (oracle/ref_cpu.py) and torch.autograd of it in fp64, plain cross entropy at eps = 0, the embedding
gradient against torch.autograd, the un-permutation against its index formula; and the record of how far an fp32 evaluation of the loss
gradient strays from fp64, which sizes the GPU test's tolerance.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_rowops_ref as R
from oracle import ref_cpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("eps", R.LS_EPS)
def test_ls_ce_is_the_reference_formula_and_its_autograd(eps):
    for i, (rows, C) in enumerate(((40, 367), (37, 31), (16, 2), (64, 8), (9, 700))):
        z, gold = R.ls_inputs(rows, C, 1.0 if i % 2 == 0 else 30.0, _gen(10 * i + 1))
        gold = gold.long()
        n_total = int((gold >= 0).sum())
        e32 = float(np.float32(eps))                          # the restatement takes the kernel's fp32 arguments
        zz = z.double().requires_grad_(True)
        loss = R.ls_loss_formula(zz, gold, e32)
        loss.backward()
        for grad_w in R.LS_GRAD_W:
            r = R.ls_ce(z, gold, eps, 1.0 / n_total, grad_w)
            assert abs(float(r["row_loss"].sum()) / n_total - float(loss)) <= 1e-12 * abs(float(loss)), (rows, C)
            want = zz.grad * n_total * r["gscale"]
            assert (r["dlogits"] - want).abs().max() <= 1e-12 * want.abs().max(), (rows, C, grad_w)
            assert (r["dlogits"][gold < 0] == 0).all() and (r["row_loss"][gold < 0] == 0).all()
        # the oracle's restatement of the same formula (fp64 in, python-float eps)
        lo, n_correct, nt = ref_cpu.label_smoothed_ce(z.double(), gold, e32)
        assert nt == n_total and abs(float(lo) - float(loss)) <= 1e-12 * abs(float(loss))
        assert int(r["correct"].sum()) == n_correct, (rows, C)
        if eps == 0.0:
            ce = F.cross_entropy(z.double(), gold, ignore_index=-1, reduction="sum") / n_total
            assert abs(float(r["row_loss"].sum()) / n_total - float(ce)) <= 1e-12 * abs(float(ce))
        # a valid row's gradient sums to zero over the classes: qsum sum p - sum q = 0
        v = r["valid"]
        assert (r["dlogits"][v].sum(dim=1).abs() <= 1e-13 * abs(r["gscale"])).all()


def test_ls_ce_non_finite_rows():
    z = torch.tensor([[0.5, -np.inf, 1.0, 0.0], [-np.inf, -np.inf, -3.4028234663852886e38, -np.inf]])
    gold = torch.tensor([2, 2])
    r0 = R.ls_ce(z, gold, 0.0, 0.5)
    ce = F.cross_entropy(z.double(), gold, reduction="none")
    assert torch.isfinite(r0["row_loss"]).all() and torch.allclose(r0["row_loss"], ce, rtol=1e-14, atol=0)
    assert torch.isfinite(r0["dlogits"]).all() and r0["correct"].tolist() == [1, 1]
    r2 = R.ls_ce(z, gold, 0.2, 0.5)
    assert (r2["row_loss"] == np.inf).all()                 # q > 0 on a class of probability 0
    assert float(R.ls_loss_formula(z.double(), gold, 0.2)) == np.inf


def test_argmax_first():
    rng = np.random.default_rng(1)
    for _ in range(50):
        row = np.round(rng.standard_normal(70) * 4).astype(np.float32)
        assert R.argmax_first(row) == int(torch.from_numpy(row).argmax())        # (torch on the CPU: the first maximal index)
    assert R.argmax_first(np.full(5, -np.inf, np.float32)) == 0
    assert R.argmax_first(np.full(5, np.nan, np.float32)) == 0
    assert R.argmax_first(np.array([np.nan, -np.inf, -3.4028235e38, -np.inf], np.float32)) == 2
    assert R.argmax_first(np.array([np.nan, 1.0, 3.0, 3.0], np.float32)) == 2


def test_fp32_factor_per_case():
    """the deviation of the fp32 evaluation from fp64 in units of |gscale| p (|z - lse| + 1) 2^-24, per case (shape, logit scale; the largest
    over eps and grad_w is printed): what sizes the second term of the GPU test's dlogits bound, which computes it for its own inputs.  It
    is a few units where the logits are O(1) and grows with |lse| (lse = max + log(..) is itself rounded at its own magnitude, which the
    unit does not see for the classes near the maximum): bounded here by 4 + 2 |lse|_max units -- half an ulp of lse and of z - lse each
    are at most |lse| 2^-24, the exponential, the sum and the logarithm a few units more"""
    for i, (rows, C, _) in enumerate(R.LS_SHAPES):
        for scale in R.LS_SCALES:
            z, gold = R.ls_inputs(rows, C, scale, _gen(100 + i))
            n = max(1, int((gold >= 0).sum()))
            worst = 0.0
            for eps in R.LS_EPS:
                for gw in R.LS_GRAD_W:
                    f = R.dlogits_fp32_factor(z, gold, eps, 1.0 / n, gw)
                    assert np.isfinite(f) and f >= 0.0
                    worst = max(worst, f)
            lse_max = float(R.ls_ce(z, gold, 0.0, 1.0 / n)["lse"].abs().max())
            print(f"fp32 factor, case rows {rows} C {C} scale {scale}: {worst:.3g} (max |lse| {lse_max:.4g})")
            assert worst <= 4.0 + 2.0 * lse_max, (rows, C, scale, worst, lse_max)


def test_embed_refs_against_autograd():
    g = _gen(7)
    for n, V, E, p in ((50, 11, 64, 0.0), (300, 7, 128, 0.25), (2100, 5, 64, 0.1)):
        tok = torch.randint(0, V, (n,), generator=g)
        tok[tok == 3] = 4                                     # a row without hits
        table = torch.randn(V, E, dtype=torch.float64, generator=g, requires_grad=True)
        pe = torch.randn(n, E, dtype=torch.float64, generator=g)
        keep = (torch.rand(n, E, generator=g) >= p).double() / (1.0 - p)
        dy = torch.randn(n, E, generator=g)
        y = (F.embedding(tok, table) + pe) * keep
        y.backward(dy.double())
        ref, mag = R.embed_bwd(tok, dy, V, keep)
        assert torch.allclose(ref, table.grad, rtol=1e-13, atol=1e-13)
        assert (ref[3] == 0).all() and (mag >= ref.abs() - 1e-12).all()
        k32 = R.embed_bwd_kernel_order(tok, dy, V, keep.float())
        cnt = torch.bincount(tok, minlength=V).double()[:, None]
        assert ((k32.double() - ref).abs() <= cnt * R.U24 * mag).all()           # the sequential-summation bound the GPU test uses
        # forward: the fp32 two-operation form is the fp64 value to its roundings
        f32 = R.embed_fwd(tok.view(1, n), table.detach().float(), pe.float(), keep.float().view(1, n, E))
        f64 = (table.detach().float().double()[tok] + pe.float().double()) * keep
        assert ((f32.double()[0] - f64).abs() <= 3 * R.U24 * f64.abs()).all()          # (the third: keep itself rounded to fp32)


def test_cast_dropout_ref():
    x = torch.randn(1000, generator=_gen(3))
    keep = (torch.rand(1000, generator=_gen(4)) >= 0.25).float() / 0.75
    assert torch.equal(R.cast_dropout(x), x.bfloat16())
    y = R.cast_dropout(x, keep)
    assert (y[keep == 0] == 0).all() and torch.equal(y, (x * keep).bfloat16())


def test_unpermute_is_the_index_formula():
    for E, C, Dp in ((3, 4, 5), (2, 128, 3), (5, 1, 7)):
        g = torch.arange(E * C * Dp, dtype=torch.float32).reshape(E, Dp * C)
        dw = R.vgg2enc_unpermute(g, E, C, Dp)
        assert dw.shape == (E, C * Dp)
        for e in range(E):
            for c in range(C):
                for d in range(Dp):
                    assert dw[e, c * Dp + d] == g[e, d * C + c]
        # the inverse of the permutation the forward applies to the weight: [E][C][Dp] -> [E][Dp][C]
        assert torch.equal(dw.reshape(E, C, Dp).transpose(1, 2).reshape(E, Dp * C), g)
