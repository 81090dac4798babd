"""Plain restatements of the training step's row kernels (rowops.hip ls_ce_kernel / recog_argmax_kernel / embed_fwd_kernel /
cast_dropout_kernel, folds.h embed_bwd_body / vgg2enc_unpermute_body) in torch on the CPU, fp64 unless said otherwise.  No project imports:
tests/test_train_rowops_ref_cpu.py pins them against torch.autograd and the oracle's formula, tests/test_hip_train_row_kernels.py compares
the kernels with them."""
import numpy as np
import torch

F32 = np.float32
U24 = 2.0 ** -24           # fp32 unit round-off
TINY32 = 2.0 ** -126       # smallest normal fp32 (and bf16) number: results below it may be flushed to zero


def argmax_first(row):
    """first maximal index of a 1-D numpy row; a NaN never wins, and a row with nothing above -inf gives 0 (tests/test_hip_decode_kernels.py
    argmax_ref: the two greedy arg-max kernels must agree)"""
    v = np.where(np.isnan(row), -np.inf, row)
    m = v.max()
    return 0 if m == -np.inf else int(np.flatnonzero(v == m)[0])


def ls_consts(eps, C, inv_ntotal, grad_w, dtype):
    """the kernel's scalars from the fp32 arguments it receives: on = 1 - eps, off = eps / C, qsum = on + (C - 1) off, gscale = inv_ntotal grad_w
    -- formed in fp32 (as the kernel does) or in fp64 from the same fp32 arguments"""
    eps, inv, gw = F32(eps), F32(inv_ntotal), F32(grad_w)
    if dtype == torch.float64:
        eps, inv, gw, one, Cf, Cm = float(eps), float(inv), float(gw), 1.0, float(C), float(C - 1)
    else:
        one, Cf, Cm = F32(1.0), F32(C), F32(C - 1)
    on, off = (one - eps, eps / Cf) if eps > 0 else (one, one * 0)
    return float(on), float(off), float(on + Cm * off), float(inv * gw)


def ls_ce(z, gold, eps, inv_ntotal, grad_w=1.0, dtype=torch.float64):
    """label-smoothed cross entropy of logits z [rows][C] (any float dtype) against gold [rows] (-1 = not counted), in the kernel's
    closed form and order of operations: lse = max + log sum exp(z - max); loss_r = -((on - off)(z_g - lse) + off (sum z - C lse)), plain
    -(z_g - lse) when eps == 0; dlogits = (qsum softmax - q) gscale; rows with gold -1: loss 0, gradient 0.
    -> dict(row_loss, dlogits, p, zl = z - lse, lse, correct, valid, gscale), tensors of `dtype`"""
    z = z.detach().cpu().to(dtype)
    gold = gold.detach().cpu().long()
    rows, C = z.shape
    on, off, qsum, gscale = ls_consts(eps, C, inv_ntotal, grad_w, dtype)
    valid = gold >= 0
    g = gold.clamp_min(0)[:, None]
    mx = z.max(dim=1, keepdim=True).values
    lse = mx + torch.log(torch.exp(z - mx).sum(dim=1, keepdim=True))
    lg = z.gather(1, g) - lse
    if off > 0:
        loss = -((on - off) * lg + off * (z.sum(dim=1, keepdim=True) - C * lse))
    else:
        loss = -lg
    zl = z - lse
    p = torch.exp(zl)
    q = torch.full_like(z, off).scatter_(1, g, on)
    d = (qsum * p - q) * gscale
    zn = z.numpy()
    am = torch.tensor([argmax_first(zn[r]) for r in range(rows)])
    zero = torch.zeros((), dtype=dtype)
    return dict(row_loss=torch.where(valid, loss[:, 0], zero), dlogits=torch.where(valid[:, None], d, zero), p=p, zl=zl,
                correct=(valid & (am == gold)).int(), valid=valid, gscale=gscale, lse=lse[:, 0])


def ls_loss_formula(z, gold, eps):
    """the reference's own formula (transformer_torch_trainer.py:64-84 as restated in oracle/ref_cpu.py label_smoothed_ce), differentiable:
    q = onehot (1 - eps) + (1 - onehot) eps / C, loss = sum over gold != -1 of -(q . log_softmax) / n_total; eps == 0: the gold term alone"""
    mask = gold.ne(-1)
    n_total = int(mask.sum())
    logp = torch.log_softmax(z, dim=-1)
    if eps > 0.0:
        C = z.shape[1]
        one_hot = torch.zeros_like(z).scatter(1, (mask.long() * gold).view(-1, 1), 1.0)
        q = one_hot * (1 - eps) + (1 - one_hot) * eps / C
        return (-(q * logp).sum(dim=1))[mask].sum() / n_total
    return (-logp[mask, gold[mask]]).sum() / n_total


def dlogits_unit(ref64):
    """|gscale| p (|z - lse| + 1) 2^-24: the error an fp32 evaluation of exp(z - lse) carries into the gradient (z - lse is rounded to fp32
    before the exponential, which itself is good to an ulp or two)"""
    p, zl = ref64["p"], ref64["zl"]
    return torch.where(p > 0, abs(ref64["gscale"]) * p * (zl.abs() + 1.0) * U24, torch.zeros_like(p))      # (p = 0 at z = -inf: no error)


# The few fp32 roundings that are relative to the gradient value itself (the scalars on / off / qsum / gscale, the product, the difference and
# the scaling: < 8 units of 2^-24 |v|) sit inside the 2^-9 |v| that the one-bf16-ulp term leaves beside the rounding's own half ulp, and a
# value below the smallest normal number may be flushed; neither is charged to the exponential's factor.
def dlogits_fp32_factor(z, gold, eps, inv_ntotal, grad_w):
    """largest deviation of the fp32 evaluation (torch.float32 on the CPU, the kernel's order of operations) from the fp64 one, in units of
    dlogits_unit"""
    r64 = ls_ce(z, gold, eps, inv_ntotal, grad_w)
    r32 = ls_ce(z, gold, eps, inv_ntotal, grad_w, dtype=torch.float32)
    dev = (r32["dlogits"].double() - r64["dlogits"]).abs() - 8 * U24 * r64["dlogits"].abs() - TINY32
    unit = dlogits_unit(r64)
    ratio = torch.where(dev > 0, dev / unit.clamp_min(1e-300), torch.zeros_like(dev))
    return float(ratio.max())


# The GPU test allows GPU_EXP_ALLOWANCE x the factor that dlogits_fp32_factor finds for the very launch it checks (the same logits, gold, eps,
# inv_ntotal and grad_w: one factor per case, nothing rounded up): the hardware __expf / __logf are 1-2 ulp approximations where libm is
# correctly rounded to < 1 ulp.  tests/test_train_rowops_ref_cpu.py::test_fp32_factor_per_case prints the factors of the GPU test's shapes.
GPU_EXP_ALLOWANCE = 4.0


def dlogits_bound(ref64, factor):
    """allowed |dlogits - v| for the bf16 output against the fp64 value v: one bf16 ulp of v, the flush threshold, and GPU_EXP_ALLOWANCE x the
    case's fp32 factor in units of dlogits_unit"""
    return 2.0 ** -8 * ref64["dlogits"].abs() + TINY32 + GPU_EXP_ALLOWANCE * factor * dlogits_unit(ref64)


def embed_fwd(tok, table, pe, keep=None):
    """fp32, two operations in the kernel's order: fl(fl(table[tok] + pe[l]) * keep); tok [B][L], table [V][E], pe [>= L][E], keep [B][L][E] or None"""
    B, L = tok.shape
    v = table.float()[tok.long()] + pe.float()[:L][None]
    return v * keep.float() if keep is not None else v


def embed_bwd(tok, dy, V, keep=None):
    """dtable [V][E] (fp64) = sum over positions i with tok[i] == v of dy[i] keep[i], and the same sum of |terms| (the scale of the fp32
    accumulation bound); tok [n], dy [n][E]"""
    g = dy.double() * (keep.double() if keep is not None else 1.0)
    out = torch.zeros(V, dy.shape[1], dtype=torch.float64).index_add_(0, tok.long(), g)
    mag = torch.zeros(V, dy.shape[1], dtype=torch.float64).index_add_(0, tok.long(), g.abs())
    return out, mag


def embed_bwd_kernel_order(tok, dy, V, keep=None):
    """the same sum in fp32 in the kernel's documented order: the hits of a token ascending by position; wave w of 4 takes hits w, w + 4, ..
    within each chunk of 1024 hits, eight at a time (u = 0 .. 7 -> hit h0 + 4 u, h0 = w, w + 32, ..) added one by one to a running sum that
    carries over the chunks; the result is (wave 0 + wave 1) + (wave 2 + wave 3).  -> fp32 [V][E]"""
    g = dy.float() * (keep.float() if keep is not None else 1.0)
    tok = tok.long()
    out = torch.zeros(V, dy.shape[1], dtype=torch.float32)
    for v in torch.unique(tok).tolist():
        pos = torch.nonzero(tok == v).flatten()              # ascending
        part = []
        for w in range(4):
            s = torch.zeros(dy.shape[1], dtype=torch.float32)
            for c0 in range(0, len(pos), 1024):
                for i in pos[c0:c0 + 1024][w::4].tolist():
                    s = s + g[i]
            part.append(s)
        out[v] = (part[0] + part[1]) + (part[2] + part[3])
    return out


def cast_dropout(x, keep=None):
    """bf16(fl32(x * keep)): one fp32 product, one rounding"""
    return (x.float() * keep.float() if keep is not None else x.float()).bfloat16()


def vgg2enc_unpermute(g, E, C, Dp):
    """dw [E][C][Dp] <- g [E][Dp][C]"""
    return g.reshape(E, Dp, C).transpose(1, 2).reshape(E, C * Dp).contiguous()


# ---------------------------------------------------------------- the loss head's cases (shared by the CPU self-test and the GPU test)
LS_SHAPES = ((640, 367, 384), (37, 31, 128), (5, 64, 64), (130, 128, 128), (33, 65, 128), (64, 8, 128), (257, 5002, 5120), (1, 2, 128))
LS_SCALES = (1.0, 30.0, 3000.0)
LS_EPS = (0.0, 0.1, 0.2)
LS_GRAD_W = (1.0, 0.7)


def ls_inputs(rows, C, scale, g, device="cpu"):
    """logits on the grid of multiples of 1/8 (exact in fp32 up to 2^21: the arg-max is unique or an exact tie, the same in every precision)
    and gold, with the row kinds r % 8: 0 plain, 1 gold -1, 2 gold 0, 3 gold C - 1, 4 a constant row (every class tied: arg-max 0; gold 0 or
    C - 1), 5 two equal maxima 64 columns apart (the same lane's next stride; C <= 64: neighbouring lanes) with gold on the later (wrong) or
    the earlier (right) one, 6 the gold logit far below the rest, 7 gold = the arg-max"""
    z = torch.round(torch.randn(rows, C, device=device, generator=g) * (scale * 8.0)) / 8.0
    gold = torch.randint(0, C, (rows,), device=device, generator=g)
    for r in range(rows):
        k = r % 8
        if k == 1:
            gold[r] = -1
        elif k == 2:
            gold[r] = 0
        elif k == 3:
            gold[r] = C - 1
        elif k == 4:
            z[r] = z[r, 0]
            gold[r] = 0 if r % 16 == 4 else C - 1
        elif k == 5 and C > 1:
            a = r % C
            b = (a + 64) % C if C > 64 else (a + 1) % C
            lo, hi = min(a, b), max(a, b)
            z[r, lo] = z[r, hi] = z[r].max() + 1.0
            gold[r] = hi if r % 16 == 5 else lo
        elif k == 6:
            z[r, gold[r]] = z[r].min() - 40.0 * scale
        elif k == 7:
            gold[r] = z[r].argmax()
    return z, gold.int()
