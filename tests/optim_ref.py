"""Plain restatements of the flat optimiser passes and the operand-shadow layouts of csrc/optim.hip, for tests/test_hip_optim_kernels.py and
tests/test_hip_shadow_kernels.py (the GPU side) and tests/test_optim_ref_cpu.py (which pins THIS module against torch.optim, clip_grad_norm_ and
F.conv2d, without a GPU).

Arithmetic is numpy float64 on exactly the fp32 values a kernel reads.  Next to each value stands the bound of the kernel's fp32 evaluation
against it, built rounding by rounding: an fp32 operation with a finite, normal result r adds at most U24 |r| (U24 = 2^-24; an explicit or
contracted fused multiply-add, a division and sqrtf count as ONE rounding each -- HIP's fp32 division and square root are correctly rounded by
default), and the error an operand already carries goes through the operation's derivative.  A compiler that contracts a multiply into the
following add only removes a rounding, so the bound holds for every contraction.  The products of two error terms (second order, a factor
~2^-24 below the bound) are covered by SLACK = 1 + 2^-10.

The scalars a launcher derives on the host (Adam's step size and bias correction) are restated with their roundings (dtype = float32, what the
kernel gets) or without them (dtype = float64, for the comparison with torch.optim in float64)."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
F32 = np.float32
F64 = np.float64


def f32v(x):
    """the fp32 value a float argument arrives as, as a Python float"""
    return float(F32(x))


# ---------------------------------------------------------------- the gradient norm and the clip coefficient
def norm(x):
    """sqrt(sum x^2) in fp64 (x: fp32 numpy)"""
    with np.errstate(over="ignore", invalid="ignore"):
        x64 = x.astype(F64)
        return float(np.sqrt(np.sum(x64 * x64)))


def norm_f32(x):
    """... as the kernel stores it: the fp64 value cast to fp32 (inf where it overflows)"""
    with np.errstate(over="ignore"):
        return F32(norm(x))


def clip_coef(norm_, max_norm):
    """torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6) clamped to <= 1, NaN kept -- two correctly rounded fp32 operations (numpy float32)"""
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(norm_) + F32(1e-6))
    return c if np.isnan(c) else min(c, F32(1.0))


# ---------------------------------------------------------------- clip + SGD, clip + scale, clip + accumulate
def sgd(p, g, mom, coef, lr, momentum, nesterov, step_flags):
    """torch.optim.SGD(momentum, nesterov, dampening 0) on g * coef.  step_flags bit 0: first step (buf = g, the buffer is not read); bit 1: last
    step (the buffer is not written).  p, g, mom: fp32 (or fp64) numpy; coef, lr, momentum: the values the kernel holds.
    -> {"p", "p_bound", "mom", "mom_bound"}; mom is None where the kernel must not write the buffer (momentum 0, or the last step)."""
    p64, g64 = p.astype(F64), g.astype(F64)
    coef, lr, momentum = float(coef), float(lr), float(momentum)
    first, last = bool(step_flags & 1), bool(step_flags & 2)
    gi = g64 * coef
    e_gi = U24 * np.abs(gi)                                         # 1 rounding: g * coef
    mom_new = mom_bound = None
    if momentum != 0.0:
        if first:
            b, e_b = gi, e_gi
        else:
            b = momentum * mom.astype(F64) + gi
            e_b = e_gi + U24 * np.abs(b)                            # + 1 rounding: fma(momentum, mom, gi)
        if not last:
            mom_new, mom_bound = b, e_b * SLACK
        if nesterov:
            step = momentum * b + gi
            e_step = abs(momentum) * e_b + e_gi + U24 * np.abs(step)    # + 1 rounding: fma(momentum, b, gi)
        else:
            step, e_step = b, e_b
    else:
        step, e_step = gi, e_gi
    pn = p64 - lr * step
    e_p = abs(lr) * e_step + U24 * np.abs(pn)                       # + 1 rounding: fma(-lr, step, p)
    return {"p": pn, "p_bound": e_p * SLACK, "mom": mom_new, "mom_bound": mom_bound}


def scale_bits(g, coef):
    """g * coef: one rounding of exact inputs -> the bits (numpy float32 multiplication is correctly rounded)"""
    with np.errstate(all="ignore"):
        return g.astype(F32) * F32(coef)


def axpy(acc, g, coef):
    """acc + coef * g -> (value, bound): 2 roundings (the product, the sum), or 1 where the compiler fuses them"""
    prod = float(coef) * g.astype(F64)
    out = acc.astype(F64) + prod
    return out, (U24 * (np.abs(prod) + np.abs(out))) * SLACK


# ---------------------------------------------------------------- the Adam family
def adam_scalars(lr, b1, b2, t, weight_decay=0.0, decoupled=0, dtype=F32):
    """what mk_adam / mk_adam_guarded / mk_adam_sum pass to the kernel: bias corrections in double from the fp32 betas, each scalar rounded once
    to fp32; 1 - b1, 1 - b2 and 1 - lr wd are fp32 operations of the kernel / the launcher.  dtype = float64: no rounding anywhere."""
    T = dtype
    lr_, b1_, b2_, wd_ = T(lr), T(b1), T(b2), T(weight_decay)
    bc1 = 1.0 - math.pow(float(b1_), t)
    bc2 = 1.0 - math.pow(float(b2_), t)
    return {"step_size": float(T(float(lr_) / bc1)), "inv_sqrt_bc2": float(T(1.0 / math.sqrt(bc2))),
            "b2": float(b2_), "omb1": float(T(1.0) - b1_), "omb2": float(T(1.0) - b2_),
            "decay_mul": float(T(1.0) - lr_ * wd_) if decoupled else 1.0, "l2": 0.0 if decoupled else float(wd_)}


def adam(p, g, m, v, sc, eps, e_g=None):
    """adam_kernel's statement: pi = p decay_mul; gi = g + l2 pi; m += (gi - m)(1 - b1); v = b2 v + (1 - b2) gi gi;
    p = pi - step_size m / (sqrt(v) inv_sqrt_bc2 + eps).  g may be fp64 with the error e_g it already carries (the summed-gradient form).
    -> {"p", "m", "v", "p_bound", "m_bound", "v_bound"}"""
    p64, g64, m64, v64 = (a.astype(F64) for a in (p, g, m, v))
    eps = float(eps)
    ss, isb, b2, omb1, omb2, dm, l2 = (sc[k] for k in ("step_size", "inv_sqrt_bc2", "b2", "omb1", "omb2", "decay_mul", "l2"))
    A = np.abs
    pi = p64 * dm
    e_pi = U24 * A(pi)                                              # 1: p * decay_mul
    gi = g64 + l2 * pi
    e_gi = (0.0 if e_g is None else e_g) + abs(l2) * e_pi + U24 * (A(l2 * pi) + A(gi))     # 2: the product, the sum
    d = gi - m64
    mn = m64 + d * omb1
    e_m = omb1 * e_gi + U24 * (omb1 * A(d) + A(d * omb1) + A(mn))   # 3: the difference, the product, the sum
    t1, t2 = b2 * v64, omb2 * gi
    t3 = t2 * gi
    vn = t1 + t3
    e_v = 2.0 * A(t2) * e_gi + U24 * (A(t1) + 2.0 * A(t3) + A(vn))  # 4: b2 v, (1 - b2) gi, ... gi, the sum (the second product carries the first's error)
    s = np.sqrt(vn)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(s > 0, e_v / (2.0 * s), 0.0) + U24 * s       # sqrtf: 1 (vn == 0 only where gi == 0 and v == 0: no error to carry)
    den = s * isb + eps
    e_den = isb * e_s + U24 * (s * isb + den)                       # 2: the product, the sum
    num = ss * mn
    e_num = abs(ss) * e_m + U24 * A(num)                            # 1
    q = num / den
    e_q = e_num / den + A(num) * e_den / (den * den) + U24 * A(q)   # division: 1
    pn = pi - q
    e_p = e_pi + e_q + U24 * A(pn)                                  # 1
    return {"p": pn, "m": mn, "v": vn, "p_bound": e_p * SLACK, "m_bound": e_m * SLACK, "v_bound": e_v * SLACK}


def sum_list(grads, scale):
    """(((g0 + g1) + g2) + ...) * scale, left to right -> (value, bound): one rounding per addition behind the first (0 + g0 is exact) and one
    for the product"""
    s = grads[0].astype(F64)
    e = np.zeros_like(s)
    for gk in grads[1:]:
        s = s + gk.astype(F64)
        e = e + U24 * np.abs(s)
    out = s * float(scale)
    return out, (abs(float(scale)) * e + U24 * np.abs(out)) * SLACK


def adam_sum(p, grads, gscale, m, v, sc, eps):
    """masr_adam_sum_step: plain Adam (no weight decay) on sum_list(grads, gscale)"""
    g, e_g = sum_list(grads, gscale)
    return adam(p, g, m, v, sc, eps, e_g=e_g)


def guarded(flags, slot, norm_):
    """the hand-over of adam_guarded_kernel: flags int [2] as the launch finds them -> (skip, which candidate, flags after it).  The launch is
    skipped under a NaN norm; otherwise it takes B when the launch before (flags[slot ^ 1]) was skipped, else A; it leaves its own verdict in
    flags[slot] and flags[slot ^ 1] as it was."""
    skip = bool(np.isnan(F32(norm_)))
    cand = "B" if flags[slot ^ 1] != 0 else "A"
    after = list(flags)
    after[slot] = 1 if skip else 0
    return skip, cand, after


# ---------------------------------------------------------------- the operand shadows: index maps + one round-to-nearest-even bf16 cast
def bf16(x):
    """fp32 numpy -> torch bfloat16 (round to nearest even), same shape"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)


def linear_layouts(w):
    """W [N][K] -> k16 [N][K], t16 [K][N] (the transpose; the kernel's row pitch ldt >= N is the caller's)"""
    return w, w.T


def conv_layouts(w):
    """w [CO][CI][3][3] (tap = 3 ky + kx) -> wk [CO][tap * CI + ci] = w[co][ci][tap] (forward operand) and
    wd [CI][tap' * CO + co] = w[co][ci][8 - tap'] (dgrad operand: the kernel flipped), kernels.h"""
    CO, CI = w.shape[:2]
    w9 = w.reshape(CO, CI, 9)
    wk = np.empty((CO, 9 * CI), w.dtype)
    wd = np.empty((CI, 9 * CO), w.dtype)
    for tap in range(9):
        wk[:, tap * CI:(tap + 1) * CI] = w9[:, :, tap]
        wd[:, tap * CO:(tap + 1) * CO] = w9[:, :, 8 - tap].T
    return wk, wd


def vgg2enc_layouts(w, E, C, Dp):
    """w [E][C * Dp] with the reference's feature index c * Dp + d -> wk [E][d * C + c] (the engine's NHWC order) and wt = wk^T [Dp * C][E]"""
    w3 = w.reshape(E, C, Dp)
    wk = np.empty((E, Dp * C), w.dtype)
    for d in range(Dp):
        wk[:, d * C:(d + 1) * C] = w3[:, :, d]
    return wk, wk.T


def conv_with_operand(x, wop, cout):
    """what the conv kernels compute from a [cout][tap * cin + c] operand: out[o][y][x] = sum over tap, c of in[c][y + ky - 1][x + kx - 1] *
    wop[o][tap * cin + c] with zero padding (x fp64 [cin][H][W])"""
    cin, H, W = x.shape
    xp = np.zeros((cin, H + 2, W + 2), F64)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((cout, H, W), F64)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        win = xp[:, ky:ky + H, kx:kx + W]                           # in[c][y + ky - 1][x + kx - 1]
        out += np.einsum("oc,chw->ohw", wop[:, tap * cin:(tap + 1) * cin], win)
    return out
