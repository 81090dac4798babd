"""Plain restatements of the BLSTM path's LSTM kernels (csrc/lstm.hip, csrc/lstm_rec.hip) in torch on the CPU, fp64 unless said otherwise, with
the checkers as functions of arrays.  No project imports: tests/test_lstm_ref_cpu.py pins the restatement against torch.nn.LSTM and runs the
checkers on an honest fp32 emulation of the kernels and on mutated ones; tests/test_hip_lstm_kernels.py runs the same checkers on what the
kernels wrote.

Layout (the kernels'): rows are batch-first, the gate axis is UNIT-MAJOR (index u * 4 + g, g in torch's order i, f, g, o), index 0 / 1 of a
pair = forward / reverse direction, KP = H rounded up to a multiple of 32 (the bf16 recurrent operand, pad columns zero).
    gx [2] fp32 [B][T][4H]   input contribution + biases          whh16 [2] bf16 [4H][KP]    whhT16 [2] bf16 [H][4H]
    y16 bf16 [B][T][2H]      act [2] fp32 [B][T][4H]              c [2] fp32 [B][T][H]        dy fp32 [B][T][2H]      dz16 [2] bf16 [B][T][4H]
Packed-sequence rules: sequence b takes part in steps t < lens[b] only; the forward direction starts from the zero state at t = 0, the
reverse direction at t = lens[b] - 1; outside the sequence y16 / dz16 are +0 and act / c are not written.

The checkers force the teacher: every step is recomputed in fp64 from exactly the values the kernel read for it -- its own y16 row and saved
c of the step before (forward), its own dz16 row of the step processed before (backward) -- so no tolerance has to absorb a value that was
rounded the other way ten steps earlier, and by induction over the steps the whole sequence is pinned."""
import numpy as np
import torch

U24 = 2.0 ** -24           # fp32 unit round-off
ULP32 = 2.0 ** -23         # an fp32 ulp, relative to the value (upper bound)
TINY32 = 2.0 ** -126       # smallest normal fp32 (and bf16) number: results below it may be flushed to zero
GPU_EXP_ALLOWANCE = 4.0    # ulps of fp32 allowed to the device's __expf / tanhf (the project's constant, tests/train_rowops_ref.py)
F64 = torch.float64
NAN_BITS = 0x7FC00000      # torch.full(.., nan): the sentinel of the regions nobody writes


def kp_of(H):
    return (H + 31) // 32 * 32


def bf16_half_ulp(v):
    """half an ulp of bfloat16 (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8) -- between 2^-9 |v| and 2^-8 |v|; what one correct
    rounding to bf16 can move a value by"""
    v = v.abs().clamp_min(TINY32)
    return torch.exp2(torch.floor(torch.log2(v)) - 8.0)


# ---------------------------------------------------------------- the permutations (csrc/lstm.hip lstm_perm_rows / src_col / unperm)
def unit_major_rows(H):
    """index tensor r [4H]: row u * 4 + g of the kernels' order is row r[u * 4 + g] = g * H + u of torch's"""
    pr = torch.arange(4 * H)
    return (pr % 4) * H + pr // 4


def src_col(K, pc, pd):
    """index tensor [K]: column k of the kernels' order is torch's column (k % pc) * pd + k / pc when the input is an NHWC conv map ([pd][pc],
    channel fastest; torch's feature order is c * pd + d), else k"""
    k = torch.arange(K)
    return (k % pc) * pd + k // pc if pc else k


def shadows(wih, whh, bih, bhh, H, K, pc, pd):
    """-> wih16 [4H][K], wihT16 [K][4H], whh16 [4H][KP], whhT16 [H][4H] (bf16), bias [4H] (fp32): one rounding each, one fp32 addition"""
    r = unit_major_rows(H)
    wih16 = wih.float()[r][:, src_col(K, pc, pd)].bfloat16()
    whh16 = torch.zeros(4 * H, kp_of(H), dtype=torch.bfloat16)
    whh16[:, :H] = whh.float()[r].bfloat16()
    return wih16, wih16.t().contiguous(), whh16, whh16[:, :H].t().contiguous(), (bih.float() + bhh.float())[r]


def unperm(src, H, K, pc, pd):
    """dst [4H][K] in torch's order from src [4H][K] in the kernels': dst[g H + u][src_col(k)] = src[u 4 + g][k]"""
    dst = torch.empty_like(src)
    tmp = torch.empty_like(src)
    tmp[:, src_col(K, pc, pd)] = src
    dst[unit_major_rows(H)] = tmp
    return dst


# ---------------------------------------------------------------- one step, any dtype
def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def fwd_step(z, c_prev):
    """z [B][H][4] (i, f, g, o), c_prev [B][H] -> act [B][H][4], c, h"""
    i, f, o = _sig(z[..., 0]), _sig(z[..., 1]), _sig(z[..., 3])
    g = torch.tanh(z[..., 2])
    c = f * c_prev + i * g
    return torch.stack((i, f, g, o), dim=-1), c, o * torch.tanh(c)


def bwd_step(dh, act, c, c_prev, carry):
    """dh, c, c_prev, carry [B][H], act [B][H][4] -> dz [B][H][4], dc"""
    i, f, g, o = act.unbind(-1)
    tc = torch.tanh(c)
    dc = dh * o * (1.0 - tc * tc) + carry
    return torch.stack((dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)), dim=-1), dc


def _order(d, T, backward=False):
    """the time steps of direction d in the order the pass visits them"""
    fwd = range(T) if d == 0 else range(T - 1, -1, -1)
    return list(reversed(fwd)) if backward else list(fwd)


def _first_mask(d, t, lens):
    """sequences whose FIRST forward step of direction d is t (c_prev = h_prev = 0 there)"""
    return (lens == t + 1) if d else torch.full_like(lens, t == 0, dtype=torch.bool)


def _last_mask(d, t, lens):
    """sequences whose LAST forward step of direction d is t (no dL/dc flows in there)"""
    return torch.full_like(lens, t == 0, dtype=torch.bool) if d else (lens == t + 1)


# ---------------------------------------------------------------- the free-running fp64 form (no bf16): what torch.nn.LSTM computes
def blstm_free(gx, w_hh, lens):
    """gx [2] [B][T][4H], w_hh [2] [4H][H] (unit-major rows), lens [B] -> y [B][T][2H], act [2], c [2] in fp64; zero outside the sequences"""
    B, T, G = gx[0].shape
    H = G // 4
    y = torch.zeros(B, T, 2 * H, dtype=F64)
    acts, cs = [], []
    for d in range(2):
        W = w_hh[d].to(F64)
        act, c = torch.zeros(B, T, H, 4, dtype=F64), torch.zeros(B, T, H, dtype=F64)
        h_run, c_run = torch.zeros(B, H, dtype=F64), torch.zeros(B, H, dtype=F64)
        for t in _order(d, T):
            on = (t < lens)[:, None]
            z = gx[d][:, t].to(F64) + h_run @ W.t()
            a, cn, h = fwd_step(z.view(B, H, 4), c_run)
            h_run, c_run = torch.where(on, h, h_run), torch.where(on, cn, c_run)
            y[:, t, d * H:(d + 1) * H] = torch.where(on, h, torch.zeros_like(h))
            act[:, t], c[:, t] = a * on[..., None], cn * on
        acts.append(act.view(B, T, G)); cs.append(c)
    return y, acts, cs


def blstm_free_bwd(dy, act, c, w_hh, lens):
    """the gradient wrt the gate pre-activations, fp64: dy [B][T][2H], act / c of blstm_free -> dz [2] [B][T][4H]"""
    B, T, G = act[0].shape
    H = G // 4
    out = []
    for d in range(2):
        W = w_hh[d].to(F64)
        dz = torch.zeros(B, T, G, dtype=F64)
        carry, dz_prev = torch.zeros(B, H, dtype=F64), torch.zeros(B, G, dtype=F64)
        for t in _order(d, T, backward=True):
            on = (t < lens)[:, None]
            tp = t - 1 if d == 0 else t + 1
            first = _first_mask(d, t, lens)[:, None]
            cp = torch.where(first, torch.zeros(B, H, dtype=F64), c[d][:, tp] if 0 <= tp < T else torch.zeros(B, H, dtype=F64))
            dh = dy[:, t, d * H:(d + 1) * H].to(F64) + dz_prev @ W
            dzt, dc = bwd_step(dh, act[d][:, t].view(B, H, 4), c[d][:, t], cp, carry)
            dzt = dzt.view(B, G) * on
            carry = torch.where(on, dc * act[d][:, t].view(B, H, 4)[..., 1], carry)
            dz[:, t] = dzt
            dz_prev = dzt
        out.append(dz)
    return out


# ---------------------------------------------------------------- checkers
class Worst(dict):
    """tolerance class -> worst err / bound seen"""
    def within(self, err, bound, cls, what):
        bad = ~(err <= bound)                                    # (a NaN on either side counts as over)
        finite = torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))
        ratio = float(finite.max()) if err.numel() else 0.0
        self[cls] = max(self.get(cls, 0.0), ratio)
        assert not bad.any(), (cls, what, "worst err / bound", ratio, "elements over", int(bad.sum()), "first", torch.nonzero(bad)[:4].tolist())


def _bits32(x):
    return x.contiguous().view(torch.int32)


def _bits16(x):
    return x.contiguous().view(torch.int16)


def _sig_bound(z, zb, s):
    """allowed |fp32 sigmoid - s| for s = sigmoid(z) in fp64 when the fp32 argument is within zb of z:
    zb through the largest derivative over [z - zb, z + zb] (taken at the point nearest 0); GPU_EXP_ALLOWANCE ulps of the value for __expf, the
    addition and the division; __expf(x) = exp2(x log2 e) rounds its scaled argument: a relative |z| 2^-24 on e^-z, s (1 - s) times that on s"""
    za = (z.abs() - zb).clamp_min(0.0)
    sa = _sig(za)
    return zb * sa * (1.0 - sa) + GPU_EXP_ALLOWANCE * ULP32 * s + z.abs() * U24 * s * (1.0 - s) + TINY32


def _tanh_bound(z, zb, v):
    """the same for tanhf (no scaled argument: the |z| term is the exponential's alone)"""
    ta = torch.tanh((z.abs() - zb).clamp_min(0.0))
    return zb * (1.0 - ta * ta) + GPU_EXP_ALLOWANCE * ULP32 * v.abs() + TINY32


def check_fwd(lens, gx, whh16, y16, act, c, worst, what=""):
    """everything the forward recurrence wrote for (lens, gx, whh16), step by step on the values the kernel read (module docstring)"""
    B, T, G = gx[0].shape
    H, KP = G // 4, whh16[0].shape[1]
    lens = lens.long()
    yv = y16.to(F64)
    zero = torch.zeros(B, H, dtype=F64)
    for d in range(2):
        W = whh16[d][:, :H].to(F64)
        assert (_bits16(whh16[d][:, H:]) == 0).all(), "pad columns of whh16 must be +0"
        for t in range(T):
            on = t < lens
            # -- outside the sequence: y16 +0, act / c never written
            assert (_bits16(y16[~on, t, d * H:(d + 1) * H]) == 0).all(), ("y16 outside the sequence is not +0", what, d, t)
            assert (_bits32(act[d][~on, t]) == NAN_BITS).all() and (_bits32(c[d][~on, t]) == NAN_BITS).all(), ("act / c written at t >= len", what, d, t)
            if not on.any():
                continue
            tp = t - 1 if d == 0 else t + 1
            has_prev = (on & ~_first_mask(d, t, lens))[:, None]
            if 0 <= tp < T:
                h_prev = torch.where(has_prev, yv[:, tp, d * H:(d + 1) * H], zero)
                c_prev = torch.where(has_prev, c[d][:, tp].to(F64), zero)
            else:
                h_prev, c_prev = zero, zero
            g_t = gx[d][:, t].to(F64)
            z = (g_t + h_prev @ W.t()).view(B, H, 4)
            # z: an fp32 sum of H products (exact in fp32: bf16 x bf16) and gx over KP + 1 additions, in any order or grouping -- four partial
            # chains (per-step) or one (resident): |err| <= (KP + 2) 2^-24 (sum |h_prev W| + |gx|)
            zb = ((KP + 2) * U24 * (h_prev.abs() @ W.abs().t() + g_t.abs())).view(B, H, 4)
            a64, c64, h64 = fwd_step(z, c_prev)
            ab = torch.stack((_sig_bound(z[..., 0], zb[..., 0], a64[..., 0]), _sig_bound(z[..., 1], zb[..., 1], a64[..., 1]),
                              _tanh_bound(z[..., 2], zb[..., 2], a64[..., 2]), _sig_bound(z[..., 3], zb[..., 3], a64[..., 3])), dim=-1)
            got_a = act[d][:, t].to(F64).view(B, H, 4)
            worst.within((got_a - a64).abs()[on], ab[on], "fwd act", (what, d, t))
            # c = f c_prev + i g: the gates' bounds through the two products (c_prev is the kernel's own, exact), three fp32 roundings
            i64, f64, g64, o64 = a64.unbind(-1)
            bi, bf, bg, bo = ab.unbind(-1)
            cb = c_prev.abs() * bf + g64.abs() * bi + (i64 + bi) * bg + 3.0 * U24 * ((f64 * c_prev).abs() + (i64 * g64).abs()) + TINY32
            worst.within((c[d][:, t].to(F64) - c64).abs()[on], cb[on], "fwd c", (what, d, t))
            # h = o tanh(c): c's bound through tanh's largest derivative nearby, the allowance on tanhf, one product
            tc = torch.tanh(c64)
            tb = _tanh_bound(c64, cb, tc)
            hb = o64 * tb + (tc.abs() + tb) * bo + U24 * h64.abs()
            # y16: one rounding to bf16 on top -- half a bf16 ulp of the largest magnitude the fp32 h may have -- and the flush threshold
            yb = hb + bf16_half_ulp(h64.abs() + hb) + TINY32
            worst.within((yv[:, t, d * H:(d + 1) * H] - h64).abs()[on], yb[on], "fwd y16", (what, d, t))


def check_bwd(lens, dy, act, c, whhT16, dz16, worst, what=""):
    """everything the backward recurrence wrote: dh of a step is recomputed from the kernel's own bf16 dz16 of the step processed before; the
    dL/dc carry is stored nowhere, so the reference carries its own and an error bound beside it: bound_t = local_t + f bound_next (f < 1)"""
    B, T, G = act[0].shape
    H = G // 4
    lens = lens.long()
    zero = torch.zeros(B, H, dtype=F64)
    for d in range(2):
        WT = whhT16[d].to(F64)                                   # [H][4H]
        dzv = dz16[d].to(F64)
        carry, carry_b = zero.clone(), zero.clone()
        steps = _order(d, T, backward=True)
        for s, t in enumerate(steps):
            on = t < lens
            assert (_bits16(dz16[d][~on, t]) == 0).all(), ("dz16 outside the sequence is not +0", what, d, t)
            if not on.any():
                continue
            onc = on[:, None]
            dz_next = torch.where(onc, dzv[:, steps[s - 1]], torch.zeros(B, G, dtype=F64)) if s > 0 else torch.zeros(B, G, dtype=F64)
            dy_t = dy[:, t, d * H:(d + 1) * H].to(F64)
            dh = dy_t + dz_next @ WT.t()
            # dh: an fp32 sum of 4H exact products and dy, four partial chains in either form: (4H + 2) 2^-24 (sum |dz W| + |dy|)
            dhb = (G + 2) * U24 * (dz_next.abs() @ WT.abs().t() + dy_t.abs())
            a = torch.where(onc[..., None], act[d][:, t].to(F64).view(B, H, 4), torch.zeros(B, H, 4, dtype=F64))
            cn = torch.where(onc, c[d][:, t].to(F64), zero)
            tp = t - 1 if d == 0 else t + 1
            first = _first_mask(d, t, lens)[:, None]             # c_prev = 0 at the first forward step of the sequence
            cp = torch.where(onc & ~first, c[d][:, tp].to(F64), zero) if 0 <= tp < T else zero
            last = _last_mask(d, t, lens)[:, None]               # nothing flows into the last forward step
            cin, cin_b = torch.where(last, zero, carry), torch.where(last, zero, carry_b)
            dz64, dc = bwd_step(dh, a, cn, cp, cin)
            i, f, g, o = a.unbind(-1)
            tc = torch.tanh(cn)
            tcb = GPU_EXP_ALLOWANCE * ULP32 * tc.abs()           # tanhf of the saved (exact) c
            one_m = 1.0 - tc * tc
            one_mb = 2.0 * tc.abs() * tcb + 2.0 * U24            # 1 - tc^2: tc's error, the square and the difference (each <= 2^-24 absolute)
            # dc = dh o (1 - tc^2) + carry: dh's bound and (1 - tc^2)'s through the product, its two roundings, the carry's bound, the sum's rounding
            local = dhb * o * one_m + (dh.abs() + dhb) * o * one_mb + 2.0 * U24 * (dh * o * one_m).abs() + U24 * dc.abs()
            dcb = local + cin_b
            # the four gate formulas: dc's (dh's) bound through the factors, then one rounding per operation relative to the result; 1 - g^2 is
            # rounded absolutely (<= 2 2^-24) like 1 - tc^2
            dc_hi, dh_hi = dc.abs() + dcb, dh.abs() + dhb
            zb = torch.stack((dcb * (g * i * (1.0 - i)).abs() + 5.0 * U24 * dz64[..., 0].abs(),
                              dcb * (cp * f * (1.0 - f)).abs() + 5.0 * U24 * dz64[..., 1].abs(),
                              dcb * (i * (1.0 - g * g)).abs() + dc_hi * i * 2.0 * U24 + 3.0 * U24 * dz64[..., 2].abs(),
                              dhb * (tc * o * (1.0 - o)).abs() + dh_hi * o * (1.0 - o) * tcb + 5.0 * U24 * dz64[..., 3].abs()), dim=-1)
            # dz16: one rounding to bf16 on top (half a bf16 ulp of the largest magnitude the fp32 value may have) and the flush threshold
            zb = zb + bf16_half_ulp(dz64.abs() + zb) + TINY32
            got = dzv[:, t].view(B, H, 4)
            for k, name in enumerate(("i", "f", "g", "o")):
                worst.within((got[..., k] - dz64[..., k]).abs()[on], zb[..., k][on], "bwd dz16 " + name, (what, d, t))
            # the carry into the step processed next: dc f, one more rounding
            carry = torch.where(onc, dc * f, carry)
            carry_b = torch.where(onc, dcb * f + U24 * (dc * f).abs(), carry_b)


# ---------------------------------------------------------------- inputs
# (H, B, T): every H / B / T of the issue's table and every (KS, MT) / (KQ, MT) instantiation of the resident kernels
#   KS = KP / 32 rounded up to 4 / 8 / 12, KQ = ceil(H / 32) likewise, MT = 1 (B <= 16) or 2
COMBOS = (
    (8, 1, 1),       # KS 4  KQ 4  MT 1   one k-step, no exchange at all
    (8, 17, 5),      # KS 4  KQ 4  MT 2   three idle waves per step
    (40, 3, 2),      # KS 4  KQ 4  MT 1   2 slices of 20
    (40, 32, 12),    # KS 4  KQ 4  MT 2   both buffer parities reused
    (136, 16, 5),    # KS 8  KQ 8  MT 1   KP 160, 5 slices of 28, the last with 24: masked waves
    (136, 17, 12),   # KS 8  KQ 8  MT 2
    (256, 3, 12),    # KS 8  KQ 8  MT 1   full slices
    (256, 32, 2),    # KS 8  KQ 8  MT 2
    (360, 16, 12),   # KS 12 KQ 12 MT 1   KP 384, last slice of 8
    (360, 17, 5),    # KS 12 KQ 12 MT 2
    (360, 1, 2),     # KS 12 KQ 12 MT 1   one row, a padded frame
    (40, 33, 5),     # per-step only: three row tiles; the resident form refuses B > 32
)


def make_lens(B, T, g):
    """always T, 1 and a value in between, not sorted (as far as B and T leave room: B = 1 takes the shortest that still has a step before it)"""
    mid = max(1, (T + 1) // 2)
    base = [mid, T, 1]
    if B == 1:
        return torch.tensor([max(1, T - 1)], dtype=torch.int32)
    extra = torch.randint(1, T + 1, (max(0, B - 3),), generator=g).tolist()
    return torch.tensor((base + extra)[:B], dtype=torch.int32)


def make_case(H, B, T, seed=0):
    """seeded operands of one recurrence case (CPU tensors): gx scaled per (row, unit) so that gates cover the linear and the saturated range,
    W_hh ~ U(-1/sqrt(H), 1/sqrt(H)) * 2 (torch's init range, doubled so that the recurrent term matters), dy and gx non-zero at padded frames too"""
    g = torch.Generator().manual_seed(1000003 * H + 1009 * B + T + seed)
    lens = make_lens(B, T, g)
    G, KP = 4 * H, kp_of(H)
    scale = torch.tensor([0.3, 1.5, 5.0])[torch.randint(0, 3, (2, B, T, H, 1), generator=g)]
    gxs = (torch.randn(2, B, T, H, 4, generator=g) * scale).view(2, B, T, G).float()
    w = (torch.rand(2, G, H, generator=g) * 2.0 - 1.0) * (2.0 / H ** 0.5)          # unit-major rows already
    whh16 = torch.zeros(2, G, KP, dtype=torch.bfloat16)
    whh16[:, :, :H] = w.bfloat16()
    whhT16 = whh16[:, :, :H].transpose(1, 2).contiguous()
    dy = torch.randn(B, T, 2 * H, generator=g).float()
    return dict(H=H, B=B, T=T, KP=KP, lens=lens, gx=[gxs[0].contiguous(), gxs[1].contiguous()], whh16=[whh16[0].contiguous(), whh16[1].contiguous()],
                whhT16=[whhT16[0].contiguous(), whhT16[1].contiguous()], dy=dy)


# ---------------------------------------------------------------- an honest fp32 emulation of the kernels (and mutated ones)
F32 = torch.float32
FWD_MUTATIONS = ("gate_order", "reverse_from_T", "past_len", "c0_stale", "h_unrounded", "neighbour_unit", "torch_rows")
BWD_MUTATIONS = ("gate_order", "cprev_first", "carry_last", "neighbour_unit", "torch_rows")


def _chains(a, w, resident, backward):
    """fp32 a [B][K] . w [N][K]^T accumulated MFMA k-step by k-step (32 wide) in the kernels' grouping: forward per-step = four chains over
    the k-steps w, w + 4, ..; forward resident = one chain; backward = four chains (per-step: k-steps w, w + 4, ..; resident: four contiguous
    quarters); the four meet as (0 + 1) + (2 + 3)"""
    K = a.shape[1]
    nks = (K + 31) // 32
    if resident and not backward:
        groups = [list(range(nks))]
    elif resident:
        q = (nks + 3) // 4
        groups = [list(range(i * q, min((i + 1) * q, nks))) for i in range(4)]
    else:
        groups = [list(range(i, nks, 4)) for i in range(4)]
    part = []
    for ks in groups:
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
        for k in ks:
            acc = acc + a[:, 32 * k:32 * k + 32] @ w[:, 32 * k:32 * k + 32].t()
        part.append(acc)
    return part[0] if len(part) == 1 else (part[0] + part[1]) + (part[2] + part[3])


def emulate_fwd(case, resident, mut=None):
    """fp32 arithmetic, h exchanged as bf16 -> y16, act [2], c [2] with NaN where the kernels do not write"""
    H, B, T, KP = case["H"], case["B"], case["T"], case["KP"]
    G = 4 * H
    lens = case["lens"].long()
    y16 = torch.zeros(B, T, 2 * H, dtype=torch.bfloat16)
    acts, cs = [], []
    for d in range(2):
        W = case["whh16"][d].float()
        if mut == "torch_rows":                                  # W_hh rows taken in torch's order g H + u where u 4 + g is stored
            W = W[unit_major_rows(H)]
        act, c = torch.full((B, T, G), float("nan")), torch.full((B, T, H), float("nan"))
        h_run = torch.zeros(B, KP, dtype=F32)
        c_run = torch.full((B, H), 0.25 if mut == "c0_stale" else 0.0, dtype=F32)
        for t in _order(d, T):
            on = (t < lens)[:, None]
            if mut == "past_len":                                # the lengths ignored: every step advances and writes
                on = torch.ones_like(on)
            z = (_chains(h_run, W, resident, False) + case["gx"][d][:, t]).view(B, H, 4)
            if mut == "gate_order":                              # i, g, f, o
                z = z[..., [0, 2, 1, 3]]
            if mut == "neighbour_unit":                          # the last unit takes its four gate columns from the unit before it
                z = torch.cat((z[:, :-1], z[:, -2:-1]), dim=1) if H > 1 else z
            a, cn, h = fwd_step(z, c_run)
            adv = on | (d == 1) if mut == "reverse_from_T" else on     # the reverse direction running from T - 1 through the padding
            h_keep = h if mut == "h_unrounded" else h.bfloat16().float()
            h_run = torch.cat((torch.where(adv, h_keep, h_run[:, :H]), h_run[:, H:]), dim=1)
            c_run = torch.where(adv, cn, c_run)
            y16[:, t, d * H:(d + 1) * H] = torch.where(on, h, torch.zeros_like(h)).bfloat16()
            act[:, t] = torch.where(on, a.view(B, G), act[:, t])
            c[:, t] = torch.where(on, cn, c[:, t])
        acts.append(act); cs.append(c)
    return y16, acts, cs


def emulate_bwd(case, act, c, resident, mut=None):
    """fp32 arithmetic, dz exchanged as bf16 -> dz16 [2]"""
    H, B, T = case["H"], case["B"], case["T"]
    G = 4 * H
    lens = case["lens"].long()
    out = []
    for d in range(2):
        WT = case["whhT16"][d].float()
        if mut == "torch_rows":
            WT = WT[:, unit_major_rows(H)]
        dz16 = torch.zeros(B, T, G, dtype=torch.bfloat16)
        carry = torch.zeros(B, H, dtype=F32)
        dz_prev = torch.zeros(B, G, dtype=F32)
        for t in _order(d, T, backward=True):
            on = (t < lens)[:, None]
            dy_t = case["dy"][:, t, d * H:(d + 1) * H]
            dh = dy_t + _chains(dz_prev, WT, resident, True)
            a = torch.nan_to_num(act[d][:, t]).view(B, H, 4)
            if mut == "gate_order":
                a = a[..., [0, 2, 1, 3]]
            if mut == "neighbour_unit" and H > 1:
                a = torch.cat((a[:, :-1], a[:, -2:-1]), dim=1)
            cn = torch.nan_to_num(c[d][:, t])
            tp = t - 1 if d == 0 else t + 1
            first = _first_mask(d, t, lens)[:, None]
            cp = torch.nan_to_num(c[d][:, tp]) if 0 <= tp < T else torch.zeros(B, H)
            cp = torch.where(first, cn if mut == "cprev_first" else torch.zeros(B, H), cp)      # mutated: a c_prev that is not zero
            last = _last_mask(d, t, lens)[:, None]
            cin = carry if mut == "carry_last" else torch.where(last, torch.zeros(B, H), carry)
            dzt, dc = bwd_step(dh, a, cn, cp, cin)
            dzt = torch.where(on, dzt.view(B, G), torch.zeros(B, G)).bfloat16()
            if mut == "carry_last":                              # the padded frames feed the carry and the last step does not clear it
                carry = torch.where(on, dc * a[..., 1], dy_t)
            else:
                carry = torch.where(on, dc * a[..., 1], carry)
            dz16[:, t] = dzt
            dz_prev = dzt.float()
        out.append(dz16)
    return out
