"""The BLSTM path's LSTM kernels one by one (include/masr_test.h masr_test_lstm_* and the small kernels of csrc/lstm.hip) against the plain
restatements and checkers of tests/lstm_ref.py: the recurrence forward and backward in both forms (one launch per timestep; the resident
one-launch form of csrc/lstm_rec.hip), each checked step by step in fp64 on exactly the values the kernel read; the weight shadows, the
gradient un-permutation, hprev, cast_rows_pad, mask_rows and subsample_rows bit for bit; tanh forward / backward within derived bounds.
Every region a launch must not touch is filled with NaN and compared bit for bit afterwards.  The recurrence cases are lstm_ref.COMBOS (the
list says which template instantiation each one runs); tests/test_lstm_ref_cpu.py passes an fp32 emulation through the same checkers and
fails mutated ones.  The worst err / bound of each tolerance class is printed at teardown (pytest -s)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
import lstm_ref as L  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
BF16 = torch.bfloat16
F64 = torch.float64
WORST = L.Worst()


@pytest.fixture(scope="module")
def lib():
    yield _cabi.lib()
    print("\nworst err / bound per tolerance class:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {BF16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}[a.dtype]
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def nan_rows(rows, cols, dtype=torch.float32):
    """[rows + 2][cols] of NaN: the launch's output with two sentinel rows behind it"""
    return torch.full((rows + 2, cols), NAN, device=DEV, dtype=dtype)


def tail_intact(*outs):
    for o in outs:
        assert torch.isnan(o[-2:]).all(), "a sentinel row behind the output was written"


def refused(lib, rc, needle=""):
    text = lib.masr_last_error().decode()
    assert rc < 0 and text and needle in text, (rc, text)


# ---------------------------------------------------------------- the recurrence
_CASES = {}


def case_on_device(H, B, T):
    if (H, B, T) not in _CASES:
        cs = L.make_case(H, B, T)
        dv = {k: ([x.to(DEV) for x in v] if isinstance(v, list) else v.to(DEV)) for k, v in cs.items() if not isinstance(v, int)}
        _CASES[(H, B, T)] = (cs, dv)
    return _CASES[(H, B, T)]


def launch_fwd(lib, dv, H, B, T, resident):
    R, G = B * T, 4 * H
    y16 = nan_rows(R, 2 * H, BF16)
    act, c = [nan_rows(R, G), nan_rows(R, G)], [nan_rows(R, H), nan_rows(R, H)]
    rc = lib.masr_test_lstm_fwd(resident, B, T, H, P(dv["lens"]), P(dv["gx"][0]), P(dv["gx"][1]), P(dv["whh16"][0]), P(dv["whh16"][1]), P(y16),
                                P(act[0]), P(act[1]), P(c[0]), P(c[1]), S())
    torch.cuda.synchronize()
    return rc, y16, act, c


def launch_bwd(lib, dv, act, c, H, B, T, resident):
    R, G = B * T, 4 * H
    dz = [nan_rows(R, G, BF16), nan_rows(R, G, BF16)]
    rc = lib.masr_test_lstm_bwd(resident, B, T, H, P(dv["lens"]), P(dv["dy"]), P(act[0]), P(act[1]), P(c[0]), P(c[1]), P(dv["whhT16"][0]),
                                P(dv["whhT16"][1]), P(dz[0]), P(dz[1]), S())
    torch.cuda.synchronize()
    return rc, dz


_STEPS_FWD = {}


def steps_forward(lib, H, B, T):
    """the per-step forward of a case, run once: what the backward launches of the case are fed"""
    if (H, B, T) not in _STEPS_FWD:
        _, dv = case_on_device(H, B, T)
        rc, y16, act, c = launch_fwd(lib, dv, H, B, T, 0)
        _cabi.check(rc, "lstm_fwd")
        _STEPS_FWD[(H, B, T)] = (y16, act, c)
    return _STEPS_FWD[(H, B, T)]


@pytest.mark.parametrize("resident", (0, 1))
@pytest.mark.parametrize("H,B,T", L.COMBOS)
def test_lstm_forward(lib, H, B, T, resident):
    cs, dv = case_on_device(H, B, T)
    if resident and B > 32:                                      # the resident form holds two row tiles: it must refuse, and write nothing
        rc, y16, act, c = launch_fwd(lib, dv, H, B, T, 1)
        refused(lib, rc, "resident")
        assert torch.isnan(y16).all() and all(torch.isnan(x).all() for x in act + c)
        return
    rc, y16, act, c = launch_fwd(lib, dv, H, B, T, resident) if resident else (0,) + steps_forward(lib, H, B, T)
    _cabi.check(rc, "lstm_fwd")
    tail_intact(y16, *act, *c)
    R = B * T
    L.check_fwd(cs["lens"], cs["gx"], cs["whh16"], y16[:R].cpu().view(B, T, 2 * H), [a[:R].cpu().view(B, T, 4 * H) for a in act],
                [x[:R].cpu().view(B, T, H) for x in c], WORST, (H, B, T, resident))
    if resident:                                                 # a second launch on the same inputs: the same bits
        rc, y2, act2, c2 = launch_fwd(lib, dv, H, B, T, 1)
        _cabi.check(rc, "lstm_fwd")
        assert same_bits(y16, y2) and all(same_bits(a, b) for a, b in zip(act + c, act2 + c2))


@pytest.mark.parametrize("resident", (0, 1))
@pytest.mark.parametrize("H,B,T", L.COMBOS)
def test_lstm_backward(lib, H, B, T, resident):
    cs, dv = case_on_device(H, B, T)
    _, act, c = steps_forward(lib, H, B, T)
    if resident and B > 32:
        rc, dz = launch_bwd(lib, dv, act, c, H, B, T, 1)
        refused(lib, rc, "resident")
        assert torch.isnan(dz[0]).all() and torch.isnan(dz[1]).all()
        return
    act0 = [a.clone() for a in act + c]
    rc, dz = launch_bwd(lib, dv, act, c, H, B, T, resident)
    _cabi.check(rc, "lstm_bwd")
    tail_intact(*dz)
    assert all(same_bits(a, b) for a, b in zip(act + c, act0)), "the backward wrote into the saved forward values"
    R = B * T
    L.check_bwd(cs["lens"], cs["dy"], [a[:R].cpu().view(B, T, 4 * H) for a in act], [x[:R].cpu().view(B, T, H) for x in c], cs["whhT16"],
                [z[:R].cpu().view(B, T, 4 * H) for z in dz], WORST, (H, B, T, resident))
    if resident:
        rc, dz2 = launch_bwd(lib, dv, act, c, H, B, T, 1)
        _cabi.check(rc, "lstm_bwd")
        assert same_bits(dz[0], dz2[0]) and same_bits(dz[1], dz2[1])


def test_lstm_refusals(lib):
    """lens outside [1, T] (both forms), shapes the resident form does not hold, 4H % 32 in the backward: < 0 with a text, nothing written"""
    def attempt(H, B, T, lens, resident, fwd, needle):
        R, G, KP = B * T, 4 * H, L.kp_of(H)
        lens_d = torch.tensor(lens, device=DEV, dtype=torch.int32)
        gx, whh = torch.zeros(R, G, device=DEV), torch.zeros(G, KP, device=DEV, dtype=BF16)
        y16, act, c, dz = nan_rows(R, 2 * H, BF16), nan_rows(R, G), nan_rows(R, H), nan_rows(R, G, BF16)
        if fwd:
            rc = lib.masr_test_lstm_fwd(resident, B, T, H, P(lens_d), P(gx), P(gx), P(whh), P(whh), P(y16), P(act), P(act), P(c), P(c), S())
        else:
            dy, whhT = torch.zeros(R, 2 * H, device=DEV), torch.zeros(H, G, device=DEV, dtype=BF16)
            act.zero_(); c.zero_()
            rc = lib.masr_test_lstm_bwd(resident, B, T, H, P(lens_d), P(dy), P(act), P(act), P(c), P(c), P(whhT), P(whhT), P(dz), P(dz), S())
        torch.cuda.synchronize()
        refused(lib, rc, needle)
        assert torch.isnan(y16).all() and torch.isnan(dz).all() and (not fwd or (torch.isnan(act).all() and torch.isnan(c).all()))
    for resident in (0, 1):
        for fwd in (True, False):
            attempt(8, 3, 4, [4, 0, 2], resident, fwd, "lens")
            attempt(8, 3, 4, [4, 5, 2], resident, fwd, "lens")
            attempt(8, 3, 4, [-1, 4, 2], resident, fwd, "lens")
    for fwd in (True, False):
        attempt(40, 33, 2, [2] * 33, 1, fwd, "resident")       # three row tiles
        attempt(392, 1, 1, [1], 1, fwd, "resident")             # KP 416 > 384
    attempt(12, 2, 2, [2, 1], 1, True, "resident")              # 4H = 48: no whole k-steps
    attempt(12, 2, 2, [2, 1], 0, False, "multiple of 32")
    attempt(12, 2, 2, [2, 1], 1, False, "multiple of 32")


# ---------------------------------------------------------------- the weight shadows and the gradient un-permutation: bit for bit
# (H, K, pc, pd): 4H = 96 and H = 24 ragged in the transpose's 64 x 64 tiles, K = 100 no multiple of 64; the NHWC column permutation through
# LDS (K = 640); K * 4 bytes = 66560 > 64 KB: the element-per-thread fallback
SHADOW_CASES = ((24, 100, 0, 0), (40, 640, 128, 5), (8, 16640, 128, 130), (72, 64, 0, 0))


@pytest.mark.parametrize("H,K,pc,pd", SHADOW_CASES)
def test_lstm_shadows_bit_exact(lib, H, K, pc, pd):
    g = torch.Generator().manual_seed(H + K)
    G, KP = 4 * H, L.kp_of(H)
    wih, whh = torch.randn(G, K, generator=g), torch.randn(G, H, generator=g)
    bih, bhh = torch.randn(G, generator=g), torch.randn(G, generator=g)
    wih16, wihT16, whh16, whhT16 = nan_rows(G, K, BF16), nan_rows(K, G, BF16), nan_rows(G, KP, BF16), nan_rows(H, G, BF16)
    bias = torch.full((G + 2,), NAN, device=DEV)
    d = [t.to(DEV) for t in (wih, whh, bih, bhh)]               # (kept alive over the launch)
    _cabi.check(lib.masr_test_lstm_shadows(P(d[0]), P(d[1]), P(d[2]), P(d[3]), H, K, pc, pd, P(wih16), P(wihT16), P(whh16), P(whhT16), P(bias), S()),
                "lstm_shadows")
    torch.cuda.synchronize()
    tail_intact(wih16, wihT16, whh16, whhT16, bias)
    # the only arithmetic: one fp32 -> bf16 rounding per element, and b_ih + b_hh in fp32
    want = L.shadows(wih, whh, bih, bhh, H, K, pc, pd)
    for name, got, ref in zip(("wih16", "wihT16", "whh16", "whhT16", "bias"), (wih16[:G], wihT16[:K], whh16[:G], whhT16[:H], bias[:G]), want):
        assert same_bits(got.cpu(), ref), (name, H, K, pc, pd)
    assert (whh16[:G, H:].cpu().view(torch.int16) == 0).all(), "pad columns H .. KP of whh16 must be +0"


@pytest.mark.parametrize("H,K,pc,pd,two", [(24, 1, 0, 0, True), (24, 100, 0, 0, False), (40, 640, 128, 5, False), (8, 16640, 128, 130, False),
                                           (8, 640, 128, 5, True)])
def test_lstm_unperm_bit_exact(lib, H, K, pc, pd, two):
    g = torch.Generator().manual_seed(7 * H + K)
    G = 4 * H
    src = torch.randn(G, K, generator=g)
    dst, dst2 = nan_rows(G, K), nan_rows(G, K)
    src_d = src.to(DEV)
    _cabi.check(lib.masr_test_lstm_unperm(P(src_d), P(dst), P(dst2) if two else None, H, K, pc, pd, S()), "lstm_unperm")
    torch.cuda.synchronize()
    tail_intact(dst, dst2)
    want = L.unperm(src, H, K, pc, pd)
    assert same_bits(dst[:G].cpu(), want)
    assert same_bits(dst2[:G].cpu(), want) if two else bool(torch.isnan(dst2).all())


def test_shadow_refusals(lib):
    H, K = 8, 12
    z = torch.zeros(4 * H, K, device=DEV)
    o16, o32 = nan_rows(4 * H, 32, BF16), nan_rows(4 * H, K)
    refused(lib, lib.masr_test_lstm_shadows(P(z), P(z), P(z), P(z), H, K, 5, 2, P(o16), P(o16), P(o16), P(o16), P(o32), S()), "pc * pd")
    refused(lib, lib.masr_test_lstm_unperm(P(z), P(o32), None, H, K, 4, 2, S()), "pc * pd")
    torch.cuda.synchronize()
    assert torch.isnan(o16).all() and torch.isnan(o32).all()


# ---------------------------------------------------------------- the small kernels
def rand_bf16(shape, g):
    return torch.randn(*shape, generator=g).bfloat16()


@pytest.mark.parametrize("B,T,H,KP", [(3, 5, 40, 64), (2, 1, 8, 32), (4, 7, 64, 64)])
def test_lstm_hprev_bit_exact(lib, B, T, H, KP):
    y = rand_bf16((B, T, 2 * H), torch.Generator().manual_seed(B + T))
    hp0, hp1 = nan_rows(B * T, KP, BF16), nan_rows(B * T, KP, BF16)
    y_d = y.to(DEV)
    _cabi.check(lib.masr_test_lstm_hprev(P(y_d), P(hp0), P(hp1), B, T, H, KP, S()), "lstm_hprev")
    torch.cuda.synchronize()
    tail_intact(hp0, hp1)
    w0, w1 = torch.zeros(B, T, KP, dtype=BF16), torch.zeros(B, T, KP, dtype=BF16)
    w0[:, 1:, :H] = y[:, :-1, :H]                               # direction 0: the row before; t = 0 and the pad columns zero
    w1[:, :-1, :H] = y[:, 1:, H:]                               # direction 1: the row after; t = T - 1 zero (not the next sequence's first row)
    assert same_bits(hp0[:B * T].cpu().view(B, T, KP), w0) and same_bits(hp1[:B * T].cpu().view(B, T, KP), w1)
    refused(lib, lib.masr_test_lstm_hprev(P(y_d), P(hp0), P(hp1), B, T, H, H - 1, S()), "KP < H")


@pytest.mark.parametrize("rows,C_,Cp", [(37, 367, 368), (5, 64, 64), (3, 1, 32)])
def test_cast_rows_pad_bit_exact(lib, rows, C_, Cp):
    x = torch.randn(rows, C_, generator=torch.Generator().manual_seed(C_)) * 3.0
    y = nan_rows(rows, Cp, BF16)
    x_d = x.to(DEV)
    _cabi.check(lib.masr_test_cast_rows_pad(P(x_d), P(y), rows, C_, Cp, S()), "cast_rows_pad")
    torch.cuda.synchronize()
    tail_intact(y)
    want = torch.zeros(rows, Cp, dtype=BF16)
    want[:, :C_] = x.bfloat16()
    assert same_bits(y[:rows].cpu(), want)
    refused(lib, lib.masr_test_cast_rows_pad(P(x_d), P(y), rows, C_, C_ - 1, S()), "Cp < C")


@pytest.mark.parametrize("which", ("both", "x32", "x16"))
def test_mask_rows(lib, which):
    B, T, C_ = 4, 5, 67                                         # B T C = 1340: no multiple of 256
    g = torch.Generator().manual_seed(11)
    lens = torch.tensor([5, 1, 3, 0], dtype=torch.int32)
    x32 = torch.cat((torch.randn(B * T, C_, generator=g), torch.full((2, C_), NAN)))
    x16 = x32.bfloat16()
    d32, d16, lens_d = x32.to(DEV), x16.to(DEV), lens.to(DEV)
    _cabi.check(lib.masr_test_mask_rows(P(d32) if which != "x16" else None, P(d16) if which != "x32" else None, P(lens_d), B, T, C_, S()), "mask_rows")
    torch.cuda.synchronize()
    keep = (torch.arange(T)[None, :] < lens[:, None]).reshape(B * T, 1)
    keep = torch.cat((keep, torch.ones(2, 1, dtype=torch.bool)))
    w32 = torch.where(keep, x32, torch.zeros_like(x32)) if which != "x16" else x32
    w16 = torch.where(keep, x16, torch.zeros_like(x16)) if which != "x32" else x16
    assert same_bits(d32.cpu(), w32) and same_bits(d16.cpu(), w16)         # masked rows +0, every other bit (sentinel rows included) as it was


@pytest.mark.parametrize("sub", (1, 2, 3))
def test_subsample_rows_forward_backward(lib, sub):
    B, Tin = 3, 7                                               # 7: no multiple of 2 or 3
    Tout = (Tin + sub - 1) // sub
    g = torch.Generator().manual_seed(sub)
    C8, C4 = 264, 260                                           # more than one block; C4: a multiple of 4 and not of 8
    y = rand_bf16((B, Tin, C8), g)
    ys = nan_rows(B * Tout, C8, BF16)
    y_d = y.to(DEV)
    _cabi.check(lib.masr_test_subsample_rows(P(y_d), P(ys), None, None, B, Tin, Tout, sub, C8, S()), "subsample_rows")
    torch.cuda.synchronize()
    tail_intact(ys)
    assert same_bits(ys[:B * Tout].cpu().view(B, Tout, C8), y[:, ::sub].contiguous())
    dys = torch.randn(B, Tout, C4, generator=g)
    dy = nan_rows(B * Tin, C4)
    dys_d = dys.to(DEV)
    _cabi.check(lib.masr_test_subsample_rows(None, None, P(dys_d), P(dy), B, Tin, Tout, sub, C4, S()), "subsample_rows_bwd")
    torch.cuda.synchronize()
    tail_intact(dy)
    want = torch.zeros(B, Tin, C4)                              # the dropped frames: exactly +0
    want[:, ::sub] = dys
    assert same_bits(dy[:B * Tin].cpu().view(B, Tin, C4), want)


def test_subsample_rows_refusals(lib):
    B, Tin = 2, 7
    y, ys = torch.zeros(B * Tin, 16, device=DEV, dtype=BF16), nan_rows(B * Tin, 16, BF16)
    dys, dy = torch.zeros(B * Tin, 16, device=DEV), nan_rows(B * Tin, 16)
    refused(lib, lib.masr_test_subsample_rows(P(y), P(ys), None, None, B, Tin, 4, 2, 12, S()), "C % 8")
    refused(lib, lib.masr_test_subsample_rows(P(y), P(ys), None, None, B, Tin, 3, 2, 16, S()), "Tout")
    refused(lib, lib.masr_test_subsample_rows(P(y), P(ys), None, None, B, Tin, 7, 0, 16, S()), "Tout")
    refused(lib, lib.masr_test_subsample_rows(None, None, P(dys), P(dy), B, Tin, 4, 2, 6, S()), "C % 4")
    refused(lib, lib.masr_test_subsample_rows(None, None, P(dys), P(dy), B, Tin, 5, 2, 16, S()), "Tout")
    torch.cuda.synchronize()
    assert torch.isnan(ys).all() and torch.isnan(dy).all()


def tanh_inputs(n, g):
    """the linear range, the saturated one (|x| up to 20: tanh is 1 to fp32 from 9.01 on) and tiny arguments"""
    x = torch.randn(n, generator=g) * torch.tensor([0.01, 1.0, 4.0, 20.0])[torch.randint(0, 4, (n,), generator=g)]
    x[:4] = torch.tensor([-25.0, 0.0, -0.0, 1e-30])[:n]
    return x.float()


@pytest.mark.parametrize("n", (1000, 257, 1))
def test_tanh_forward(lib, n):
    x = tanh_inputs(n, torch.Generator().manual_seed(n))
    y32 = torch.full((n + 2,), NAN, device=DEV)
    y16 = torch.full((n + 2,), NAN, device=DEV, dtype=BF16)
    x_d = x.to(DEV)
    _cabi.check(lib.masr_test_tanh(P(x_d), None, P(y32), P(y16), n, S()), "tanh fwd")
    torch.cuda.synchronize()
    tail_intact(y32, y16)
    want = torch.tanh(x.double())
    # the device tanhf against fp64: GPU_EXP_ALLOWANCE ulps of fp32 at the value, and the flush threshold
    WORST.within((y32[:n].cpu().double() - want).abs(), L.GPU_EXP_ALLOWANCE * L.ULP32 * want.abs() + L.TINY32, "tanh fwd", n)
    assert same_bits(y16[:n].cpu(), y32[:n].cpu().bfloat16()), "y16 is not the one rounding of y32"


@pytest.mark.parametrize("n", (1000, 257))
def test_tanh_backward(lib, n):
    g = torch.Generator().manual_seed(n + 1)
    y = torch.tanh(tanh_inputs(n, g))                           # includes y = +-1 exactly and y close to it
    dy = torch.randn(n, generator=g)
    dx = torch.full((n + 2,), NAN, device=DEV, dtype=BF16)
    y_d, dy_d = y.to(DEV), dy.to(DEV)
    _cabi.check(lib.masr_test_tanh(P(y_d), P(dy_d), None, P(dx), n, S()), "tanh bwd")
    torch.cuda.synchronize()
    tail_intact(dx)
    v = dy.double() * (1.0 - y.double() ** 2)
    # two fp32 roundings -- 1 - y^2 as one fused operation, the product -- each relative to the result, then one rounding to bf16
    b = (2.0 * L.U24 + L.U24 ** 2) * v.abs()
    WORST.within((dx[:n].cpu().double() - v).abs(), b + L.bf16_half_ulp(v.abs() + b) + L.TINY32, "tanh bwd", n)


def test_tanh_refusals(lib):
    x = torch.zeros(4, device=DEV)
    o = torch.full((4,), NAN, device=DEV, dtype=BF16)
    refused(lib, lib.masr_test_tanh(P(x), None, None, P(o), 4, S()))
    refused(lib, lib.masr_test_tanh(P(x), None, P(x), P(o), 0, S()))
    assert torch.isnan(o).all()
