"""The flat optimiser passes of csrc/optim.hip one by one against the fp64 restatements of tests/optim_ref.py: the gradient norm, clip + SGD,
clip + scale, clip + accumulate, Adam / AdamW / Adam with L2, the guarded Adam with its flag hand-over, the summed-gradient Adam and the list sum,
scale and axpy.  Every array a kernel touches is a view inside a larger allocation of marker words, 16-byte aligned or one float past such a
boundary (the scalar form), and the markers, the read-only inputs and everything under a NaN norm are compared bit for bit after each call.
Lengths: below four, around the tail, several workgroups, and one past a full grid stride of each pass.  Every tolerance is derived in
optim_ref.py or next to its assert; the worst err / bound of each class is printed (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
import optim_ref as O  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
NAN = float("nan")
GUARD = 64                                                     # marker words on either side (a multiple of four: offset 0 stays 16-byte aligned)
MARK = 0x7FC5A5A5                                              # (a NaN as a float: a marker that was read would show, too)
FLAT_NS = (1, 3, 4, 5, 1023, 4101, 10007)
BIG = 4 * 2 ** 20 + 4099                                       # past one grid stride of a flat pass: 4096 workgroups x 256 lanes x 4 floats
SS_BIG = (2 ** 20 + 7, 3 * 2 ** 20 + 5)                        # ... of sumsq_kernel: 1024 workgroups x 256 lanes x 4 floats
WORST = {}


@pytest.fixture(scope="module")
def lib():
    yield _cabi.lib()
    print("\nworst err / bound per tolerance class:", {k: round(v, 4) for k, v in WORST.items()})


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """n words of `data` (numpy float32 / int32) inside GUARD marker words on either side, `off` words past a 16-byte boundary"""

    def __init__(self, data, off=0):
        data = np.ascontiguousarray(data)
        self.n, self.lo, self.np_dtype = data.size, GUARD + off, data.dtype
        self.full = torch.full((2 * GUARD + self.n + 4,), MARK, dtype=torch.int32, device=DEV)
        self.full[self.lo:self.lo + self.n] = torch.from_numpy(data.view(np.int32).reshape(-1)).to(DEV)
        self.first = data.view(np.int32).reshape(-1).copy()

    def ptr(self, at=0):
        return C.c_void_p(self.full.data_ptr() + 4 * (self.lo + at))

    def bits(self):
        return self.full[self.lo:self.lo + self.n].cpu().numpy()

    def get(self):
        return self.bits().view(self.np_dtype)

    def guard_ok(self):
        return bool((self.full[:self.lo] == MARK).all()) and bool((self.full[self.lo + self.n:] == MARK).all())

    def untouched(self):
        return self.guard_ok() and np.array_equal(self.bits(), self.first)


def PTR(b):
    return b.ptr() if b is not None else None


@functools.lru_cache(maxsize=48)
def _rnd(seed, n, scale):
    x = (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)
    x[seed % 5::97] = 0.0                                      # exact zeros among the values
    return x


def rnd(seed, n, scale=1.0):
    return _rnd(seed, n, scale).copy()


def dev_scalar(v, dtype=F32):
    return Buf(np.array([v], dtype))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def within(got, ref, bound, cls, what):
    """|got - ref| <= bound on every element; records the worst ratio of the class"""
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), (cls, what, "non-finite")
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    assert (err <= bound).all(), (cls, what, "worst err / bound", ratio, "elements over", int((err > bound).sum()), "of", err.size)


def refused(lib, rc, fragment):
    assert rc == -1, rc
    msg = lib.masr_last_error().decode()
    assert fragment in msg, msg


def sizes_and_offsets(big=BIG):
    return [(n, off) for n in FLAT_NS for off in (0, 1)] + [(big, 0), (big, 1)]


# ---------------------------------------------------------------- the gradient norm (sumsq_kernel + sumsq_final)
def run_sumsq(lib, x):
    xb, out = Buf(x), dev_scalar(-7.0)
    _cabi.check(lib.masr_test_sumsq(xb.ptr(), x.size, out.ptr(), S()), "sumsq")
    assert xb.untouched() and out.guard_ok()
    return out.get()[0]


def check_norm(got, x, what):
    """the sum is accumulated in fp64 (n 2^-53 relative: nothing next to fp32's 2^-24), so the cast of the root is the one visible rounding, half an
    ulp <= 2^-24 ref; 2^-23 ref leaves the cast of a root that the fp64 summation order moved across a rounding boundary inside"""
    ref = O.norm(x)
    if not np.isfinite(O.norm_f32(x)):
        assert same_bits(np.array([got]), np.array([O.norm_f32(x)])) or (np.isnan(ref) and np.isnan(got)), (what, got, ref)
        return
    assert np.isfinite(got), (what, got)
    err, bound = abs(float(got) - ref), 2.0 ** -23 * ref
    WORST["norm"] = max(WORST.get("norm", 0.0), err / bound if bound else 0.0)
    assert err <= bound, (what, got, ref)


@pytest.mark.parametrize("n", FLAT_NS + SS_BIG)
def test_sumsq(lib, n):
    check_norm(run_sumsq(lib, rnd(n, n)), rnd(n, n), ("random", n))
    assert run_sumsq(lib, np.zeros(n, F32)) == 0.0
    last = np.zeros(n, F32)
    last[-1] = 3.0                                             # the last element of the tail (or of the last float4) alone
    assert run_sumsq(lib, last) == 3.0
    for val in (1e30, 3e38, 1e-30):                            # squares beyond fp32's range on either side, inside fp64's: 3e38 sqrt(n) overflows the cast from n = 2
        x = np.full(n, val, F32)
        got = run_sumsq(lib, x)
        assert np.isfinite(got) == np.isfinite(O.norm_f32(x)), (val, n, got)
        check_norm(got, x, (val, n))
    for bad in (NAN, float("inf")):
        x = rnd(n + 1, n)
        x[n // 2] = bad
        got = run_sumsq(lib, x)
        assert np.isnan(got) if np.isnan(bad) else got == np.inf, (bad, n, got)


def test_sumsq_refusals(lib):
    xb, out = Buf(rnd(1, 64)), dev_scalar(-7.0)
    refused(lib, lib.masr_test_sumsq(xb.ptr(1), 16, out.ptr(), S()), "16-byte")
    refused(lib, lib.masr_test_sumsq(xb.ptr(), 0, out.ptr(), S()), "n outside")
    refused(lib, lib.masr_test_sumsq(None, 16, out.ptr(), S()), "null")
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------- clip + SGD (clip_sgd_kernel)
LR, MOMENTUM = 0.05, 0.9


def norm_cases(g):
    """(name, the device norm or None, max_norm): coefficient exactly 1 twice, below 1, 0, NaN, no norm"""
    nv = float(O.norm_f32(g))
    return (("far_above", nv, 1e6 * (nv + 1.0)), ("zero_norm", 0.0, 5.0), ("clipped", nv, 0.37 * nv + 1e-3), ("max_norm_0", nv, 0.0),
            ("nan", NAN, 5.0), ("no_norm", None, 0.0))


def run_sgd(lib, n, off, norm_v, max_norm, momentum, nesterov, flags, mom_null=False, seed=0, check=True):
    p0, g0, m0 = rnd(seed + 1, n), rnd(seed + 2, n, 0.3), rnd(seed + 3, n, 0.2)
    p, g = Buf(p0, off), Buf(g0, off)
    mom = None if mom_null else Buf(m0, off)
    nb = dev_scalar(norm_v) if norm_v is not None else None
    _cabi.check(lib.masr_test_clip_sgd(p.ptr(), g.ptr(), PTR(mom), n, PTR(nb), max_norm, LR, momentum, nesterov, flags, S()), "clip_sgd")
    what = (n, off, norm_v, max_norm, momentum, nesterov, flags, mom_null)
    assert p.guard_ok() and g.untouched() and (mom is None or mom.guard_ok()) and (nb is None or nb.untouched()), what
    got_p, got_m = p.get(), (mom.get() if mom is not None else None)
    if not check:
        return got_p, got_m
    if norm_v is not None and np.isnan(norm_v):
        assert p.untouched() and (mom is None or mom.untouched()), ("a NaN norm skips the step", what)
        return got_p, got_m
    coef = O.clip_coef(F32(norm_v), max_norm) if norm_v is not None else F32(1.0)
    if norm_v is not None and max_norm > 0 and (norm_v == 0.0 or max_norm > 1e3 * norm_v):
        assert coef == 1.0
    r = O.sgd(p0, g0, m0, coef, O.f32v(LR), O.f32v(momentum), nesterov, flags)
    within(got_p, r["p"], r["p_bound"], "sgd p", what)
    if r["mom"] is None:
        assert mom is None or mom.untouched(), ("the buffer is written without momentum / on a last step", what)
    else:
        within(got_m, r["mom"], r["mom_bound"], "sgd mom", what)
    return got_p, got_m


@pytest.mark.parametrize("n,off", sizes_and_offsets())
def test_clip_sgd_flags_and_settings(lib, n, off):
    nv = float(O.norm_f32(rnd(2, n, 0.3)))
    combos = [(f, nes) for f in (0, 1, 2, 3) for nes in (0, 1)] if n != BIG else [(0, 1), (3, 0)]
    for flags, nes in combos:
        run_sgd(lib, n, off, nv, 0.37 * nv + 1e-3, MOMENTUM, nes, flags)
    run_sgd(lib, n, off, nv, 0.37 * nv + 1e-3, MOMENTUM, 1, 3, mom_null=True)
    run_sgd(lib, n, off, nv, 0.37 * nv + 1e-3, 0.0, 0, 0, mom_null=True)
    run_sgd(lib, n, off, nv, 0.37 * nv + 1e-3, 0.0, 1, 1)      # momentum 0 with a buffer: it stays as it is


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("n", (5, 4101))
def test_clip_sgd_norms(lib, n, off):
    g = rnd(2, n, 0.3)
    for name, nv, mx in norm_cases(g):
        for flags in (0, 1, 2):
            got_p, _ = run_sgd(lib, n, off, nv, mx, MOMENTUM, 1, flags)
            if name == "max_norm_0" and flags == 1:            # coefficient 0 on a first step: buf = 0, step = 0, p - lr 0 = p
                assert same_bits(got_p, rnd(1, n))


@pytest.mark.parametrize("n", (3, 10007, BIG))
def test_clip_sgd_last_step_and_forms(lib, n):
    nv = float(O.norm_f32(rnd(2, n, 0.3)))
    for nes in (0, 1):
        res = {(f, off): run_sgd(lib, n, off, nv, 0.37 * nv, MOMENTUM, nes, f, check=(n != BIG)) for f in (0, 1, 2, 3) for off in (0, 1)}
        for off in (0, 1):
            for f in (0, 1):
                assert same_bits(res[(f | 2, off)][0], res[(f, off)][0]), "p of a last step == p of the same step without the bit"
                assert same_bits(res[(f | 2, off)][1], rnd(3, n, 0.2)), "mom keeps its bits on a last step"
        for f in (0, 1, 2, 3):                                 # the scalar form == the 16-byte form (SgdUpd's explicit fused multiply-adds)
            assert same_bits(res[(f, 0)][0], res[(f, 1)][0]) and same_bits(res[(f, 0)][1], res[(f, 1)][1]), (n, nes, f)


def test_sgd_step_public(lib):
    """masr_sgd_step: the same kernel without a norm"""
    n = 4101
    p0, g0, m0 = rnd(1, n), rnd(2, n, 0.3), rnd(3, n, 0.2)
    p, g, mom = Buf(p0), Buf(g0), Buf(m0)
    _cabi.check(lib.masr_sgd_step(p.ptr(), g.ptr(), mom.ptr(), n, LR, MOMENTUM, 1, 0, S()), "sgd_step")
    torch.cuda.synchronize()
    r = O.sgd(p0, g0, m0, 1.0, O.f32v(LR), O.f32v(MOMENTUM), 1, 0)
    within(p.get(), r["p"], r["p_bound"], "sgd p", "public")
    within(mom.get(), r["mom"], r["mom_bound"], "sgd mom", "public")
    assert p.guard_ok() and mom.guard_ok() and g.untouched()


def test_clip_sgd_refusals(lib):
    n = 64
    p, g, nb = Buf(rnd(1, n)), Buf(rnd(2, n)), dev_scalar(1.0)
    refused(lib, lib.masr_test_clip_sgd(p.ptr(), g.ptr(), None, n, nb.ptr(), 5.0, LR, MOMENTUM, 1, 0, S()), "mom may be null only")
    refused(lib, lib.masr_test_clip_sgd(p.ptr(), g.ptr(), None, n, nb.ptr(), 5.0, LR, MOMENTUM, 1, 1, S()), "mom may be null only")
    refused(lib, lib.masr_test_clip_sgd(p.ptr(), g.ptr(), None, n, nb.ptr(), 5.0, LR, 0.0, 0, 4, S()), "step_flags")
    refused(lib, lib.masr_test_clip_sgd(p.ptr(), g.ptr(), None, 0, nb.ptr(), 5.0, LR, 0.0, 0, 0, S()), "n outside")
    refused(lib, lib.masr_test_clip_sgd(None, g.ptr(), None, n, nb.ptr(), 5.0, LR, 0.0, 0, 0, S()), "null")
    torch.cuda.synchronize()
    assert p.untouched() and g.untouched()


# ---------------------------------------------------------------- clip + scale, clip + accumulate, scale, axpy
@pytest.mark.parametrize("n,off", sizes_and_offsets())
def test_clip_scale_and_axpy(lib, n, off):
    g0, a0 = rnd(2, n, 0.3), rnd(4, n)
    cases = norm_cases(g0)[:5] if n != BIG else norm_cases(g0)[2:3]
    for name, nv, mx in cases:
        for nan_zero in (0, 1):
            what = (n, off, name, nan_zero)
            g, nb = Buf(g0, off), dev_scalar(nv)
            _cabi.check(lib.masr_test_clip_scale(g.ptr(), n, nb.ptr(), mx, nan_zero, S()), "clip_scale")
            assert g.guard_ok() and nb.untouched(), what
            coef = O.clip_coef(F32(nv), mx)
            if np.isnan(nv):
                assert (g.bits() == 0).all() if nan_zero else np.isnan(g.get()).all(), what
            else:
                assert same_bits(g.get(), O.scale_bits(g0, coef)), what      # one rounding of exact inputs: the bits
            acc, g = Buf(a0, off), Buf(g0, off)
            _cabi.check(lib.masr_test_clip_axpy(acc.ptr(), g.ptr(), n, nb.ptr(), mx, nan_zero, S()), "clip_axpy")
            assert acc.guard_ok() and g.untouched() and nb.untouched(), what
            if np.isnan(nv):
                assert acc.untouched() if nan_zero else np.isnan(acc.get()).all(), what
            else:
                ref, bound = O.axpy(a0, g0, coef)
                within(acc.get(), ref, bound, "axpy", what)


@pytest.mark.parametrize("chunks", (2, 3, 16))
def test_clip_scale_in_chunks(lib, chunks):
    """one call over the buffer == calls over ragged chunks at odd offsets (how the all-reduce path scales a buffer), bit for bit"""
    n = 10007
    g0 = rnd(2, n, 0.3)
    nv = float(O.norm_f32(g0))
    nb, whole, parts = dev_scalar(nv), Buf(g0), Buf(g0)
    _cabi.check(lib.masr_test_clip_scale(whole.ptr(), n, nb.ptr(), 0.37 * nv, 0, S()), "clip_scale")
    cuts = sorted({0, n} | {(n * k // chunks) | 1 for k in range(1, chunks)})      # odd interior boundaries, ragged lengths
    assert len(cuts) == chunks + 1
    for a, b in zip(cuts[:-1], cuts[1:]):
        _cabi.check(lib.masr_test_clip_scale(parts.ptr(a), b - a, nb.ptr(), 0.37 * nv, 0, S()), "clip_scale chunk")
    assert parts.guard_ok() and same_bits(whole.get(), parts.get())
    _cabi.check(lib.masr_clip_scale_flat(parts.ptr(), n, nb.ptr(), 1e9, S()), "clip_scale_flat")       # the public form, coefficient 1
    torch.cuda.synchronize()
    assert same_bits(whole.get(), parts.get())


@pytest.mark.parametrize("n,off", sizes_and_offsets())
def test_scale_and_axpy_public(lib, n, off):
    x0, y0 = rnd(5, n), rnd(6, n)
    for a in (0.0, 1.0 / 3.0, -1.0):
        x = Buf(x0, off)
        _cabi.check(lib.masr_scale(x.ptr(), n, a, S()), "scale")
        y, xr = Buf(y0, off), Buf(x0, off)
        _cabi.check(lib.masr_axpy(y.ptr(), xr.ptr(), n, a, S()), "axpy")
        torch.cuda.synchronize()
        assert x.guard_ok() and y.guard_ok() and xr.untouched()
        assert same_bits(x.get(), O.scale_bits(x0, F32(a))), (n, off, a)
        ref, bound = O.axpy(y0, x0, F32(a))
        within(y.get(), ref, bound, "axpy", (n, off, a))


def test_clip_scale_axpy_refusals(lib):
    n = 64
    a, g, nb = Buf(rnd(1, n)), Buf(rnd(2, n)), dev_scalar(1.0)
    refused(lib, lib.masr_test_clip_scale(g.ptr(), n, None, 5.0, 0, S()), "null")
    refused(lib, lib.masr_test_clip_scale(g.ptr(), 0, nb.ptr(), 5.0, 0, S()), "n outside")
    refused(lib, lib.masr_test_clip_axpy(a.ptr(), g.ptr(), n, None, 5.0, 0, S()), "null")
    refused(lib, lib.masr_test_clip_axpy(a.ptr(), None, n, nb.ptr(), 5.0, 0, S()), "null")
    refused(lib, lib.masr_test_clip_axpy(a.ptr(), g.ptr(), -1, nb.ptr(), 5.0, 0, S()), "n outside")
    torch.cuda.synchronize()
    assert a.untouched() and g.untouched()


# ---------------------------------------------------------------- Adam / AdamW / Adam with L2 (adam_kernel)
B1, B2, EPS, WD = 0.9, 0.98, 1e-8, 0.125                      # (wd a power of two: lr wd is exact, whatever the host contracts)


def adam_state(n, seed=0):
    v = rnd(seed + 14, n, 0.1) ** 2
    return rnd(seed + 11, n), rnd(seed + 12, n, 0.1), rnd(seed + 13, n, 0.1), v.astype(F32)


def check_adam(bufs, r, what, cls="adam"):
    p, m, v = bufs
    within(p.get(), r["p"], r["p_bound"], cls + " p", what)
    within(m.get(), r["m"], r["m_bound"], cls + " m", what)
    within(v.get(), r["v"], r["v_bound"], cls + " v", what)
    assert p.guard_ok() and m.guard_ok() and v.guard_ok(), what


@pytest.mark.parametrize("n,off", sizes_and_offsets())
def test_adam_family(lib, n, off):
    p0, g0, m0, v0 = adam_state(n)
    kinds = (("adam", 0.0, 0), ("l2", WD, 0), ("adamw", WD, 1)) if n != BIG else (("adamw", WD, 1),)
    for kind, wd, dec in kinds:
        for t in (1, 7):
            p, g, m, v = Buf(p0, off), Buf(g0, off), Buf(m0, off), Buf(v0, off)
            if kind == "adam":
                _cabi.check(lib.masr_adam_step(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, B1, B2, EPS, t, S()), "adam")
            else:
                _cabi.check(lib.masr_adamw_step(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, B1, B2, EPS, wd, dec, t, S()), "adamw")
            torch.cuda.synchronize()
            assert g.untouched()
            check_adam((p, m, v), O.adam(p0, g0, m0, v0, O.adam_scalars(1e-3, B1, B2, t, wd, dec), O.f32v(EPS)), (kind, n, off, t))


# ---------------------------------------------------------------- the guarded Adam (adam_guarded_kernel)
A_SC, B_SC = (1e-3, 9), (4e-3, 2)                              # far apart: the wrong candidate moves every element by ~ 3 lr, the bound is ~ 1e-7 lr
SEQ_NORMS = (1.0, NAN, 1.0, 1.0, NAN, NAN, 1.0)


def call_guarded(lib, bufs, g, n, a, b, wd, dec, nb, fl, slot):
    p, m, v = bufs
    _cabi.check(lib.masr_test_adam_guarded(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, a[0], a[1], b[0], b[1], B1, B2, EPS, wd, dec, nb.ptr(),
                                           fl.ptr(), slot, S()), "adam_guarded")


@pytest.mark.parametrize("n,off,dec,flags0", [(n, off, dec, fl) for n in (5, 4101) for off in (0, 1) for dec in (0, 1) for fl in ((0, 0), (0, 7))]
                         + [(BIG, 0, 1, (0, 0)), (BIG, 1, 0, (0, 7))])
def test_adam_guarded_sequence(lib, n, off, dec, flags0):
    p0, _, m0, v0 = adam_state(n)
    bufs = (Buf(p0, off), Buf(m0, off), Buf(v0, off))
    fl = Buf(np.array(flags0, np.int32))
    flags = list(flags0)
    norms = SEQ_NORMS if n != BIG else SEQ_NORMS[:3]
    for i, nv in enumerate(norms):
        slot = i & 1
        a, b = (A_SC[0], A_SC[1] + i), (B_SC[0], B_SC[1] + i)
        g0 = rnd(50 + i, n, 0.1)
        g, nb = Buf(g0, off), dev_scalar(nv)
        before = [x.get() for x in bufs]
        call_guarded(lib, bufs, g, n, a, b, WD, dec, nb, fl, slot)
        skip, cand, flags = O.guarded(flags, slot, nv)
        what = (n, off, dec, flags0, "launch", i, "candidate", cand)
        assert g.untouched() and nb.untouched() and fl.guard_ok(), what
        assert fl.get().tolist() == flags, (what, fl.get().tolist())          # own verdict in flags[slot]; flags[slot ^ 1] as it was
        if skip:
            assert all(same_bits(x.get(), y) for x, y in zip(bufs, before)) and all(x.guard_ok() for x in bufs), ("skipped launch wrote", what)
            continue
        lr, t = b if cand == "B" else a
        check_adam(bufs, O.adam(before[0], g0, before[1], before[2], O.adam_scalars(lr, B1, B2, t, WD, dec), O.f32v(EPS)), what, "guarded")


@pytest.mark.parametrize("dec", (0, 1))
@pytest.mark.parametrize("n,off", [(3, 0), (10007, 0), (10007, 1)])
def test_adam_guarded_equals_adamw_step(lib, n, off, dec):
    """A == B and a finite norm: the same statement as adam_kernel with the same scalars -> the bits of masr_adamw_step"""
    p0, g0, m0, v0 = adam_state(n)
    g, nb, fl = Buf(g0, off), dev_scalar(2.5), Buf(np.array([0, 1], np.int32))
    x = (Buf(p0, off), Buf(m0, off), Buf(v0, off))
    y = (Buf(p0, off), Buf(m0, off), Buf(v0, off))
    call_guarded(lib, x, g, n, (2e-3, 4), (2e-3, 4), WD, dec, nb, fl, 0)
    _cabi.check(lib.masr_adamw_step(y[0].ptr(), g.ptr(), y[1].ptr(), y[2].ptr(), n, 2e-3, B1, B2, EPS, WD, dec, 4, S()), "adamw")
    torch.cuda.synchronize()
    assert all(same_bits(a.get(), b.get()) for a, b in zip(x, y)), (n, off, dec)
    assert fl.get().tolist() == [0, 1]


def test_adam_guarded_refusals(lib):
    n = 64
    p0, g0, m0, v0 = adam_state(n)
    p, g, m, v, nb, fl = Buf(p0), Buf(g0), Buf(m0), Buf(v0), dev_scalar(1.0), Buf(np.array([0, 0], np.int32))
    f = lib.masr_test_adam_guarded
    refused(lib, f(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, 1, 1e-3, 1, B1, B2, EPS, 0.0, 0, nb.ptr(), fl.ptr(), 2, S()), "slot")
    refused(lib, f(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, 0, 1e-3, 1, B1, B2, EPS, 0.0, 0, nb.ptr(), fl.ptr(), 0, S()), "step numbers")
    refused(lib, f(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, 1, 1e-3, 1, B1, B2, EPS, 0.0, 0, None, fl.ptr(), 0, S()), "null")
    refused(lib, f(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, 1e-3, 1, 1e-3, 1, B1, B2, EPS, 0.0, 0, nb.ptr(), None, 0, S()), "null")
    refused(lib, f(p.ptr(), g.ptr(), m.ptr(), v.ptr(), 0, 1e-3, 1, 1e-3, 1, B1, B2, EPS, 0.0, 0, nb.ptr(), fl.ptr(), 0, S()), "n outside")
    torch.cuda.synchronize()
    assert all(x.untouched() for x in (p, g, m, v, fl))


# ---------------------------------------------------------------- the summed-gradient Adam and the list sum (adam_sum_kernel, sum_n_kernel)
def ptr_list(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr().value for b in bufs])


def run_sum_cases(lib, n, n_grads, gscale, mis=None, bits=True):
    """masr_adam_sum_step and masr_sum_n on n_grads buffers (member `mis` one float past a 16-byte boundary: the launch takes the scalar form)
    against the fp64 reference and, with everything aligned, against the passes they replaced: zero, n axpy, scale, then Adam / a copy"""
    what = (n, n_grads, gscale, mis)
    p0, _, m0, v0 = adam_state(n)
    gs0 = [rnd(70 + k, n, 0.1) for k in range(n_grads)]
    gs = [Buf(x, 1 if k == mis else 0) for k, x in enumerate(gs0)]
    p, m, v, out = Buf(p0), Buf(m0), Buf(v0), Buf(rnd(5, n))
    _cabi.check(lib.masr_adam_sum_step(p.ptr(), ptr_list(gs), n_grads, gscale, m.ptr(), v.ptr(), n, 1e-3, B1, B2, EPS, 3, S()), "adam_sum")
    _cabi.check(lib.masr_sum_n(out.ptr(), ptr_list(gs), n_grads, gscale, n, S()), "sum_n")
    torch.cuda.synchronize()
    assert all(x.untouched() for x in gs) and out.guard_ok(), what
    check_adam((p, m, v), O.adam_sum(p0, gs0, F32(gscale), m0, v0, O.adam_scalars(1e-3, B1, B2, 3), O.f32v(EPS)), what, "adam_sum")
    ref, bound = O.sum_list(gs0, F32(gscale))
    within(out.get(), ref, bound, "sum_n", what)
    if n_grads == 2 and gscale == 1.0:
        assert same_bits(out.get(), gs0[0] + gs0[1]), ("one rounding of exact inputs", what)
    if not bits or mis is not None:
        return
    acc = Buf(rnd(6, n))                                       # a finite buffer: times 0 it is (signed) zero
    _cabi.check(lib.masr_scale(acc.ptr(), n, 0.0, S()), "scale 0")
    for x in gs:
        _cabi.check(lib.masr_axpy(acc.ptr(), x.ptr(), n, 1.0, S()), "axpy")
    _cabi.check(lib.masr_scale(acc.ptr(), n, gscale, S()), "scale")
    p2, m2, v2 = Buf(p0), Buf(m0), Buf(v0)
    _cabi.check(lib.masr_adam_step(p2.ptr(), acc.ptr(), m2.ptr(), v2.ptr(), n, 1e-3, B1, B2, EPS, 3, S()), "adam")
    torch.cuda.synchronize()
    # (-0 + g and +0 + g are g whatever the sign of the zero -- unless g is a zero itself: compare values where both are zero)
    a, b = out.get(), acc.get()
    assert np.array_equal(a, b) and same_bits(np.where(a == 0, F32(0), a), np.where(b == 0, F32(0), b)), ("sum_n != zero + axpy + scale", what)
    for name, x, y in (("p", p, p2), ("m", m, m2), ("v", v, v2)):
        nd = int((x.bits() != y.bits()).sum())
        assert nd == 0, ("adam_sum != zero + axpy + scale + adam", name, what, "elements that differ", nd, "of", n)


@pytest.mark.parametrize("n_grads", (1, 2, 3, 8))
@pytest.mark.parametrize("n", FLAT_NS)
def test_adam_sum_and_sum_n(lib, n, n_grads):
    for gscale in (1.0, 1.0 / 3.0, -1.0):
        run_sum_cases(lib, n, n_grads, gscale)
    run_sum_cases(lib, n, n_grads, 1.0 / 3.0, mis=n_grads - 1)
    if n_grads > 1:
        run_sum_cases(lib, n, n_grads, 1.0 / 3.0, mis=0)


@pytest.mark.parametrize("mis", (None, 1))
def test_adam_sum_and_sum_n_past_a_grid_stride(lib, mis):
    run_sum_cases(lib, BIG, 3, 1.0 / 3.0, mis=mis)


def test_adam_sum_and_sum_n_refusals(lib):
    n = 64
    p0, g0, m0, v0 = adam_state(n)
    p, m, v, out = Buf(p0), Buf(m0), Buf(v0), Buf(rnd(5, n))
    gs = [Buf(g0) for _ in range(9)]
    for k in (0, 9):
        refused(lib, lib.masr_adam_sum_step(p.ptr(), ptr_list(gs), k, 1.0, m.ptr(), v.ptr(), n, 1e-3, B1, B2, EPS, 1, S()), "1 to 8")
        refused(lib, lib.masr_sum_n(out.ptr(), ptr_list(gs), k, 1.0, n, S()), "1 to 8")
    torch.cuda.synchronize()
    assert all(x.untouched() for x in (p, m, v, out))
