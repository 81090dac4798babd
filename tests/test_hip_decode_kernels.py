"""The decode-step kernels one by one (include/masr_test.h) against plain high-precision restatements: the skinny GEMM of every decoder
Linear, the one-query attention against the KV cache and the encoder memory, the fp32 last projection, the greedy arg-max and the beam
step's row top-K + K-way select.  Operands are rounded to bf16 (or fp32) first and the references are fp64 on exactly those values, so
the tolerances are fp32 accumulation bounds.  Every region a launch must not touch is filled with NaN or a sentinel and compared bit for
bit afterwards."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


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


def randn16(shape, g, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).bfloat16()


# ---------------------------------------------------------------- skinny GEMM (decode.hip skinny_gemm_kernel)
EPIS = ("none", "bias", "bias_relu", "bias_res")
OUTS = ("c32", "c16", "both")


def run_skinny(L, M, N, K, epi, out, seed, neg_res=False, relu_res=False):
    g = gen(seed)
    lda, ldw = K + 8, K + 24
    A = torch.full((M, lda), NAN, device=DEV, dtype=torch.bfloat16)      # the pad columns must never be read
    W = torch.full((N, ldw), NAN, device=DEV, dtype=torch.bfloat16)
    A[:, :K] = randn16((M, K), g)
    W[:, :K] = randn16((N, K), g)
    bias = torch.randn(N, device=DEV, generator=g) if epi != "none" else None
    relu = 1 if epi == "bias_relu" or relu_res else 0
    res = None
    if epi == "bias_res" or relu_res:
        res = torch.randn(M, N, device=DEV, generator=g)
        if neg_res:
            res = -res.abs() - 0.5
    # outputs: [M][N] (the launch's ldc is N) plus a NaN tail that stands for rows >= M
    c32 = torch.full((M + 2, N), NAN, device=DEV) if out in ("c32", "both") else None
    c16 = torch.full((M + 2, N), NAN, device=DEV, dtype=torch.bfloat16) if out in ("c16", "both") else None
    c32_0 = c32.clone() if c32 is not None else None
    c16_0 = c16.clone() if c16 is not None else None
    _cabi.check(L.masr_test_skinny_gemm(P(A), lda, P(W), ldw, M, N, K, P(bias), relu, P(res), P(c32), P(c16), S()), "skinny")
    torch.cuda.synchronize()
    a64, w64 = A[:, :K].double(), W[:, :K].double()
    ref = a64 @ w64.t()
    scale = a64.abs() @ w64.abs().t()                     # sum_k |a_mk w_nk|
    if bias is not None:
        ref = ref + bias.double()
        scale = scale + bias.double().abs()
    if relu:
        ref = ref.clamp_min(0.0)
    if res is not None:
        ref = ref + res.double()                           # documented order: bias, then ReLU, then residual
        scale = scale + res.double().abs()
    what = (M, N, K, epi, out, neg_res)
    if c32 is not None:
        assert same_bits(c32[M:], c32_0[M:]), ("C32 rows >= M written", what)
        got = c32[:M].double()
        assert torch.isfinite(got).all(), what
        # fp32 accumulation: (K/128 MFMA steps + 4-wave combine + epilogue adds) roundings of 2^-24 each, relative to the sum of |terms|;
        # a missing or doubled 8-wide k-chunk is ~8/K of that sum.  (The bias / residual magnitudes enter for their own additions.)
        err = (got - ref).abs()
        bad = err > 1e-6 * scale
        assert not bad.any(), ("C32", what, float(err.max()), int(bad.sum()))
    if c16 is not None:
        assert same_bits(c16[M:], c16_0[M:]), ("C16 rows >= M written", what)
        if c32 is not None:
            assert same_bits(c16[:M], c32[:M].bfloat16()), ("C16 != bf16(C32)", what)
        r16 = ref.float().bfloat16().double()
        got = c16[:M].double()
        mag = torch.maximum(got.abs(), r16.abs())
        ulp = torch.ldexp(torch.ones_like(mag), torch.frexp(mag.clamp_min(1e-30)).exponent - 8)
        # one bf16 ulp, plus the fp32 bound above carried through the rounding: where the sum cancels to near 0, the fp32 error alone
        # exceeds an ulp of the tiny result
        assert ((got - r16).abs() <= ulp + 1e-6 * scale).all(), ("C16 more than 1 bf16 ulp from bf16(ref)", what)


def _skinny_cases():
    Ms = (1, 5, 16, 17, 64, 80, 320, 1024)                # greedy B, B*K for K = 4, 5, 20, 64
    Ns = (1, 12, 64, 367, 512, 1536, 2048)
    Ks = (32, 64, 96, 128, 160, 384, 416, 512, 544, 1024, 2048)   # idle waves, the 1-step tail, the 4-deep loop at its boundary
    cases = []
    for i, K in enumerate(Ks):
        cases.append((Ms[i % len(Ms)], Ns[(3 * i + 1) % len(Ns)], K))
    for i, M in enumerate(Ms):
        cases.append((M, Ns[(i + 2) % len(Ns)], Ks[(5 * i + 3) % len(Ks)]))
    for i, N in enumerate(Ns):
        cases.append((Ms[(3 * i + 1) % len(Ms)], N, Ks[(2 * i + 7) % len(Ks)]))
    return cases


def test_skinny_gemm_shapes(L):
    for i, (M, N, K) in enumerate(_skinny_cases()):
        run_skinny(L, M, N, K, EPIS[i % 4], OUTS[(i // 4 + i) % 3], seed=100 + i)


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("out", OUTS)
def test_skinny_gemm_epilogues(L, epi, out):
    for i, (M, N, K) in enumerate(((17, 367, 416), (80, 64, 544), (5, 12, 32))):
        run_skinny(L, M, N, K, epi, out, seed=1000 + 17 * EPIS.index(epi) + 5 * OUTS.index(out) + i)


def test_skinny_gemm_relu_then_residual(L):
    """ReLU with a negative residual: the result may be negative only if the residual comes after the ReLU"""
    for i, (M, N, K) in enumerate(((5, 12, 160), (80, 64, 544), (1, 367, 2048))):
        for out in OUTS:
            run_skinny(L, M, N, K, "bias_res", out, seed=2000 + i, neg_res=True, relu_res=True)


def test_skinny_gemm_errors(L):
    g = gen(3)
    A = randn16((16, 64 + 8), g)
    W = randn16((16, 64 + 8), g)
    c32 = torch.full((16, 16), 7.0, device=DEV)
    c0 = c32.clone()
    st = S()
    assert L.masr_test_skinny_gemm(P(A), 72, P(W), 72, 16, 16, 48, None, 0, None, P(c32), None, st) != 0        # K % 32
    assert L.masr_test_skinny_gemm(P(A), 68, P(W), 72, 16, 16, 64, None, 0, None, P(c32), None, st) != 0        # lda % 8
    assert L.masr_test_skinny_gemm(P(A, 8), 72, P(W), 72, 15, 16, 64, None, 0, None, P(c32), None, st) != 0     # A not 16-B aligned
    assert L.masr_last_error()
    torch.cuda.synchronize()
    assert same_bits(c32, c0)


# ---------------------------------------------------------------- decode attention (decode.hip attn_decode_kernel)
# The kernel starts its running maximum at -3.0e38 rather than -inf.  With bf16 operands no finite scaled score gets below it: a finite
# fp32 dot product is at most FLT_MAX in magnitude and is then multiplied by 1/sqrt(hd) <= 1/4 (hd >= 16), so |score| <= 8.6e37; a dot
# product that overflows is +-inf, which no finite start value would change.  That start is therefore left as it is.

def _tol_check(o, ref, vmax, what):
    """|o - ref| <= 2^-8 |ref| + 2^-12 max|v| (bf16 output rounding plus fp32 soft-max / P.V accumulation)"""
    o = o.double()
    assert torch.isfinite(o).all(), what
    err = (o - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -12 * vmax
    assert (err <= bound).all(), (what, float(err.max()), float((err - bound).max()))


def attn_ref(q, keys, vals, hd):
    """q [R][H][hd], keys / vals [R][n][H][hd] (fp64) -> softmax(q k^T / sqrt(hd)) v [R][H][hd] and max|v| per (row, head)"""
    s = torch.einsum("rhd,rnhd->rhn", q, keys) / math.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("rhn,rnhd->rhd", p, vals), vals.abs().amax(dim=(1, 3))[..., None]


def run_self_attn(L, R, H, hd, step, seed, utt_rows=0, huge=False):
    """greedy (utt_rows = 0) or beam (utt_rows = K: R rows in utterances of K, keys gathered through a [2][R][Lmax] slot table) self-
    attention at `step` in the engine's layout: q / knew / vnew at columns 0 / E / 2E of a [R][3E] row, the cache [R][slots][3E]"""
    g = gen(seed)
    E = H * hd
    slots = step + 3
    cache = torch.full((R, slots, 3 * E), NAN, device=DEV, dtype=torch.bfloat16)
    cache[:, :step - 1, E:] = randn16((R, step - 1, 2 * E), g)
    row = randn16((R, 3 * E), g)
    if huge:
        # |scores| ~ 3e4, keys 400+ apart: the soft-max is one-hot to fp64 precision
        u = torch.where(torch.rand(H, hd, device=DEV, generator=g) < 0.5, -1.0, 1.0)
        sv = (torch.randperm(148, device=DEV, generator=g)[:step].double() * 0.5 - 37.0).view(1, step, 1, 1)
        keys = (sv * u).expand(R, step, H, hd)
        cache[:, :step - 1, E:2 * E] = keys[:, :step - 1].reshape(R, step - 1, E).bfloat16()
        row[:, E:2 * E] = keys[:, step - 1].reshape(R, E).bfloat16()
        row[:, :E] = (100.0 * u).reshape(1, E).expand(R, E).bfloat16()
    src = None
    if utt_rows:
        K = utt_rows
        base = (torch.arange(R, device=DEV) // K * K).view(1, R, 1)
        src = (base + torch.randint(0, K, (2, R, slots), device=DEV, generator=g)).int()   # both parities: valid, different rows
        src[step & 1, torch.arange(R), step - 1] = torch.arange(R, device=DEV, dtype=torch.int32)
    step_d = torch.tensor([step, 0], device=DEV, dtype=torch.int32)
    o = torch.full((R, E + 8), NAN, device=DEV, dtype=torch.bfloat16)
    c0, o0 = cache.clone(), o.clone()
    _cabi.check(L.masr_test_attn_decode(P(row), 3 * E, P(cache, 2 * E), P(cache, 4 * E), 3 * E, slots * 3 * E, P(row, 2 * E),
                                        P(row, 4 * E), 3 * E, P(step_d), None, P(o), E + 8, R, H, hd, slots, 0, P(src),
                                        slots if src is not None else 0, R * slots if src is not None else 0, S()), "attn_decode")
    torch.cuda.synchronize()
    what = (R, H, hd, step, utt_rows, huge)
    want = c0.clone()
    want[:, step - 1, E:] = row[:, E:]                      # the append goes to each row's own slot step-1, nothing else changes
    assert same_bits(cache, want), ("cache", what)
    assert same_bits(o[:, E:], o0[:, E:]), ("o pad columns written", what)
    j = torch.arange(step - 1, device=DEV).view(1, -1)
    idx = src[step & 1, :, :step - 1].long() if src is not None else torch.arange(R, device=DEV).view(-1, 1).expand(R, step - 1)
    old = c0[idx, j].double()                               # [R][step-1][3E]: key j of row r from cache row src[r][j]
    keys = torch.cat([old[..., E:2 * E], row[:, None, E:2 * E].double()], dim=1).view(R, step, H, hd)
    vals = torch.cat([old[..., 2 * E:], row[:, None, 2 * E:].double()], dim=1).view(R, step, H, hd)
    ref, vmax = attn_ref(row[:, :E].double().view(R, H, hd), keys, vals, hd)
    _tol_check(o[:, :E].view(R, H, hd), ref, vmax, what)


@pytest.mark.parametrize("hd", (16, 32, 64))
def test_attn_decode_greedy_self(L, hd):
    for i, step in enumerate((1, 2, 37, 255, 256, 257, 1000, 3000)):
        run_self_attn(L, 3, 4 if i % 2 else 8, hd, step, seed=10 * hd + i)


@pytest.mark.parametrize("hd", (16, 32, 64))
def test_attn_decode_beam_self(L, hd):
    """keys read through the slot table at both step parities (the other parity holds different valid rows)"""
    for i, (K, step) in enumerate(((4, 36), (4, 37), (5, 300), (5, 301), (20, 2), (1, 3))):
        run_self_attn(L, 2 * K, 8 if i % 2 else 4, hd, step, seed=500 + 10 * hd + i, utt_rows=K)


def run_cross_attn(L, klens, H, hd, rpu, seed, Tk_cap=None, huge=False):
    g = gen(seed)
    E = H * hd
    U = len(klens)
    B = U * rpu if rpu > 1 else U
    Tp = Tk_cap or max(klens) + 3
    ldk = 2 * E + 8
    mem = torch.full((U, Tp, ldk), NAN, device=DEV, dtype=torch.bfloat16)    # keys / values past each klen: NaN, never read
    for u, n in enumerate(klens):
        mem[u, :n, :2 * E] = randn16((n, 2 * E), g)
    q = torch.full((B, E + 8), NAN, device=DEV, dtype=torch.bfloat16)
    q[:, :E] = randn16((B, E), g)
    if huge:
        u_ = torch.where(torch.rand(H, hd, device=DEV, generator=g) < 0.5, -1.0, 1.0)
        for u, n in enumerate(klens):
            sv = (torch.randperm(148, device=DEV, generator=g)[:n].double() * 0.5 - 37.0).view(n, 1, 1)
            mem[u, :n, :E] = (sv * u_).reshape(n, E).bfloat16()
        q[:, :E] = (100.0 * u_).reshape(1, E).expand(B, E).bfloat16()
    kl = torch.tensor(klens, device=DEV, dtype=torch.int32)
    o = torch.full((B, E + 8), NAN, device=DEV, dtype=torch.bfloat16)
    m0, o0 = mem.clone(), o.clone()
    _cabi.check(L.masr_test_attn_decode(P(q), E + 8, P(mem), P(mem, 2 * E), ldk, Tp * ldk, None, None, 0, None, P(kl), P(o), E + 8,
                                        B, H, hd, Tp, rpu, None, 0, 0, S()), "attn_decode")
    torch.cuda.synchronize()
    what = (klens, H, hd, rpu, huge)
    assert same_bits(mem, m0), ("memory written", what)
    assert same_bits(o[:, E:], o0[:, E:]), ("o pad columns written", what)
    for b in range(B):
        u = b // rpu if rpu > 1 else b
        n = klens[u]
        kv = mem[u, :n].double()
        ref, vmax = attn_ref(q[b:b + 1, :E].double().view(1, H, hd), kv[None, :, :E].reshape(1, n, H, hd),
                             kv[None, :, E:2 * E].reshape(1, n, H, hd), hd)
        _tol_check(o[b:b + 1, :E].view(1, H, hd), ref, vmax, what + (b,))


@pytest.mark.parametrize("hd", (16, 32, 64))
def test_attn_decode_cross(L, hd):
    """ragged key counts, NaN past each; rows_per_utt 4 and 20: row b reads utterance b / K"""
    for i, rpu in enumerate((1, 4, 20)):
        run_cross_attn(L, [1, 17, 256, 257, 700], 4 if (i + hd) % 2 else 8, hd, rpu, seed=700 + 10 * hd + i)


@pytest.mark.parametrize("hd", (16, 64))
def test_attn_decode_huge_scores(L, hd):
    """|scores| ~ 3e4 (the diverging-run case of test_attention_huge_scores): the one-hot result, no NaN"""
    run_cross_attn(L, [1, 40, 148], 4, hd, 1, seed=900 + hd, huge=True)
    run_self_attn(L, 3, 4, hd, 100, seed=950 + hd, huge=True)
    run_self_attn(L, 8, 4, hd, 77, seed=960 + hd, utt_rows=4, huge=True)


def test_attn_decode_lds_limit(L):
    """klen = Tk_cap = 15360 keys: the most the 60 KiB score row holds"""
    run_cross_attn(L, [15360], 4, 64, 1, seed=11, Tk_cap=15360)


def test_attn_decode_errors(L):
    """rejected before anything is launched: o keeps its sentinel"""
    H, hd = 4, 16
    E = H * hd
    g = gen(12)
    q = randn16((2, E + 8), g)
    mem = randn16((2, 32, 2 * E), g)
    o = torch.full((2, E), NAN, device=DEV, dtype=torch.bfloat16)
    o0 = o.clone()
    st = S()

    def call(klens, Tk_cap, hd_=hd, ldq=E, src=None, step=None):
        kl = torch.tensor(klens, device=DEV, dtype=torch.int32)
        row = torch.cat([q[:, :E], mem[:, 0]], dim=1).contiguous() if step is not None else None
        if step is not None:                                # self-attention form: q / knew / vnew in one [2][3E] row
            return L.masr_test_attn_decode(P(row), 3 * E, P(mem), P(mem, 2 * E), 2 * E, 32 * 2 * E, P(row, 2 * E), P(row, 4 * E), 3 * E,
                                           P(kl), None, P(o), E, 2, H, hd_, Tk_cap, 0, P(src), 32 if src is not None else 0,
                                           64 if src is not None else 0, st)
        return L.masr_test_attn_decode(P(q), ldq, P(mem), P(mem, 2 * E), 2 * E, 32 * 2 * E, None, None, 0, None, P(kl), P(o), E,
                                       2, H, hd_, Tk_cap, 0, None, 0, 0, st)

    assert call([10, 10], 32) == 0                            # (the valid form of the calls below)
    torch.cuda.synchronize()
    o.fill_(NAN)
    assert call([10, 10], 15361) != 0                         # more keys than the LDS score row holds
    assert call([10, 10], 32, hd_=48) != 0                    # head dim not 16/32/64
    assert call([10, 10], 32, ldq=E + 4) != 0                 # ldq % 8 != 0
    assert call([10, 33], 32) != 0                            # key count above Tk_cap
    assert call([0, 10], 32) != 0                             # no key
    bad = torch.zeros(2, 2, 32, device=DEV, dtype=torch.int32)
    bad[1, 1, 3] = 2                                          # step 5 reads parity 1; row 2 is not a cache row
    assert call([5], 32, step=True, src=bad) != 0
    assert L.masr_last_error()
    torch.cuda.synchronize()
    assert same_bits(o, o0)


# ---------------------------------------------------------------- fp32 logits (decode.hip logits_f32_kernel)
def run_logits(L, rows, Cn, E, seed):
    g = gen(seed)
    ld = Cn + 3
    # one flat buffer each, used at offset 0 (16-byte rows -> <true>) and at offset 1 float (4-byte loads -> <false>)
    yb = torch.empty(rows * E + 4, device=DEV)
    wb = torch.empty(Cn * E + 4, device=DEV)
    y = torch.randn(rows, E, device=DEV, generator=g)
    w = torch.randn(Cn, E, device=DEV, generator=g)
    bias = torch.randn(Cn, device=DEV, generator=g)
    zs = []
    for off in (0, 1):
        yb.fill_(NAN); wb.fill_(NAN)
        yb[off:off + rows * E] = y.flatten()
        wb[off:off + Cn * E] = w.flatten()
        z = torch.full((rows, ld), NAN, device=DEV)
        _cabi.check(L.masr_test_logits_f32(P(yb, 4 * off), P(wb, 4 * off), P(bias), P(z), ld, rows, Cn, E, S()), "logits_f32")
        zs.append(z)
    torch.cuda.synchronize()
    what = (rows, Cn, E)
    for z in zs:
        assert torch.isnan(z[:, Cn:]).all(), ("pad columns written", what)
    # the same products in the same order: the 16-byte and 4-byte forms agree bit for bit
    assert same_bits(zs[0], zs[1]), ("aligned and unaligned runs differ", what)
    ref = y.double() @ w.double().t() + bias.double()
    # per lane E/256 fmas, a 64-lane tree, the bias: at most E/256 + 7 roundings of 2^-24 relative to sum |y w| + |bias|  (<= 2^-20 at E <= 2304)
    scale = y.double().abs() @ w.double().abs().t() + bias.double().abs()
    err = (zs[0][:, :Cn].double() - ref).abs()
    assert (err <= 2.0 ** -20 * scale).all(), (what, float(err.max()))


def test_logits_f32_shapes(L):
    Cs = (1, 12, 63, 64, 65, 367, 5000)
    Es = (64, 256, 260, 512, 1024)
    Rs = (1, 4, 80, 320)
    i = 0
    for Cn in Cs:
        for E in Es:
            run_logits(L, Rs[i % len(Rs)], Cn, E, seed=3000 + i)
            i += 1
    for rows in Rs:
        run_logits(L, rows, 367, 260, seed=3100 + rows)


def test_logits_f32_errors(L):
    y = torch.randn(4, 64, device=DEV)
    w = torch.randn(12, 64, device=DEV)
    b = torch.randn(12, device=DEV)
    z = torch.full((4, 12), 7.0, device=DEV)
    assert L.masr_test_logits_f32(P(y), P(w), P(b), P(z), 12, 4, 12, 62, S()) != 0       # E % 4 != 0
    assert L.masr_test_logits_f32(P(y), P(w), P(b), P(z), 12, 0, 12, 64, S()) != 0       # rows = 0
    torch.cuda.synchronize()
    assert (z == 7.0).all()


# ---------------------------------------------------------------- greedy arg-max (decode.hip recog_argmax_step_kernel)
FMAX = float(np.finfo(F32).max)


def argmax_ref(row):
    """first maximal index; a NaN never wins, and a row with nothing above -inf gives 0.  (torch.argmax would return the index of the
    first NaN of a row that holds one: the kernel's comparisons are all false for NaN, so it skips them)"""
    v = np.where(np.isnan(row), -np.inf, row)
    m = v.max()
    return 0 if m == -np.inf else int(np.flatnonzero(v == m)[0])


def _argmax_rows(B, Cn, rng):
    z = rng.standard_normal((B, Cn)).astype(F32)
    for b in range(B):
        kind = b % 12
        r = z[b]
        if kind == 1 and Cn > 256:                          # equal maxima in the same lane (c, c + 256)
            c = int(rng.integers(0, Cn - 256)); r[c] = r[c + 256] = 9.0
        elif kind == 2 and Cn > 1:                          # in different lanes of one wave
            c = int(rng.integers(0, min(Cn, 64) - 1)) if Cn > 1 else 0; d = min(Cn - 1, c + 1 + int(rng.integers(0, 20)))
            r[d] = r[c] = 9.0
        elif kind == 3 and Cn > 64:                         # in different waves (and the later one first in its lane order)
            c = int(rng.integers(64, min(Cn, 256))); r[c] = 9.0; r[c - 64] = 9.0; r[min(Cn - 1, c + 128)] = 9.0
        elif kind == 4:                                     # +inf (twice)
            r[int(rng.integers(0, Cn))] = np.inf; r[int(rng.integers(0, Cn))] = np.inf
        elif kind == 5:                                     # all -inf
            r[:] = -np.inf
        elif kind == 6:                                     # all NaN
            r[:] = np.nan
        elif kind == 7:                                     # NaN mixed with finite values, a NaN ahead of the maximum
            r[rng.random(Cn) < 0.3] = np.nan; r[0] = np.nan
        elif kind == 8:                                     # the only finite value is -FLT_MAX
            r[:] = -np.inf; r[int(rng.integers(0, Cn))] = -FMAX
        elif kind == 9:                                     # values below -3.4e38 only, one of them the larger
            r[:] = -np.inf; r[int(rng.integers(0, Cn))] = -3.40e38; r[Cn - 1] = -3.401e38 if Cn > 1 else r[Cn - 1]
        elif kind == 10:                                    # the maximum at the last column
            r[Cn - 1] = 50.0
        elif kind == 11 and Cn > 1:                         # -inf everywhere but a NaN and one finite value
            r[:] = -np.inf; r[0] = np.nan; r[Cn - 1] = -1.0
    return z


@pytest.mark.parametrize("B", (1, 7, 64))
def test_recog_argmax_step(L, B):
    rng = np.random.default_rng(B)
    for Cn in (1, 12, 255, 256, 257, 367, 5000):
        for rot in range(12 if B == 1 else 1):              # B = 1: every row kind once
            z = np.roll(_argmax_rows(B + rot, Cn, rng), -rot, axis=0)[:B] if B == 1 else _argmax_rows(B, Cn, rng)
            ld = Cn + 5
            zd = torch.full((B, ld), float("inf"), device=DEV)      # +inf pads: a read past C would win
            zd[:, :Cn] = torch.from_numpy(z).to(DEV)
            st = 3 + rot
            step = torch.tensor([st, 0], device=DEV, dtype=torch.int32)
            out = torch.full((st + 2, B), -7, device=DEV, dtype=torch.int32)
            for rep in range(2):                            # twice in a row: the ticket counter resets
                _cabi.check(L.masr_test_recog_argmax_step(P(step), P(zd), ld, P(out), B, Cn, S()), "argmax")
            torch.cuda.synchronize()
            assert step.tolist() == [st + 2, 0], (B, Cn, step.tolist())
            want = np.full((st + 2, B), -7, np.int32)
            want[st - 1] = want[st] = [argmax_ref(z[b]) for b in range(B)]
            got = out.cpu().numpy()
            assert np.array_equal(got, want), (B, Cn, rot, np.argwhere(got != want)[:8].tolist(),
                                               [(int(got[st - 1, b]), int(want[st - 1, b])) for b in range(B) if got[st - 1, b] != want[st - 1, b]][:8])


# ---------------------------------------------------------------- beam step glue (beam.hip beam_rows_kernel without an LM + beam_select_kernel<false>)
NEG = -np.inf
SENT_TOK, SENT_SC, SENT_HIST = 12345, 777.0, -99


def row_topk_ref(z, ps, K, eos, no_eos):
    """one row's list: the K best tokens by (logit descending, token ascending), eos barred while the hypothesis is shorter than
    minlen, with fp64 scores ps + ((z - max) - logsumexp(z - max)); padded with -1 / -inf"""
    toks = [-1] * K
    scs = [NEG] * K
    if ps == NEG:
        return toks, scs
    cand = np.array([c for c in range(len(z)) if not (no_eos and c == eos)], np.int64)
    order = cand[np.lexsort((cand, -z[cand].astype(np.float64)))][:K]
    zz = z.astype(np.float64)
    mx = zz.max()
    lse = math.log(np.exp(zz - mx).sum())
    for i, c in enumerate(order):
        toks[i] = int(c)
        scs[i] = float(ps) + ((zz[c] - mx) - lse)
    return toks, scs


def select_ref(lt, ls, u, K, t, sos, eos, maxlen, best):
    """one utterance's step from its rows' lists (the kernel's own list values, so that the order is exact): candidates by (score
    descending, parent rank ascending, list position ascending = logit descending, token ascending), the K best; then tests/beam_ref.py's
    bookkeeping for one step -- an eos candidate ends its parent (t - 1 tokens), a running one takes the next row, at t = maxlen running
    hypotheses end too; the earlier / lower-ranked of equal ended scores stays; stop when nothing runs, at maxlen, or when the best ended
    score is >= the best running one.  -> (tok row, par row, score row, best, fin, number of eos candidates taken)"""
    r0 = u * K
    cands = []
    for k in range(K):
        for h in range(K):
            c, sc = int(lt[r0 + k, h]), ls[r0 + k, h]
            if c >= 0 and sc != NEG:
                cands.append((-float(sc), k, h, c, sc))
    cands.sort(key=lambda x: (x[0], x[1], x[2]))
    bs, bl, br = best
    tok, par, score = [sos] * K, [r0 + k for k in range(K)], [F32(NEG)] * K
    j, run_best, ended = 0, NEG, 0
    for _, k, _, c, sc in cands[:K]:
        if c == eos:
            ended += 1
            if sc > bs:
                bs, bl, br = sc, t - 1, r0 + k
            continue
        tok[j], par[j], score[j] = c, r0 + k, sc
        if run_best == NEG:
            run_best = sc
        if t >= maxlen and sc > bs:
            bs, bl, br = sc, t, r0 + j
        j += 1
    fin = int(j == 0 or t >= maxlen or bs >= run_best)
    return tok, par, score, (bs, bl, br), fin, ended


def _beam_inputs(B, K, Cn, t, rng, case):
    """logits / beam state for one step; utterance kinds (rotated by case): 0 plain, 1 finished, 2 eos barred (with a large eos logit),
    3 t = maxlen, 4 eos on top (stop rule, shrinking beam), 5 dead rows.  Every kind: rows 0 and 1 identical (logits and score), equal
    logits inside rows."""
    R = B * K
    eos, sos = Cn - 1, 0
    z = (rng.standard_normal((R, Cn)) * 3.0).astype(F32)
    ps = (-rng.random(R) * 10.0).astype(F32)
    if t == 1:
        ps[np.arange(R) % K != 0] = NEG                    # at step 1 only rank 0 is live
    fin = np.zeros(B, np.int32)
    minlen = np.zeros(B, np.int32)
    maxlen = np.full(B, t + 10, np.int32)
    bs = np.full(B, NEG, F32)
    bl = np.zeros(B, np.int32)
    br = np.arange(B, dtype=np.int32) * K
    for u in range(B):
        kind = (u + case) % 6
        rows = slice(u * K, (u + 1) * K)
        zu, pu = z[rows], ps[rows]
        for r in range(K):                                  # equal logits: the row's two best and two others
            a, b = rng.choice(Cn, size=2, replace=False) if Cn > 1 else (0, 0)
            zu[r, a] = zu[r, b] = zu[r].max()
            if Cn > 3:
                a, b = rng.choice(Cn, size=2, replace=False)
                zu[r, a] = zu[r, b]
        if K > 1 and t > 1:                                 # identical rows: bit-identical scores, the lower rank must win
            zu[1] = zu[0]
            pu[1] = pu[0]
        if kind == 1:
            fin[u] = 1
            bs[u], bl[u], br[u] = -1.5, t - 2, u * K + 1
        elif kind == 2:
            minlen[u] = t
            zu[:, eos] = zu.max(axis=1) + 2.0
        elif kind == 3:
            maxlen[u] = t
            bs[u], bl[u], br[u] = -4.0, t - 1, u * K
        elif kind == 4:
            zu[0, eos] = zu[0].max() + 6.0
            if K > 2:
                zu[2, eos] = zu[2].max() + 6.0
            pu[0] = pu.max() + 1.0 if np.isfinite(pu.max()) else pu[0]
            if K > 1 and t > 1:
                pu[1] = pu[0]; zu[1] = zu[0]
            bs[u], bl[u], br[u] = -30.0, t - 1, u * K
        elif kind == 5 and t > 1 and K > 1:
            pu[K // 2:] = NEG
    return z, ps, fin, minlen, maxlen, (bs, bl, br), sos, eos


BEAM_CASES = [(1, 1, 367, 4), (3, 1, 12, 2), (16, 1, 5000, 9), (1, 4, 367, 1), (3, 4, 5, 3), (16, 4, 367, 2), (1, 20, 12, 5),
              (3, 20, 367, 1), (16, 20, 64, 37), (1, 64, 5000, 2), (3, 64, 40, 6), (16, 64, 367, 3)]


@pytest.mark.parametrize("B,K,Cn,t", BEAM_CASES)
def test_beam_step(L, B, K, Cn, t):
    rng = np.random.default_rng(B * 1000 + K * 10 + t)
    for case in range(6 if B < 16 else 1):                  # B = 1, 3: every utterance kind in turn
        R = B * K
        z, ps, fin, minlen, maxlen, best, sos, eos = _beam_inputs(B, K, Cn, t, rng, case)
        ld = Cn + 3
        zd = torch.full((R, ld), NAN, device=DEV)
        zd[:, :Cn] = torch.from_numpy(z).to(DEV)
        T = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)   # noqa: E731
        score_d, fin_d = T(ps, torch.float32), T(fin)
        bs_d, bl_d, br_d = T(best[0], torch.float32), T(best[1]), T(best[2])
        lt = torch.full((R, K), SENT_TOK, device=DEV, dtype=torch.int32)
        ls = torch.full((R, K), SENT_SC, device=DEV)
        th = torch.full((R,), SENT_HIST, device=DEV, dtype=torch.int32)
        ph = torch.full((R,), SENT_HIST, device=DEV, dtype=torch.int32)
        step = torch.zeros(2, device=DEV, dtype=torch.int32)
        minlen_d, maxlen_d = T(minlen), T(maxlen)           # (held: a temporary's block could be handed out again before the launch)
        _cabi.check(L.masr_test_beam_step(B, K, Cn, sos, eos, t, P(minlen_d), P(maxlen_d), P(zd), ld, P(score_d), P(fin_d), P(bs_d),
                                          P(bl_d), P(br_d), P(lt), P(ls), P(th), P(ph), P(step), S()), "beam_step")
        torch.cuda.synchronize()
        what = (B, K, Cn, t, case)
        assert step.tolist() == [t + 1, 0], (what, step.tolist())      # every utterance takes its ticket, finished ones included
        glt, gls = lt.cpu().numpy(), ls.cpu().numpy()
        gth, gph, gsc, gfin = th.cpu().numpy(), ph.cpu().numpy(), score_d.cpu().numpy(), fin_d.cpu().numpy()
        gbs, gbl, gbr = bs_d.cpu().numpy(), bl_d.cpu().numpy(), br_d.cpu().numpy()
        for u in range(B):
            rows = slice(u * K, (u + 1) * K)
            wu = what + (u,)
            if fin[u]:                                      # a finished utterance: nothing of it is written
                assert (glt[rows] == SENT_TOK).all() and (gls[rows] == SENT_SC).all(), ("lists of a finished utterance", wu)
                assert (gth[rows] == SENT_HIST).all() and (gph[rows] == SENT_HIST).all(), ("history of a finished utterance", wu)
                assert np.array_equal(gsc[rows], ps[rows]) and gfin[u] == 1, wu
                assert (gbs[u], gbl[u], gbr[u]) == (best[0][u], best[1][u], best[2][u]), wu
                continue
            no_eos = (t - 1) < minlen[u]
            for r in range(u * K, (u + 1) * K):
                toks, scs = row_topk_ref(z[r], ps[r], K, eos, no_eos)
                assert glt[r].tolist() == toks, ("row list tokens", wu, r, glt[r].tolist(), toks)
                want = np.array(scs)
                fin_ = np.isfinite(want)
                assert np.array_equal(np.isneginf(gls[r]), ~fin_), ("row list padding", wu, r)
                assert (np.abs(gls[r][fin_] - want[fin_]) <= 1e-5).all(), ("row list scores", wu, r, np.abs(gls[r][fin_] - want[fin_]).max())
            tok, par, score, (bs, bl, br), f, _ = select_ref(glt, gls, u, K, t, sos, eos, maxlen[u], (best[0][u], best[1][u], best[2][u]))
            assert gth[rows].tolist() == tok and gph[rows].tolist() == par, ("tokens / parents", wu, gth[rows].tolist(), tok,
                                                                              gph[rows].tolist(), par)
            assert np.array_equal(gsc[rows], np.array(score, F32)), ("scores", wu)
            assert (gbs[u], gbl[u], gbr[u]) == (F32(bs), bl, br), ("best ended", wu, (gbs[u], gbl[u], gbr[u]), (bs, bl, br))
            assert gfin[u] == f, ("finished flag", wu)


def test_beam_step_features_reached():
    """the inputs of test_beam_step do reach the cases they are meant for (a property of the inputs, checked on the restatement)"""
    seen = set()
    for B, K, Cn, t in BEAM_CASES:
        rng = np.random.default_rng(B * 1000 + K * 10 + t)
        for case in range(6 if B < 16 else 1):
            z, ps, fin, minlen, maxlen, best, sos, eos = _beam_inputs(B, K, Cn, t, rng, case)
            for u in range(B):
                if fin[u]:
                    seen.add("finished"); continue
                lists = [row_topk_ref(z[r], ps[r], K, eos, (t - 1) < minlen[u]) for r in range(u * K, (u + 1) * K)]
                lt = np.array([x[0] for x in lists]); ls = np.array([x[1] for x in lists], F32)
                if Cn < K:
                    seen.add("C<K")
                if (ls == NEG).all(axis=1).any():
                    seen.add("dead row")
                if K > 1 and t > 1 and np.isfinite(ps[u * K]) and np.array_equal(ls[0], ls[1]):
                    seen.add("identical rows")
                if minlen[u] > t - 1:
                    seen.add("eos barred")
                pad = np.zeros((B * K, K), np.int32); pads = np.zeros((B * K, K), F32)
                pad[u * K:(u + 1) * K], pads[u * K:(u + 1) * K] = lt, ls
                tok, par, score, (bs, bl, br), f, ended = select_ref(pad, pads, u, K, t, sos, eos, maxlen[u],
                                                                     (best[0][u], best[1][u], best[2][u]))
                if t >= maxlen[u]:
                    seen.add("maxlen")
                if ended and score[K - 1] == NEG:
                    seen.add("shrunk")
                if f and t < maxlen[u] and bs >= score[0] and score[0] != NEG:
                    seen.add("stop rule")
    assert seen >= {"finished", "C<K", "dead row", "identical rows", "eos barred", "maxlen", "shrunk", "stop rule"}, seen


def test_beam_step_errors(L):
    z = torch.zeros(4, 8, device=DEV)
    i = torch.zeros(64, device=DEV, dtype=torch.int32)
    f = torch.zeros(64, device=DEV)
    for K in (0, 65):
        assert L.masr_test_beam_step(1, K, 8, 7, 7, 1, P(i), P(i), P(z), 8, P(f), P(i), P(f), P(i), P(i), P(i), P(f), P(i), P(i), P(i),
                                     S()) != 0
    assert L.masr_last_error()
