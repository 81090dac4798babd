"""The shared epilogue of the Linear GEMMs (gemm.hip gemm_epilogue), bit for bit (GPU).

A and B hold integers in [-3, 3] and K <= 256, so every accumulation order gives the same fp32 sum; bias, residual, positional encoding and
the accumulated-into output are multiples of 1/8.  The expected output is then the epilogue restated in torch fp32 in the kernel's documented
order (alpha = 1, bias, pe, relu, mask, dropout, residual, accumulate) with the keep-scales of masr_test_dropout_mask, and is compared with
torch.equal on the bit patterns of both outputs (bf16 rounded to nearest-even), so that the sign of a zero counts too.  The stages behind
the dropout are adds even where they add nothing (`+ 0`), which is what makes a dropped negative value a +0 in the output.  Every output
is followed by a sentinel row, and padded rows by sentinel columns, that must stay untouched.

Shapes: the smallest that reach each kernel form and edge case (mk_gemm picks the tile by workgroup count against 192, launch_glds the
loader-wave form by workgroup count against the CU count):
  130 x 200 x 64     gemm_ring_kernel<64, 64>: ragged rows, a last column tile with 8 of 64 columns
  130 x 203 x 64     odd N: the scalar store paths and, with dropout, the odd-start hash path
  1601 x 1020 x 128  gemm_ring_kernel<128, 64>, 208 workgroups; N a multiple of 4 and not of 8: the last 8-wide strip is half valid
  1601 x 1280 x 64   gemm_glds_kernel<128, 64>, 260 workgroups (more than the CUs)
  1601 x 1924 x 64   gemm_glds_kernel<128, 128>, 208 workgroups: interior and edge tiles in one launch
  1601 x 1928 x 64   the same kernel with N a multiple of 8: its bf16 epilogues take the interior path too
  130 x 200 x 72     K not a multiple of 64: gemm_kernel"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402

SHAPES = [(130, 200, 64), (130, 203, 64), (1601, 1020, 128), (1601, 1280, 64), (1601, 1924, 64), (1601, 1928, 64), (130, 200, 72)]
# flavour -> (bias, relu, mask, residual, fp32 output): the specialised epilogues of the training step that masr_test_gemm_epi reaches
FLAVOURS = {
    "bias_bf16": (True, False, False, False, False),
    "bias_res_fp32": (True, False, False, True, True),
    "bias_relu_bf16": (True, True, False, False, False),
    "plain_bf16": (False, False, False, False, False),
    "mask_bf16": (False, False, True, False, False),
    "res_fp32": (False, False, False, True, True),
    "plain_fp32": (False, False, False, False, True),
    "bias_fp32": (True, False, False, False, True),
}
SENT = 77.0


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


def eighths(shape, g):
    return (torch.randint(-16, 17, shape, generator=g).float() / 8).cuda()


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """A, B (bf16, integers in [-3, 3]), their exact product in fp32 and the side inputs of the shape; computed once, never written"""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randint(-3, 4, (M, K), generator=g).float().cuda().bfloat16()
    B = torch.randint(-3, 4, (N, K), generator=g).float().cuda().bfloat16()
    acc = (A.double() @ B.double().t()).float()                  # |sum| <= 9 K: exact in fp32 whatever the order
    bias = eighths((N,), g)
    res = torch.empty(M * N + 4, device="cuda")                   # [4:] sits on a 16-byte boundary, [1:] does not
    res[1:1 + M * N] = eighths((M * N,), g)
    res[4:] = res[1:1 + M * N].clone()
    mask = (torch.rand(M, N, generator=g) > 0.4).cuda().bfloat16()
    return A, B, acc, bias, res, mask


@functools.lru_cache(maxsize=None)
def keep_scale(seed, site, M, N, p):
    k = torch.empty(M * N, device="cuda")
    _cabi.check(_cabi.lib().masr_test_dropout_mask(seed, site, M * N, p, P(k), S()), "dropout_mask")
    return k.view(M, N)


def expected(acc, bias=None, pe=None, relu=False, mask=None, keep=None, res=None, old=None):
    x = acc                                                      # alpha = 1
    if bias is not None:
        x = x + bias
    if pe is not None:
        x = x + pe
    if relu:
        x = torch.clamp_min(x, 0.0)
    if mask is not None:
        x = torch.where(mask.float() > 0, x * 1.0, torch.zeros_like(x))
    if keep is not None:
        x = x * keep
    x = x + (res if res is not None else 0.0)                    # (-0 + 0 = +0)
    return x + (old if old is not None else 0.0)


def check_out(C32, C16, want, M, N):
    """C32 [M + 1][ld], C16 [M + 1][ld] (or None): exact inside, sentinel outside"""
    if C32 is not None:
        got, w32 = C32[:M, :N].contiguous().view(torch.int32), want.contiguous().view(torch.int32)
        assert torch.equal(got, w32), f"fp32 output: {int((got != w32).sum())} bit patterns differ"
        assert bool((C32[M] == SENT).all()) and bool((C32[:M, N:] == SENT).all()), "fp32 output: written outside M x N"
    if C16 is not None:
        got, w16 = C16[:M, :N].contiguous().view(torch.int16), want.bfloat16().view(torch.int16)
        assert torch.equal(got, w16), f"bf16 output: {int((got != w16).sum())} bit patterns differ"
        assert bool((C16[M].float() == SENT).all()) and bool((C16[:M, N:].float() == SENT).all()), "bf16 output: written outside M x N"


def outputs(M, N, fp32, ld=None):
    ld = ld or N
    if fp32:
        return torch.full((M + 1, ld), SENT, device="cuda"), None
    return None, torch.full((M + 1, ld), SENT, device="cuda").bfloat16()


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogue_exact(L, M, N, K, flavour):
    """each specialised epilogue without and with dropout (seed 1, site 2 inside masr_test_gemm_epi) on each kernel form"""
    has_bias, relu, has_mask, has_res, fp32 = FLAVOURS[flavour]
    A, B, acc, bias, res, mask = operands(M, N, K)
    r = res[4:].view(M, N) if has_res else None
    for p in (0.0, 0.1):
        C32, C16 = outputs(M, N, fp32)
        _cabi.check(L.masr_test_gemm_epi(P(A), K, P(B), K, M, N, K, P(bias) if has_bias else None, int(relu), p, P(r), P(mask) if has_mask else None,
                                         P(C32), P(C16), S()), "gemm_epi")
        want = expected(acc, bias if has_bias else None, None, relu, mask if has_mask else None,
                        keep_scale(1, 2, M, N, p) if p > 0 else None, r)
        check_out(C32, C16, want, M, N)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dropout_seed_site(L, M, N, K):
    """plain -> fp32 with dropout through masr_test_gemm_dropout (its own seed and site)"""
    A, B, acc, _, _, _ = operands(M, N, K)
    C32, _ = outputs(M, N, True)
    _cabi.check(L.masr_test_gemm_dropout(P(A), K, P(B), K, M, N, K, 0.1, 77, 3, P(C32), N, S()), "gemm_dropout")
    check_out(C32, None, expected(acc, keep=keep_scale(77, 3, M, N, 0.1)), M, N)


def test_dropout_odd_width_aligned_rows(L):
    """odd N under a row pitch of N + 1: every stream is 16-byte aligned, so interior tiles pass the alignment test of the short path, but
    element indices m N + n start odd in every other row: those tiles must still take the three-word hash"""
    M, N, K = 130, 203, 64
    A, B, acc, _, _, _ = operands(M, N, K)
    C32, _ = outputs(M, N, True, N + 1)
    _cabi.check(L.masr_test_gemm_dropout(P(A), K, P(B), K, M, N, K, 0.1, 77, 3, P(C32), N + 1, S()), "gemm_dropout")
    check_out(C32, None, expected(acc, keep=keep_scale(77, 3, M, N, 0.1)), M, N)


@pytest.mark.parametrize("pad", [8, 5])
@pytest.mark.parametrize("M,N,K", [(130, 200, 64), (1601, 1924, 64), (130, 200, 72)])
def test_padded_fp32_rows(L, M, N, K, pad):
    """bias (+ ReLU) -> fp32 with a row pitch larger than N: 8 further (16-byte stores) and 5 further (rows off the boundary: scalar
    stores); the pad columns stay untouched"""
    A, B, acc, bias, _, _ = operands(M, N, K)
    for relu in (0, 1):
        C32, _ = outputs(M, N, True, N + pad)
        _cabi.check(L.masr_test_gemm(P(A), K, P(B), K, M, N, K, 0, P(bias), relu, P(C32), N + pad, S()), "gemm")
        check_out(C32, None, expected(acc, bias, relu=bool(relu)), M, N)


@pytest.mark.parametrize("has_bias", [True, False])
@pytest.mark.parametrize("M,N,K", [(130, 200, 64), (1601, 1280, 64), (1601, 1924, 64)])
def test_unaligned_residual(L, M, N, K, has_bias):
    """a residual 4 bytes off a 16-byte boundary: its loads take the scalar path (every tile the general one), still exact"""
    A, B, acc, bias, res, _ = operands(M, N, K)
    r = res[1:1 + M * N].view(M, N)
    assert r.data_ptr() % 16 == 4
    for p in (0.0, 0.1):
        C32, _ = outputs(M, N, True)
        _cabi.check(L.masr_test_gemm_epi(P(A), K, P(B), K, M, N, K, P(bias) if has_bias else None, 0, p, P(r), None, P(C32), None, S()), "gemm_epi")
        check_out(C32, None, expected(acc, bias if has_bias else None, keep=keep_scale(1, 2, M, N, p) if p > 0 else None, res=r), M, N)


@pytest.mark.parametrize("M,N,K", [(130, 200, 64), (130, 203, 64), (1601, 1280, 64), (1601, 1924, 64), (1601, 1928, 64), (130, 200, 72)])
def test_positional_encoding(L, M, N, K):
    """bias + pe -> fp32 and bf16 in one launch (the vgg2enc epilogue): pe row m % 50, a period that divides no tile height; padded rows
    (N = 1924: the bf16 pitch is no multiple of 8, every tile takes the general path; 1928: the interior path of the 128 x 128 tiles)"""
    A, B, acc, bias, _, _ = operands(M, N, K)
    period = 50
    pe = eighths((period, N), torch.Generator().manual_seed(N))
    ld32, ld16 = N + 4, N + 8
    C32, _ = outputs(M, N, True, ld32)
    _, C16 = outputs(M, N, False, ld16)
    _cabi.check(L.masr_test_gemm_pe_acc(P(A), K, P(B), K, M, N, K, P(bias), P(pe), period, 0, P(C32), ld32, P(C16), ld16, S()), "gemm_pe_acc")
    want = expected(acc, bias, pe[torch.arange(M, device="cuda") % period])
    check_out(C32, C16, want, M, N)


@pytest.mark.parametrize("M,N,K", [(130, 200, 64), (130, 203, 64), (1601, 1020, 128), (1601, 1924, 64), (130, 200, 72)])
def test_accumulate(L, M, N, K):
    """C32 += A B^T (the memory gradient summed over decoder layers)"""
    A, B, acc, _, _, _ = operands(M, N, K)
    C32, _ = outputs(M, N, True)
    old = eighths((M, N), torch.Generator().manual_seed(M + N))
    C32[:M] = old
    _cabi.check(L.masr_test_gemm_pe_acc(P(A), K, P(B), K, M, N, K, None, None, 0, 1, P(C32), N, None, 0, S()), "gemm_pe_acc")
    check_out(C32, None, expected(acc, old=old), M, N)
