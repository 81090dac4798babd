"""The persistent conv grids under a workgroup cap (csrc/conv.hip conv_grid_limit) compute the bits of the uncapped launch (GPU).

From three task slots on the training step caps its persistent conv grids (ConvArgs::shared: 5/8 of the CUs for the tile-counter kernels,
half of them for the static walks).  Which workgroup computes a tile
or a partial slab changes; what is computed and the order it is added in must not:
* the counter-fed kernels (conv3x3_stream_kernel in its forward, sign-bit, masked and UNPOOL flavours, conv3x3_resw_kernel) hand tiles to
  whoever asks, and the last workgroup to run dry -- counted against the launched grid -- re-arms the counter (every case launches twice);
* the static-walk kernels (conv3x3_wgrad2_kernel, conv3x3_resw_w1x_kernel) keep their partition into partial slabs and run it as virtual
  workgroups: a launched workgroup runs several ids one after the other, writes each id's slab and zeroes its accumulators.
masr_test_set_conv_grid_cap forces a cap in workgroups whatever the launch's hint says, so that maps of a few tiles reach those paths.  Every
case runs with the hook at 0, then under each cap, and every output must be np.array_equal.  Operands are standard normals: the summation
order is part of the bits compared.  The hook overrides `shared`: the `shared >= 3` branch of conv_grid_limit and its plumbing through train.hip
are not reached by these tests (the bench A/B per slot count and the kernel profile are what exercise them)."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))
import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


@pytest.fixture
def cap(L):
    """cap(n) sets the hook; it is back at 0 when the test ends, passed or not"""
    yield lambda n: L.masr_test_set_conv_grid_cap(int(n))
    L.masr_test_set_conv_grid_cap(0)


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy() for t in ts]


def _same_under_caps(cap, run, caps):
    """run() -> list of arrays.  Uncapped once (the reference, not recomputed), then twice under every cap: the second launch on the same stream
    finds the tile counter as the first one left it."""
    cap(0)
    want = run()
    assert any(np.any(w != 0) for w in want)
    for n in caps:
        cap(n)
        for rep in range(2):
            got = run()
            for i, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), (n, rep, i)


@functools.lru_cache(maxsize=None)
def _fwd_operands(B, H, W, CIN, COUT):
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W + CIN)
    x = torch.randn(B, H, W, CIN, device="cuda", generator=g).bfloat16()
    wk = (torch.randn(COUT, 9 * CIN, device="cuda", generator=g) * 0.05).bfloat16()
    bias = torch.randn(COUT, device="cuda", generator=g) * 0.3
    return x, wk, bias


def _pool_idx_run(L, B, H, W, CIN, COUT):
    x, wk, bias = _fwd_operands(B, H, W, CIN, COUT)

    def run():
        out = torch.zeros(B, H, W, COUT, device="cuda").bfloat16()
        pool = torch.zeros(B, H // 2, W // 2, COUT, device="cuda").bfloat16()
        idx = torch.full((B, H // 2, W // 2, COUT), 9, device="cuda", dtype=torch.uint8)
        _cabi.check(L.masr_test_conv3x3_pool_idx(P(x), P(wk), P(bias), P(out), P(pool), P(idx), 0, B, H, W, CIN, COUT, S()))
        return _np(out, pool, idx)
    return run


def test_stream_forward_with_pool(L, cap):
    """conv3x3_stream_kernel<128,128,32,8,0>: 3 x 2 = 6 tiles; one workgroup walks all, three take two each, four leave two with one"""
    _same_under_caps(cap, _pool_idx_run(L, 1, 40, 20, 128, 128), (1, 3, 4))


def test_resw_forward_with_pool(L, cap):
    """conv3x3_resw_kernel: 3 x 3 = 9 tiles of 16 x 16"""
    _same_under_caps(cap, _pool_idx_run(L, 1, 33, 40, 64, 64), (1, 2, 4))


def test_stream_forward_sign_bits(L, cap):
    """conv3x3_stream_kernel<64,128,16,8,0> writing the ReLU sign words of its output"""
    B, H, W = 1, 33, 21
    x, wk, bias = _fwd_operands(B, H, W, 64, 128)

    def run():
        out = torch.zeros(B, H, W, 128, device="cuda").bfloat16()
        bits = torch.full((B, H, W, 4), -1, device="cuda", dtype=torch.int32)
        _cabi.check(L.masr_test_conv3x3_sign_bits(P(x), P(wk), P(bias), 1, None, None, P(out), P(bits), B, H, W, 64, 128, S()))
        return _np(out, bits)
    _same_under_caps(cap, run, (1, 2))


@functools.lru_cache(maxsize=None)
def _pooled_gradient(B, H, W, Cc):
    g = torch.Generator(device="cuda").manual_seed(7 * H + W + Cc)
    dyp = torch.randn(B, H // 2, W // 2, Cc, device="cuda", generator=g).bfloat16()
    codes = torch.randint(0, 5, (B, H // 2, W // 2, Cc), device="cuda", generator=g).to(torch.uint8)      # 4 = nothing passed the ReLU
    wdk = (torch.randn(Cc, 9 * Cc, device="cuda", generator=g) * 0.05).bfloat16()
    return dyp, codes, wdk, g


def _unpool(codes, gp, H, W):
    """MaxPool2d(2, 2) + ReLU backward from the pool codes -- indexing only, exact (as tests/test_hip_kernels.py)"""
    B, H2, W2, Cc = gp.shape
    exp = torch.zeros(B, H2, W2, Cc, 4, device=gp.device, dtype=gp.dtype)
    exp.scatter_(-1, codes.long().clamp(max=3).unsqueeze(-1), torch.where(codes < 4, gp, torch.zeros_like(gp)).unsqueeze(-1))
    full = torch.zeros(B, H, W, Cc, device=gp.device, dtype=gp.dtype)
    full[:, :2 * H2, :2 * W2] = exp.reshape(B, H2, W2, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H2, 2 * W2, Cc)
    return full.contiguous()


def test_stream_dgrad_behind_the_pool(L, cap):
    """the UNPOOL flavour: a workgroup's first tile is its index, the later ones the launched grid + the counter"""
    B, H, W = 2, 40, 20
    dyp, codes, wdk, g = _pooled_gradient(B, H, W, 128)
    words = torch.randint(-2 ** 31, 2 ** 31, (B, H, W, 4), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)

    def run():
        o = torch.full((B, H, W, 128), 7.0, device="cuda").bfloat16()
        _cabi.check(L.masr_test_conv3x3_dgrad_pooled(None, P(dyp), P(codes), P(wdk), P(words), P(o), B, H, W, S()))
        return _np(o)
    _same_under_caps(cap, run, (1, 5))


# (shape, caps).  Virtual workgroups per channel block = min(256 / blocks, tiles); the cap counts workgroups of the whole grid, blocks per id.
# 1x17x80, 64 -> 64: 15 ids of one tile, one block: 4 does not divide 15.  2x40x20, 128 -> 128: 18 ids, four blocks: 1 and 2 leave one workgroup
# per block, 16 gives four (18 = 4 + 4 + 4 + 4 + 2 ids), 20 five.  4x200x160: 1 000 tiles on 256 ids of four or three tiles -- both staging
# registers rotate across an id boundary, odd and even walks alternate the LDS buffer an id starts on; 128 workgroups run two ids each, 96
# become 86 running three (the last of them two).
WGRAD_CASES = [((1, 17, 80, 64, 64), (1, 2, 4)), ((2, 40, 20, 128, 128), (1, 2, 16, 20)), ((4, 200, 160, 64, 64), (128, 96))]


@functools.lru_cache(maxsize=None)
def _wgrad_operands(shape):
    B, H, W, CIN, COUT = shape
    g = torch.Generator(device="cuda").manual_seed(H + W + CIN)
    x = torch.randn(B, H, W, CIN, device="cuda", generator=g).bfloat16()
    dyp = torch.randn(B, H // 2, W // 2, COUT, device="cuda", generator=g).bfloat16()
    codes = torch.randint(0, 5, (B, H // 2, W // 2, COUT), device="cuda", generator=g).to(torch.uint8)
    return x, dyp, codes, _unpool(codes, dyp, H, W)


@pytest.mark.parametrize("shape,caps", WGRAD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_wgrad2_plain(L, cap, shape, caps):
    B, H, W, CIN, COUT = shape
    x, _, _, dy = _wgrad_operands(shape)
    n = int(L.masr_test_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT))

    def run():
        slab = torch.zeros(n, device="cuda")
        dw = torch.full((COUT, CIN, 3, 3), 7.0, device="cuda")
        _cabi.check(L.masr_test_conv3x3_wgrad(P(x), P(dy), P(dw), P(slab), n, B, H, W, CIN, COUT, S()))
        return _np(dw, slab)
    _same_under_caps(cap, run, caps)


@pytest.mark.parametrize("shape,caps", WGRAD_CASES[1:], ids=lambda v: "x".join(map(str, v)))
def test_wgrad2_pooled(L, cap, shape, caps):
    """with the bias gradient: its partials are folded per id, out of the LDS buffer the id's first tile had"""
    B, H, W, CIN, COUT = shape
    x, dyp, codes, _ = _wgrad_operands(shape)
    n = int(L.masr_test_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT))

    def run():
        slab = torch.zeros(n, device="cuda")
        dw = torch.full((COUT, CIN, 3, 3), 7.0, device="cuda")
        db = torch.full((COUT,), 7.0, device="cuda")
        _cabi.check(L.masr_test_conv3x3_wgrad_pooled(P(x), P(dyp), P(codes), P(dw), P(db), P(slab), n, B, H, W, CIN, COUT, S()))
        return _np(dw, db, slab)
    _same_under_caps(cap, run, caps)


# 1x33x40: 9 tiles = 9 rows of one tile.  4x200x160: 520 tiles on 256 rows of three or two tiles, the patch pipeline running across the ids.
@pytest.mark.parametrize("B,H,W,caps", [(1, 33, 40, (1, 2, 4)), (4, 200, 160, (128, 96))])
@pytest.mark.parametrize("pooled", [False, True], ids=["map", "pooled"])
def test_conv1_wgrad_fused(L, cap, pooled, B, H, W, caps):
    """conv3x3_resw_w1x_kernel, the DMA flavour (fed the map) and the UNPOOL flavour (fed the pooled gradient + codes)"""
    dyp, codes, wdk, g = _pooled_gradient(B, H, W, 64)
    dy = _unpool(codes, dyp, H, W)
    x1 = torch.randn(B, H, W, device="cuda", generator=g)
    words = torch.randint(-2 ** 62, 2 ** 62, (B, H, W), device="cuda", generator=g, dtype=torch.int64)
    n = int(L.masr_test_conv1_wgrad_fused_slab_floats(B, H, W))

    def run():
        slab = torch.zeros(n, device="cuda")
        dw = torch.full((64, 9), 3.0, device="cuda")
        db = torch.full((64,), 3.0, device="cuda")
        a = (None, P(dyp), P(codes)) if pooled else (P(dy), None, None)
        _cabi.check(L.masr_test_conv1_wgrad_fused(*a, P(wdk), P(words), P(x1), P(slab), n, P(dw), P(db), B, H, W, S()))
        return _np(dw, db, slab)
    _same_under_caps(cap, run, caps)


def test_training_step_beside_other_slots(L, cap):
    """one run_batch(train=True) of the tiny transformer as one of four task slots, every conv grid capped at 3 workgroups, against the lone
    uncapped slot: loss, logits and the whole gradient buffer bit for bit"""
    from masr_amd.engine import MasrEngine
    from oracle import ref_cpu
    from oracle.make_goldens import TINY, ODIM, synth_batch
    sd = ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)
    xs, il, ys, ol = synth_batch(11, [64, 52, 40, 33], [9, 7, 5, 3])

    def step(slots, n):
        cap(n)
        eng = MasrEngine(TINY, ODIM, label_smoothing=0.2)
        eng.load_state_dict(sd)
        eng.set_concurrency(slots)
        eng.run_batch(xs, il, ys, ol, train=True)
        loss = eng.read_stats()["loss"]
        lg, gd = eng.last_logits()
        return [np.float32(loss)] + _np(lg.clone(), gd.clone(), eng.grads.clone())
    want = step(1, 0)
    got = step(4, 3)
    assert np.isfinite(want[0]) and np.any(want[3] != 0)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), i
