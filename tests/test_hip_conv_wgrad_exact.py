"""conv3x3_wgrad2_kernel (csrc/conv.hip) to the bit, through masr_test_conv3x3_wgrad / _wgrad_pooled (GPU).

* Integer operands: bf16 values in {-2 .. 2}, so every product is an integer of magnitude <= 4 and every fp32 sum of them is exact in ANY
  order as long as the sum of the magnitudes stays below 2^24 (checked on the CPU for the inputs drawn here).  dw and db must then EQUAL an
  integer restatement of the definition -- a half-fragment taken from the wrong patch row or column shift, a register window that survives a
  tile or LDS-buffer change, or a halo / ragged-tile chunk that was not zero all change an integer.
* Normal operands: the summation ORDER is part of the result's bits.  The SHA-256 of dw / db must be the one the library of the commit
  before the kernel's half-fragment window and buffer-load staging produced (tests/golden/conv_wgrad_parent_digests.json, recorded on an
  MI355X by running this file as a script with MASR_LIB naming that library: `python tests/test_hip_conv_wgrad_exact.py OUT.json`).
"""
import ctypes as C
import functools
import hashlib
import json
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

DIGESTS = REPO / "tests" / "golden" / "conv_wgrad_parent_digests.json"

# (B, H, W, CIN, COUT): each the smallest shape that reaches a distinct path of the kernel
SHAPES = [
    (1, 8, 16, 64, 64),       # 16-wide tile, exactly one: every patch row is read
    (1, 17, 80, 64, 64),      # conv2's width: a ragged last tile row, left and right edges
    (2, 10, 9, 64, 64),       # a map smaller than a tile
    (2, 40, 20, 128, 128),    # 8-wide tiles, three tile columns for 20 columns; channel slabs cs > 0 carry no bias gradient
    (1, 33, 21, 64, 128),     # 8-wide as the launcher picks it; output-channel half ch > 0
    (1, 21, 47, 128, 128),    # odd H and W: the row and column a floor-mode pool crops
    (4, 200, 160, 64, 64),    # 1 000 tiles on 256 workgroups: every workgroup walks >= 3 (both staging registers rotate, walk-end re-reads)
]
RANDN_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[4]]


def _pooled_ok(shape):
    return shape[3] == shape[4] and shape[3] in (64, 128)


CASES = [(s, m) for s in SHAPES for m in ("plain", "pooled") if m == "plain" or _pooled_ok(s)]
RANDN_CASES = [(s, m) for s in RANDN_SHAPES for m in ("plain", "pooled") if m == "plain" or _pooled_ok(s)]


def _ident(case):
    (B, H, W, CIN, COUT), mode = case
    return f"{B}x{H}x{W}x{CIN}x{COUT}-{mode}"


def _unpool(codes, gp, H, W):
    """MaxPool2d(2, 2) + ReLU backward from pool codes (window position 0..3, row-major; 4 = nothing passed the ReLU) -- numpy, exact"""
    B, H2, W2, Cc = gp.shape
    full = np.zeros((B, H, W, Cc), gp.dtype)
    for k in range(4):
        full[:, (k >> 1):2 * H2:2, (k & 1):2 * W2:2] = np.where(codes == k, gp, 0)
    return full


@functools.lru_cache(maxsize=None)
def _operands(shape, mode, kind):
    """x [B][H][W][CIN], and dy [B][H][W][COUT] (plain) or pooled dy + codes [B][H/2][W/2][COUT] (pooled); float32 arrays of bf16-exact values
    ("int": integers in -2 .. 2) or standard normals ("randn", rounded to bf16 on upload).  numpy's RandomState: the same stream everywhere."""
    B, H, W, CIN, COUT = shape
    rs = np.random.RandomState(((1000 * H + W) * 4 + CIN // 64) * 4 + 2 * (mode == "pooled") + (kind == "randn"))
    draw = (lambda *s: rs.randint(-2, 3, s).astype(np.float32)) if kind == "int" else (lambda *s: rs.standard_normal(s).astype(np.float32))
    x = draw(B, H, W, CIN)
    if mode == "plain":
        return x, draw(B, H, W, COUT), None
    return x, draw(B, H // 2, W // 2, COUT), rs.randint(0, 5, (B, H // 2, W // 2, COUT)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _integer_reference(shape, mode):
    """dw[co][ci][ky][kx] = sum over pixels of dy[b][i][j][co] * x[b][i + ky - 1][j + kx - 1][ci] (zero outside the map), db[co] = sum of dy:
    on integers, in float64 (exact: every sum is far below 2^53) and returned as int64.  Also the bound that makes fp32 exact."""
    B, H, W, CIN, COUT = shape
    x, dy, codes = _operands(shape, mode, "int")
    if mode == "pooled":
        dy = _unpool(codes, dy, H, W)
    assert np.abs(x).max() <= 2 and np.abs(dy).max() <= 2
    # |any partial sum of dw| <= max|x| * sum over pixels of |dy[.][co]|, and db's are below the same sum
    bound = 2.0 * np.abs(dy).reshape(-1, COUT).sum(0).max()
    assert bound < 2 ** 24, bound
    xp = torch.from_numpy(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))).double()
    d2 = torch.from_numpy(dy).double().reshape(-1, COUT).t().contiguous()
    dw = torch.zeros(COUT, CIN, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d2 @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, CIN)
    db = d2.sum(1)
    assert torch.equal(dw, dw.round()) and float(dw.abs().max()) <= bound
    return dw.long(), db.long()


def _run(L, shape, mode, kind):
    """-> (dw [COUT][CIN][3][3], db [COUT] or None: the plain entry computes no bias gradient) on the CPU"""
    B, H, W, CIN, COUT = shape
    x, dy, codes = _operands(shape, mode, kind)
    P = lambda t: C.c_void_p(t.data_ptr())
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xg = torch.from_numpy(x).cuda().bfloat16()
    dyg = torch.from_numpy(dy).cuda().bfloat16()
    n = int(L.masr_test_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT))
    slab = torch.zeros(n, device="cuda")
    dw = torch.full((COUT, CIN, 3, 3), 7.0, device="cuda")
    if mode == "plain":
        _cabi.check(L.masr_test_conv3x3_wgrad(P(xg), P(dyg), P(dw), P(slab), n, B, H, W, CIN, COUT, S))
        torch.cuda.synchronize()
        return dw.cpu(), None
    cg = torch.from_numpy(codes).cuda()
    db = torch.full((COUT,), 7.0, device="cuda")
    _cabi.check(L.masr_test_conv3x3_wgrad_pooled(P(xg), P(dyg), P(cg), P(dw), P(db), P(slab), n, B, H, W, CIN, COUT, S))
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def _sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


@pytest.mark.parametrize("case", CASES, ids=_ident)
def test_wgrad_integer_operands_exact(L, case):
    shape, mode = case
    dw_ref, db_ref = _integer_reference(shape, mode)
    dw, db = _run(L, shape, mode, "int")
    assert torch.equal(dw, dw_ref.float())
    if db is not None:
        assert torch.equal(db, db_ref.float())
    assert int(dw_ref.abs().max()) > 0


@pytest.mark.parametrize("case", RANDN_CASES, ids=_ident)
def test_wgrad_same_summation_order_as_parent(L, case):
    shape, mode = case
    want = json.loads(DIGESTS.read_text())[_ident(case)]
    dw, db = _run(L, shape, mode, "randn")
    assert _sha(dw) == want["dw"]
    if db is not None:
        assert _sha(db) == want["db"]


if __name__ == "__main__":
    lib = _cabi.lib()
    out = {}
    for case in RANDN_CASES:
        dw, db = _run(lib, case[0], case[1], "randn")
        out[_ident(case)] = {"dw": _sha(dw)} if db is None else {"dw": _sha(dw), "db": _sha(db)}
    Path(sys.argv[1]).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps(out, indent=1, sort_keys=True))
