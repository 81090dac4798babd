"""The bf16 operand-shadow kernels of csrc/optim.hip alone: the one-launch refresh (all_shadows_kernel) on single jobs of every type, on a mixed
list in masr_bind's order with the cross-attention arrangement, and on a list of exactly SHADOW_JOBS_MAX jobs; and the BLSTM engine's three
passes (cast, transpose + cast, conv weight shadows).  These are index maps and one round-to-nearest-even cast, so every output is compared
bit for bit with tests/optim_ref.py -- the whole allocation, markers around and inside it (row pads, a neighbour's columns) included.  The
sources sit in one flat NaN-filled buffer at dword offsets of every residue mod 4."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
import optim_ref as O  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
GUARD = 64                                                     # marker elements around every output (128 B of bf16: the interior stays 16-byte aligned)
MARK16, MARK32 = 0x7FC5, 0x7FC5A5A5                            # NaNs as bf16 / fp32
LINEAR, CONV, VGG2ENC, COPY32 = 0, 1, 2, 3
JOBS_MAX = 56                                                  # kernels.h SHADOW_JOBS_MAX
FLAT_NS = (1, 3, 4, 5, 1023, 4101, 10007, 4 * 2 ** 20 + 4099)  # the last: past one grid stride of cast_bf16_kernel (4096 workgroups x 256 lanes)


@pytest.fixture(scope="module")
def lib():
    return _cabi.lib()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def bits16(x):
    return O.bf16(x).view(torch.int16).numpy()


class Out:
    """n output elements (bf16 as int16 words, or fp32 as int32 words), marker-filled, between GUARD markers; `exp` is the image the launch must
    leave: markers wherever nothing is expected"""

    def __init__(self, n, wide=False):
        self.np_dtype, mark = (np.int32, MARK32) if wide else (np.int16, MARK16)
        self.t = torch.full((n + 2 * GUARD,), mark, dtype=torch.int32 if wide else torch.int16, device=DEV)
        self.exp = np.full(n + 2 * GUARD, mark, self.np_dtype)
        self.size = 4 if wide else 2

    def ptr(self, at=0):
        return self.t.data_ptr() + self.size * (GUARD + at)

    def expect(self, at, mat, pitch=None):
        """rows of the 2-D array of words `mat` at element at + r * pitch"""
        mat = np.atleast_2d(mat)
        pitch = mat.shape[1] if pitch is None else pitch
        for r in range(mat.shape[0]):
            lo = GUARD + at + r * pitch
            assert (self.exp[lo:lo + mat.shape[1]] == self.exp[0]).all(), "two expectations overlap"
            self.exp[lo:lo + mat.shape[1]] = mat[r]

    def ok(self):
        got = self.t.cpu().numpy()
        bad = np.nonzero(got != self.exp)[0]
        return (True, None) if bad.size == 0 else (False, (int(bad.size), "first at element", int(bad[0]) - GUARD))

    def clean(self):
        return bool((self.t == int(self.exp[0])).all())


class Flat:
    """the flat parameter buffer: tensors appended at chosen gaps of NaN, the first at dword 4, at least four NaNs behind the last"""

    def __init__(self):
        self.parts, self.n = [], 4

    def add(self, x, gap=0):
        self.n += gap
        src = self.n
        self.parts.append((src, np.ascontiguousarray(x, F32).reshape(-1)))
        self.n += x.size
        return src

    def device(self):
        host = np.full(self.n + 8, np.nan, F32)
        for src, x in self.parts:
            host[src:src + x.size] = x
        t = torch.from_numpy(host).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t


def job(kind, src, N=0, K=0, ldt=0, a0=0, a1=0, p0=0, p1=0):
    return ((src, kind, N, K, ldt, a0, a1), (p0, p1))


def launch(lib, P, jobs, expect_rc=0):
    desc = np.ascontiguousarray([j[0] for j in jobs], np.int64).reshape(-1)
    outs = (C.c_void_p * (2 * len(jobs)))(*[p or None for j in jobs for p in j[1]])
    rc = lib.masr_test_shadow_jobs(C.c_void_p(P.data_ptr()), len(jobs), desc.ctypes.data_as(C.c_void_p), outs, S())
    assert rc == expect_rc, (rc, lib.masr_last_error().decode())
    torch.cuda.synchronize()


def all_ok(outs, what):
    for name, o in outs.items():
        ok, where = o.ok()
        assert ok, (what, name, "words that differ", where)


# what a job of each type must leave: (the job tuple, {name: Out}) with the expectations entered
def conv_job(flat, seed, CO, CI, gap=0):
    w = rnd(seed, CO, CI, 3, 3)
    wk, wd = O.conv_layouts(w)
    o = {"wk": Out(wk.size), "wd": Out(wd.size)}
    o["wk"].expect(0, bits16(wk))
    o["wd"].expect(0, bits16(wd))
    return job(CONV, flat.add(w, gap), N=CO, K=CI, p0=o["wk"].ptr(), p1=o["wd"].ptr()), o


def vgg_job(flat, seed, E, Cc, Dp, gap=0):
    w = rnd(seed, E, Cc * Dp)
    wk, wt = O.vgg2enc_layouts(w, E, Cc, Dp)
    o = {"wk": Out(wk.size), "wt": Out(wt.size)}
    o["wk"].expect(0, bits16(wk))
    o["wt"].expect(0, bits16(wt))
    return job(VGG2ENC, flat.add(w, gap), N=E, a0=Cc, a1=Dp, p0=o["wk"].ptr(), p1=o["wt"].ptr()), o


def copy_job(flat, seed, N, gap=0):
    x = rnd(seed, N)
    o = {"copy": Out(N, wide=True)}
    o["copy"].expect(0, x.view(np.int32))
    return job(COPY32, flat.add(x, gap), N=N, p0=o["copy"].ptr()), o


def linear_job(flat, seed, N, K, ldt, gap=0, t16=None, t16_at=0):
    """t16 given: the transpose goes to columns t16_at .. t16_at + N of that shared [K][ldt] matrix"""
    w = rnd(seed, N, K)
    k, t = O.linear_layouts(w)
    o = {"k16": Out(N * K)}
    o["k16"].expect(0, bits16(k))
    if t16 is None:
        t16 = o["t16"] = Out(K * ldt)
    t16.expect(t16_at, bits16(t), pitch=ldt)
    return job(LINEAR, flat.add(w, gap), N=N, K=K, ldt=ldt, p0=o["k16"].ptr(), p1=t16.ptr(t16_at)), o


def run_single(lib, make, *args):
    for gap in (0, 1, 2, 3):                                   # the source at every residue mod 4
        flat = Flat()
        j, outs = make(flat, 7 + gap, *args, gap=gap)
        launch(lib, flat.device(), [j])
        all_ok(outs, (make.__name__, args, "gap", gap))


# ---------------------------------------------------------------- single jobs
@pytest.mark.parametrize("CO,CI", ((64, 64), (128, 64), (8, 3), (5, 7)))       # the last two: ragged last workgroups
def test_conv_job(lib, CO, CI):
    run_single(lib, conv_job, CO, CI)


@pytest.mark.parametrize("E,Cc,Dp", ((64, 128, 10), (70, 6, 11), (8, 128, 20)))     # (70, 6, 11): 66 columns, ragged tiles both ways
def test_vgg2enc_job(lib, E, Cc, Dp):
    run_single(lib, vgg_job, E, Cc, Dp)


@pytest.mark.parametrize("N", (1, 255, 256, 257, 1024))
def test_copy32_job(lib, N):
    run_single(lib, copy_job, N)


@pytest.mark.parametrize("N,K,ldt", ((64, 64, 64), (37, 64, 40), (130, 72, 136), (33, 50, 40), (5, 3, 8), (200, 128, 200)))
def test_linear_job(lib, N, K, ldt):
    """full aligned tiles, a padded transpose, a ragged last tile column behind an aligned one, rows that are no multiple of four floats"""
    run_single(lib, linear_job, N, K, ldt)


# ---------------------------------------------------------------- job lists
def mixed_list(flat):
    """masr_bind's order: convs, vgg2enc, an odim-like Linear with a padded transpose, Linears of several tile counts, and per decoder layer the
    query Linear, the key|value Linear into its column block of the shared [K][NK] transpose, and the copy of the biases"""
    E, NK = 64, 2 * 128 + 8                                    # two layers' 2E columns and eight columns nobody writes
    outs, jobs = {}, []

    def take(name, made):
        jobs.append(made[0])
        outs.update({name + "." + k: v for k, v in made[1].items()})

    take("conv0", conv_job(flat, 1, 8, 3, gap=1))
    take("conv1", conv_job(flat, 2, 64, 64))
    take("conv2", conv_job(flat, 3, 5, 7, gap=2))
    take("v2e", vgg_job(flat, 4, 70, 6, 11))
    take("odim", linear_job(flat, 5, 37, E, 40, gap=3))
    take("lin0", linear_job(flat, 6, 64, 64, 64))
    take("lin1", linear_job(flat, 7, 130, 72, 136, gap=2))
    take("lin2", linear_job(flat, 8, 33, 50, 40))
    outs["kvT"] = kvT = Out(E * NK)
    for layer in range(2):
        take(f"q{layer}", linear_job(flat, 10 + layer, E, E, E, gap=layer))
        take(f"kv{layer}", linear_job(flat, 20 + layer, 2 * E, E, NK, gap=1, t16=kvT, t16_at=layer * 2 * E))
        take(f"kvb{layer}", copy_job(flat, 30 + layer, 2 * E))
    return jobs, outs


def test_mixed_list_layout():
    """(no launch) the list holds every type and its Linear sources sit at every residue mod 4"""
    jobs, _ = mixed_list(Flat())
    assert {j[0][1] for j in jobs} == {LINEAR, CONV, VGG2ENC, COPY32} and 10 <= len(jobs) <= JOBS_MAX
    assert {j[0][0] % 4 for j in jobs if j[0][1] == LINEAR} == {0, 1, 2, 3}


def test_mixed_job_list(lib):
    flat = Flat()
    jobs, outs = mixed_list(flat)
    launch(lib, flat.device(), jobs)
    all_ok(outs, "mixed list")


def test_full_job_list(lib):
    """exactly SHADOW_JOBS_MAX single-workgroup jobs: the search over tile_start reaches its last index; one more job is refused"""
    flat, jobs, outs = Flat(), [], {}
    for i in range(JOBS_MAX + 1):
        made = (linear_job(flat, i, 8, 8, 8, gap=i % 3), conv_job(flat, i, 2, 2), vgg_job(flat, i, 4, 2, 3, gap=1), copy_job(flat, i, 1 + i))[i % 4]
        jobs.append(made[0])
        if i < JOBS_MAX:
            outs.update({f"job{i}.{k}": v for k, v in made[1].items()})
        else:
            extra = made[1]
    P = flat.device()
    launch(lib, P, jobs, expect_rc=-1)
    assert "n_jobs outside" in lib.masr_last_error().decode()
    assert all(o.clean() for o in list(outs.values()) + list(extra.values()))
    launch(lib, P, jobs[:JOBS_MAX])
    all_ok(outs, "full list")
    assert all(o.clean() for o in extra.values())


def test_shadow_jobs_refusals(lib):
    flat = Flat()
    (dl, pl), ol = linear_job(flat, 1, 8, 8, 8)
    (dc, pc), oc = conv_job(flat, 2, 2, 2)
    (dv, pv), ov = vgg_job(flat, 3, 4, 2, 3)
    (dy, py), oy = copy_job(flat, 4, 5)
    P = flat.device()

    def edit(d, i, v):
        return tuple(v if k == i else x for k, x in enumerate(d))

    cases = (
        ([], "n_jobs outside"),
        ([(edit(dl, 0, 3), pl)], "src >= 4"), ([(edit(dl, 4, 7), pl)], "ldt >= N"), ([(edit(dl, 2, 0), pl)], "N"), ([(edit(dl, 3, 0), pl)], "K"),
        ([(edit(dl, 0, -4), pl)], "negative src"), ([(edit(dl, 1, 4), pl)], "type"), ([(edit(dl, 1, -1), pl)], "type"),
        ([(dl, (0, pl[1]))], "null output"), ([(dl, (pl[0], 0))], "null output"),
        ([(edit(dc, 2, -1), pc)], "N"), ([(edit(dc, 3, 0), pc)], "K"), ([(dc, (pc[0], 0))], "null output"),
        ([(edit(dv, 5, 0), pv)], "a0 / a1"), ([(edit(dv, 6, 0), pv)], "a0 / a1"), ([(edit(dv, 2, 0), pv)], "N"), ([(dv, (0, pv[1]))], "null output"),
        ([(edit(dy, 2, 0), py)], "N"), ([(dy, (0, 0))], "null output"),
        ([(dy, py), (edit(dl, 4, 7), pl)], "ldt >= N"),          # a bad job behind a good one: nothing of the list runs
    )
    outs = {**ol, **oc, **ov, **oy}
    for jobs, fragment in cases:
        if jobs:
            launch(lib, P, jobs, expect_rc=-1)
        else:
            one = (C.c_void_p * 2)(pl[0], pl[1])
            d = np.array(dl, np.int64)
            assert lib.masr_test_shadow_jobs(C.c_void_p(P.data_ptr()), 0, d.ctypes.data_as(C.c_void_p), one, S()) == -1
        assert fragment in lib.masr_last_error().decode(), (fragment, lib.masr_last_error().decode())
    one = (C.c_void_p * 2)(pl[0], pl[1])
    d = np.array(dl, np.int64)
    assert lib.masr_test_shadow_jobs(C.c_void_p(P.data_ptr() + 4), 1, d.ctypes.data_as(C.c_void_p), one, S()) == -1
    assert "16-byte" in lib.masr_last_error().decode()
    assert lib.masr_test_shadow_jobs(None, 1, d.ctypes.data_as(C.c_void_p), one, S()) == -1
    torch.cuda.synchronize()
    assert all(o.clean() for o in outs.values())
    launch(lib, P, [(dy, (py[0], 0))])                         # (a copy's second output is not used: null is fine)
    all_ok(oy, "copy with a null second output")


# ---------------------------------------------------------------- the BLSTM engine's passes
@pytest.mark.parametrize("R,Cc,ldy", ((1, 1, 8), (31, 33, 32), (32, 32, 32), (367, 64, 368), (70, 100, 72)))
def test_transpose_cast(lib, R, Cc, ldy):
    x = rnd(R * 1000 + Cc, R, Cc)
    xd = torch.from_numpy(x).to(DEV)
    y = Out(Cc * ldy)
    y.expect(0, bits16(x.T), pitch=ldy)                        # the pads R .. ldy of every row keep the marker
    _cabi.check(lib.masr_test_transpose_cast_bf16(C.c_void_p(xd.data_ptr()), C.c_void_p(y.ptr()), R, Cc, ldy, S()), "transpose_cast")
    all_ok({"y": y}, (R, Cc, ldy))
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("n", FLAT_NS)
def test_cast_bf16(lib, n):
    x = rnd(n, n + 1)
    x[n] = np.nan                                              # behind the n elements: never to be cast
    xd = torch.from_numpy(x).to(DEV)
    y = Out(n)
    y.expect(0, bits16(x[:n]))
    _cabi.check(lib.masr_test_cast_bf16(C.c_void_p(xd.data_ptr()), C.c_void_p(y.ptr()), n, S()), "cast_bf16")
    all_ok({"y": y}, n)


@pytest.mark.parametrize("CO,CI", ((64, 64), (8, 3), (5, 7)))
def test_conv_weight_shadows(lib, CO, CI):
    """the BLSTM form == the refresh's conv job == the reference, bit for bit; wd may be left out"""
    flat = Flat()
    j, outs = conv_job(flat, 9, CO, CI, gap=1)
    P = flat.device()
    launch(lib, P, [j])
    all_ok(outs, "conv job")
    w = C.c_void_p(P.data_ptr() + 4 * j[0][0])
    n = CO * CI * 9
    wk, wd, wk_only = Out(n), Out(n), Out(n)
    _cabi.check(lib.masr_test_conv_weight_shadows(w, C.c_void_p(wk.ptr()), C.c_void_p(wd.ptr()), CO, CI, S()), "conv_weight_shadows")
    _cabi.check(lib.masr_test_conv_weight_shadows(w, C.c_void_p(wk_only.ptr()), None, CO, CI, S()), "conv_weight_shadows, no wd")
    assert torch.equal(wk.t, outs["wk"].t) and torch.equal(wd.t, outs["wd"].t) and torch.equal(wk_only.t, outs["wk"].t)


def test_blstm_shadow_refusals(lib):
    xd = torch.from_numpy(rnd(1, 64)).to(DEV)
    y = Out(64)
    x, yp = C.c_void_p(xd.data_ptr()), C.c_void_p(y.ptr())
    calls = ((lambda: lib.masr_test_transpose_cast_bf16(x, yp, 0, 4, 8, S()), "R, C >= 1"),
             (lambda: lib.masr_test_transpose_cast_bf16(x, yp, 4, 0, 8, S()), "R, C >= 1"),
             (lambda: lib.masr_test_transpose_cast_bf16(x, yp, 8, 4, 7, S()), "ldy >= R"),
             (lambda: lib.masr_test_transpose_cast_bf16(None, yp, 4, 4, 8, S()), "null"),
             (lambda: lib.masr_test_cast_bf16(x, yp, 0, S()), "n outside"),
             (lambda: lib.masr_test_cast_bf16(x, None, 8, S()), "null"),
             (lambda: lib.masr_test_conv_weight_shadows(x, yp, None, 0, 2, S()), "CO, CI >= 1"),
             (lambda: lib.masr_test_conv_weight_shadows(x, yp, None, 2, -1, S()), "CO, CI >= 1"),
             (lambda: lib.masr_test_conv_weight_shadows(x, None, yp, 2, 2, S()), "null"))
    for call, fragment in calls:
        assert call() == -1
        assert fragment in lib.masr_last_error().decode(), fragment
    torch.cuda.synchronize()
    assert y.clean()
