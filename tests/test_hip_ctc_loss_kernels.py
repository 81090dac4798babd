"""The CTC loss kernels of csrc/ctc.hip alone (ctc_lse_kernel, ctc_sweep_kernel, ctc_grad_kernel<float | bf16>, ctc_mean_kernel,
ctc_mix_kernel) against the float64 lattice of tests/ctc_loss_ref.py, whose cases these are (pinned on the CPU by
tests/test_ctc_loss_ref_cpu.py, feasibility of every utterance included).

Accuracy (masr_ctc_loss, time-major): the wide lattice (S = 257, 601, 255, 513 and an infeasible 601) at logit scale 1 and 8, the lattice
limit S = 2047, the vocabulary tail (C = 2 .. 4096), utterances of 1 .. 13 frames around the sweep's prefetch ring with the empty target and
in_len == tgt_len, and a blank that is not class 0.  nll and the mean within 2e-5 max(1, |ref|); a gradient element within 2e-6 + 2e-3 |g64|
or within 4 E32, E32 the largest error of torch's fp32 CPU CTCLoss gradient on the same case; padded rows, infeasible utterances and the
sentinels exactly.  Bit for bit: the batch-first layout against the time-major one, a work buffer wider than needed, repeated launches, and
the joint form's bf16 gradient against the fp32 gradient times the weight rounded to nearest even (common.h's bf16 is the compiler's
__bf16, whose conversion from float rounds to nearest even as torch's does).  Every output starts as a NaN sentinel and the work buffer as
NaNs too: the launch may rely on nothing it did not write.  The figures of each case are printed (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402
import ctc_loss_ref as R  # noqa: E402

DEV = "cuda:0"
MARK = 0x7FC5A5A5                                              # a NaN as a float
MARK16 = 0x7FA5                                                # a NaN as a bf16
KEYS = ([("wide", 1), ("wide", 8), ("limit", 0)] + [("vocab", c) for c in R.VOCAB_CS] + [("short", 0), ("short", 8), ("short", 4)])
ID = lambda k: f"{k[0]}-{k[1]}"  # noqa: E731


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def marked(*shape):
    return torch.full(shape, MARK, dtype=torch.int32, device=DEV)


def f32(t):
    return t.cpu().numpy().view(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def is_mark(a):
    return np.ascontiguousarray(a).view(np.int32) == MARK


@functools.lru_cache(maxsize=None)
def case(key):
    kind, arg = key
    return {"wide": R.case_wide, "limit": lambda _: R.case_limit(), "vocab": R.case_vocab, "short": R.case_short}[kind](arg)


@functools.lru_cache(maxsize=None)
def ref64(key):
    c = case(key)
    return R.ctc_loss(c.logits, c.targets, c.tgt_off, c.in_len, c.tgt_len, c.blank)


@functools.lru_cache(maxsize=None)
def torch32_grad(key):
    c = case(key)
    z = torch.from_numpy(c.logits).requires_grad_(True)
    loss = torch.nn.CTCLoss(blank=c.blank, reduction="mean", zero_infinity=True)(
        torch.log_softmax(z, -1), torch.from_numpy(R.concatenated(c)), torch.from_numpy(c.in_len.astype(np.int64)),
        torch.from_numpy(c.tgt_len.astype(np.int64)))
    loss.backward()
    return z.grad.numpy()


def tight(c):
    return 2 * int(c.tgt_len.max()) + 1


class Call:
    """the device buffers of one masr_ctc_loss / masr_test_ctc_loss_layout call on a case; run() launches and reads everything back"""

    def __init__(self, c, maxS=None, batch_first=None):
        self.c, self.bf = c, batch_first
        self.T, self.B, self.C = c.logits.shape
        self.maxS = tight(c) if maxS is None else maxS
        self.L = _cabi.lib()
        self.logits = dev(c.logits.transpose(1, 0, 2) if batch_first else c.logits)
        self.tgt, self.off, self.il, self.tl = dev(c.targets), dev(c.tgt_off), dev(c.in_len), dev(c.tgt_len)
        self.work = marked(int(self.L.masr_ctc_work_floats(self.T, self.B, self.maxS)))
        self.nll, self.loss = marked(self.B), marked(1)
        self.grad = marked(self.B, self.T, self.C) if batch_first else marked(self.T, self.B, self.C)

    def launch(self):
        a = (P(self.logits), P(self.tgt), P(self.off), P(self.il), P(self.tl), self.T, self.B, self.C, self.c.blank, P(self.nll), P(self.loss),
             P(self.grad), P(self.work), self.maxS, S())
        return self.L.masr_ctc_loss(*a) if self.bf is None else self.L.masr_test_ctc_loss_layout(*a, int(self.bf))

    def run(self):
        _cabi.check(self.launch(), "ctc loss")
        self.status = self.L.masr_ctc_status(P(self.work), self.T, self.B, self.maxS, S())
        return f32(self.nll), f32(self.loss), f32(self.grad)


@functools.lru_cache(maxsize=None)
def public(key):
    """(nll [B], loss [1], grad [T][B][C], status) of masr_ctc_loss with the tight maxS"""
    k = Call(case(key))
    return (*k.run(), k.status)


@functools.lru_cache(maxsize=None)
def batch_first(key):
    """(nll, loss, grad [B][T][C], status) of masr_test_ctc_loss_layout with batch_first = 1 on the transposed logits"""
    k = Call(case(key), batch_first=1)
    return (*k.run(), k.status)


def check_structure(c, nll, loss, grad_tm, status):
    assert status == 0
    assert not is_mark(nll).any() and not is_mark(loss).any() and not is_mark(grad_tm).any(), "an output word was not written"
    for b, ok in enumerate(c.feasible):
        n = int(c.in_len[b])
        assert not grad_tm[n:, b].any(), f"utterance {b}: a gradient row at t >= in_len is not zero"
        if not ok:
            assert nll[b] == 0.0 and not grad_tm[:, b].any(), f"infeasible utterance {b}: nll or gradient not zero"
        else:
            assert np.isfinite(nll[b]) and (n == 0 or grad_tm[:n, b].any())
    assert np.isfinite(grad_tm).all()


def check_accuracy(key):
    c, r = case(key), ref64(key)
    nll, loss, grad, status = public(key)
    check_structure(c, nll, loss, grad, status)
    nerr = np.abs(nll.astype(np.float64) - r.nll) / np.maximum(1.0, np.abs(r.nll))
    lerr = abs(float(loss[0]) - r.loss) / max(1.0, abs(r.loss))
    e = np.abs(grad.astype(np.float64) - r.grad)
    E32 = float(np.abs(torch32_grad(key).astype(np.float64) - r.grad).max())
    first = e <= 2e-6 + 2e-3 * np.abs(r.grad)
    ok = first | (e <= 4.0 * E32)
    print(f"\n{c.name}: nll err {nerr.max():.2e} loss err {lerr:.2e} | grad: kernel max err {e.max():.3e}  E32 {E32:.3e}  max|g64| {np.abs(r.grad).max():.3e}"
          f"  needed 4 E32: {np.mean(~first):.2e} of the elements  worst err / allowed {np.max(e / np.maximum(2e-6 + 2e-3 * np.abs(r.grad), 4.0 * E32)):.3f}")
    assert nerr.max() <= 2e-5, (nll, r.nll)
    assert lerr <= 2e-5, (float(loss[0]), r.loss)
    assert ok.all(), f"{int((~ok).sum())} gradient elements outside both bounds; worst {float(e[~ok].max()):.3e} against 4 E32 = {4 * E32:.3e}"


@pytest.mark.parametrize("scale", [1, 8])
def test_wide_lattice(scale):
    """S = 257, 601, 513 take the strided alpha and beta loops of ctc_sweep_kernel (S > 256), S = 255 the last narrow width beside them, the
    fifth utterance is wide and infeasible.  Scale 8 makes the posteriors peaked: most of them underflow.
    Measured on an MI355X (kernel max err / E32 / max|g64| / share needing the 4 E32 clause):
    scale 1: 2.08e-6 / 1.48e-6 / 1.47e-3 / 0        (nll err 5.1e-7 of the 2e-5 allowed; worst element at 0.35 of its bound)
    scale 8: 4.59e-6 / 4.15e-6 / 1.58e-3 / 2.2e-3   (nll err 1.2e-6; worst element at 0.28 of its bound)"""
    check_accuracy(("wide", scale))


def test_lattice_limit():
    """S = 2047 = the widest lattice a call can hold (maxS 2047: eight strides of the wide loops, row[2][2048] of LDS, post[2048]); maxS = 2049
    is refused on the host before any launch.
    Measured on an MI355X (kernel max err / E32 / max|g64| / share needing the 4 E32 clause):
    3.15e-6 / 3.54e-6 / 9.76e-4 / 0   (nll err 8.3e-7; worst element at 0.22 of its bound)"""
    check_accuracy(("limit", 0))
    k = Call(case(("limit", 0)), maxS=2049)
    assert k.launch() == -1 and b"2048" in k.L.masr_last_error()
    torch.cuda.synchronize()
    assert is_mark(f32(k.nll)).all() and is_mark(f32(k.loss)).all() and is_mark(f32(k.grad)).all() and is_mark(f32(k.work)).all()


@pytest.mark.parametrize("Cn", R.VOCAB_CS)
def test_vocabulary_tail(Cn):
    """ctc_lse_kernel keeps classes below 512 in eight registers per lane (C = 2, 63, 64, 65: the lane edges; 512: all eight full) and re-reads
    the classes from 512 on in a second loop (513: one lane, 577: a ragged second pass, 4096: the launcher's limit and all of acc[4096]); class
    C - 1 is a target, so a wrong normaliser or a missed tail class shows in nll and gradient.
    Measured on an MI355X (kernel max err / E32 / max|g64| / share needing the 4 E32 clause):
    C 2: 6.7e-7 / 9.6e-7, C 63: 1.28e-6 / 1.55e-6, C 64: 1.71e-6 / 1.28e-6, C 65: 1.26e-6 / 5.2e-7, C 512: 1.29e-6 / 1.04e-6,
    C 513: 1.29e-6 / 8.8e-7, C 577: 1.27e-6 / 1.57e-6, C 4096: 1.29e-6 / 1.27e-6; max|g64| 0.333 and share 0 in all of them (the largest
    errors sit on elements near 1/3, inside 2e-3 |g64|; C = 2 has the worst element, at 0.14 of its bound); nll err <= 1.4e-7"""
    check_accuracy(("vocab", Cn))


@pytest.mark.parametrize("blank", [0, 8, 4])
def test_short_inputs_and_blank(blank):
    """in_len 1, 2, 5, 6, 7, 8, 12, 13 around the PF = 6 prefetch ring of the narrow sweep (the ring is filled past the utterance's end, the
    loop breaks mid-unroll at every residue), the empty target (S = 1), in_len == tgt_len = 3 with distinct labels (one path) and with a
    repeat (none); the same with the blank as the last class and as a class in the middle.
    Measured on an MI355X (kernel max err / E32 / max|g64| / share needing the 4 E32 clause):
    blank 0: 1.49e-7 / 1.79e-7 / 9.0e-2 / 0, blank 8: 3.52e-7 / 2.60e-7 / 9.6e-2 / 0, blank 4: 8.9e-8 / 1.25e-7 / 9.4e-2 / 0
    (nll err <= 1.5e-7; worst element at 0.005 of its bound)"""
    check_accuracy(("short", blank))


LAYOUT_KEYS = [("wide", 1), ("wide", 8), ("vocab", 513), ("short", 0), ("short", 4)]


@pytest.mark.parametrize("key", LAYOUT_KEYS, ids=ID)
def test_batch_first_layout_same_bits(key):
    """what blstm.hip calls: logits and gradient [B][T][C].  Only addresses differ, so nll and loss have the same bits and
    grad_bf[b][t] == grad[t][b] bit for bit"""
    nll, loss, grad, status = public(key)
    nll_b, loss_b, grad_b, status_b = batch_first(key)
    assert status_b == 0 and not is_mark(grad_b).any()
    assert same_bits(nll, nll_b) and same_bits(loss, loss_b)
    assert same_bits(grad, grad_b.transpose(1, 0, 2))


@pytest.mark.parametrize("key", [("short", 0), ("wide", 1)], ids=ID)
def test_wider_work_buffer_same_bits(key):
    """maxS 37 above the need (unaligned: Spad rounds up to a multiple of four) moves every parked row, the normalisers, the
    log-likelihoods and the status word inside the work buffer, and nothing else"""
    c = case(key)
    nll, loss, grad, _ = public(key)
    k = Call(c, maxS=tight(c) + 37)
    nll_w, loss_w, grad_w = k.run()
    assert k.status == 0
    assert same_bits(nll, nll_w) and same_bits(loss, loss_w) and same_bits(grad, grad_w)


def test_repeat_launches_same_bits():
    """the alpha and the beta workgroup of an utterance run side by side and every class sum has one owner: three launches on the same
    buffers (the second and third over the first's results) give the same bits"""
    k = Call(case(("wide", 1)))
    outs = [k.run() for _ in range(3)]
    assert k.status == 0
    for o in outs[1:]:
        assert all(same_bits(a, b) for a, b in zip(outs[0], o))
    assert all(same_bits(a, b) for a, b in zip(outs[0], public(("wide", 1))[:3]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the joint form
class Joint:
    """the device buffers of one masr_test_ctc_loss_joint call on a case: batch-first logits with ld the next multiple of 8 above C and large
    finite garbage in the pad columns, targets as a padded [B][Lmax] array with tgt_off = b * Lmax (the engine's gold array)"""

    def __init__(self, c, with_grad=True):
        assert c.blank == 0
        self.c = c
        self.T, self.B, self.C = c.logits.shape
        self.ld = (self.C // 8 + 1) * 8
        self.maxS = tight(c)
        self.L = _cabi.lib()
        z = np.empty((self.B, self.T, self.ld), np.float32)
        z[:, :, :self.C] = c.logits.transpose(1, 0, 2)
        rng = np.random.default_rng(5)
        z[:, :, self.C:] = np.where(rng.random((self.B, self.T, self.ld - self.C)) < 0.5, -1.0, 1.0) * 1e30
        tg, off, _ = R.padded(c)
        self.logits, self.tgt, self.off, self.il, self.tl = dev(z), dev(tg), dev(off), dev(c.in_len), dev(c.tgt_len)
        self.work = marked(int(self.L.masr_ctc_work_floats(self.T, self.B, self.maxS)))
        self.nll = marked(self.B)
        self.stats = marked(4)
        self.grad16 = torch.full((self.B, self.T, self.ld), MARK16, dtype=torch.int16, device=DEV)
        self.with_grad = with_grad

    def launch(self, w, **over):
        """over: T, C, ld, maxS or a device array to pass instead of the case's"""
        self.stats[0] = int(np.float32(2.5).view(np.int32))    # the decoder's CE on entry
        g = lambda n: over.get(n, getattr(self, n))  # noqa: E731
        return self.L.masr_test_ctc_loss_joint(P(self.logits), g("ld"), P(g("tgt")), P(self.off), P(g("il")), P(g("tl")), g("T"), self.B, g("C"),
                                               P(self.nll), P(self.grad16) if self.with_grad else None, w, P(self.stats), P(self.work), g("maxS"), S())

    def untouched(self):
        st = self.stats.cpu().numpy()
        return (is_mark(f32(self.nll)).all() and st[0] == np.float32(2.5).view(np.int32) and (st[1:] == MARK).all() and
                bool((self.grad16 == MARK16).all()))


@pytest.mark.parametrize("w", [0.3, 1.0])
@pytest.mark.parametrize("key", [("wide", 1), ("wide", 8), ("vocab", 65), ("vocab", 513), ("short", 0)], ids=ID)
def test_joint_form(key, w):
    """mk_ctc_loss_joint as train.hip calls it: the row stride ld > C (no pad column may be read: they hold +-1e30), ctc_grad_kernel<bf16> =
    the fp32 instantiation's arithmetic, one more multiply by w and one rounding to bf16, pad columns zero on every kind of row,
    ctc_mix_kernel's (1 - w) CE + w CTC (four fp32 roundings, at most 4 ulp = 5e-7 relative: 1e-6 allowed, 7e-9 .. 9.5e-8 measured on an
    MI355X), and the forward-only call"""
    c = case(key)
    nll_b, _, grad_b, _ = batch_first(key)
    j = Joint(c)
    _cabi.check(j.launch(w), "joint ctc")
    nll, stats = f32(j.nll), j.stats.cpu().numpy()
    g16 = j.grad16.cpu().numpy()
    assert same_bits(nll, nll_b)
    want = torch.from_numpy(grad_b * np.float32(w)).to(torch.bfloat16).view(torch.int16).numpy()
    assert not (g16 == np.int16(MARK16)).any(), "a bf16 gradient word was not written"
    assert np.array_equal(g16[:, :, :j.C], want), f"{int((g16[:, :, :j.C] != want).sum())} bf16 gradient words differ"
    assert not g16[:, :, j.C:].any(), "a pad column of the gradient is not zero"
    for b, ok in enumerate(c.feasible):                        # (the zero rows are zero in bf16 too, pads included)
        assert not g16[b, int(c.in_len[b]):].any() and (ok or not g16[b].any())
    assert (stats[1:] == MARK).all()
    w32 = float(np.float32(w))
    mean = float(np.mean(nll.astype(np.float64) / np.maximum(c.tgt_len.astype(np.float64), 1.0)))
    expect = (1.0 - w32) * 2.5 + w32 * mean
    got = float(stats[:1].view(np.float32)[0])
    print(f"\n{c.name} w {w}: stats[0] {got!r} expected {expect!r} rel {abs(got - expect) / abs(expect):.2e}")
    assert abs(got - expect) <= 1e-6 * abs(expect)
    # forward only: the same nll and stats bits, no gradient written
    f = Joint(c, with_grad=False)
    _cabi.check(f.launch(w), "joint ctc, forward only")
    assert same_bits(f32(f.nll), nll) and f.stats.cpu().numpy()[0] == stats[0]
    assert bool((f.grad16 == MARK16).all())


def test_joint_entry_refusals():
    """the entry vets what the kernels would index with (this path has no status word): -1 with a message before any launch, nothing written"""
    c = case(("short", 0))
    j = Joint(c)
    tg, _, Lmax = R.padded(c)
    assert Lmax == 3 and j.ld == 16 and j.maxS == 7

    def refused(what, **over):
        rc = j.launch(0.3, **over)
        msg = j.L.masr_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and msg, what
        assert j.untouched(), what
        return msg

    il = c.in_len.copy(); il[3] = j.T + 1
    assert "in_len" in refused("in_len > T", il=dev(il))
    il[3] = -1
    assert "in_len" in refused("in_len < 0", il=dev(il))
    tl = c.tgt_len.copy(); tl[7] = 4                           # 2 * 4 + 1 = 9 > maxS = 7 (the padded row has 3 columns: the entry must stop before reading it)
    assert "maxS" in refused("target wider than maxS", tl=dev(tl))
    assert "maxS" in refused("maxS below the widest target", maxS=5)
    for bad in (0, j.C):                                       # (C itself is a pad column of the row: in bounds even if it were read)
        t2 = tg.copy().reshape(j.B, Lmax); t2[6, 1] = bad
        assert "target id" in refused(f"target id {bad}", tgt=dev(t2.reshape(-1)))
    refused("ld < C", ld=8)
    refused("ld % 8 != 0 with a gradient", ld=12)
    # the same buffers, unchanged arguments: accepted
    _cabi.check(j.launch(0.3), "joint ctc")
    assert not j.untouched()
