"""masr_ctc_align alone (include/masr.h, DESIGN 5.9: ctc_align_frames + ctc_align_sweep) against the restatements of tests/ctc_align_ref.py.

Logits are normal * 3 rounded to multiples of 0.5: the max-shifted emissions and every sum of them are then exact in fp32, ties between
paths are common, and the tie rule decides them.  Padded frames and the columns in [C, ld) are NaN; outputs sit between guard words and
start as junk, like the work buffer, so a position the kernels leave unwritten or write outside shows.

frames / start / end must equal align_f32's bit for bit.  The score is compared with the fp64 log-probability lp of the SAME path:
  |score - lp| <= 2^-24 (n + 2) M + sum over t < n of eps_t                                                  (ctc_align_ref.score_bound)
M = the largest partial sum in magnitude the fp64 recursion sees (viterbi_f64).  Derivation: score = fl(v - acc).  v is n - 1 fp32 additions
of emissions that are multiples of 0.5 below 2^23: exact.  acc is n additions of the lsum_t, the subtraction is one more; each rounds by at
most half an ulp = 2^-24 of its result, a partial sum of magnitude <= M; n + 1 roundings, n + 2 in the bound.  eps_t is the error of the
device's fp32 log-sum against the exact one, bounded from the formats in ctc_align_ref.lse_err_bound.  The returned path's lp must reach
the fp64 optimum less 2 n 2^-24 M: the rounding of n additions on either path.  Each test prints the worst fraction of the bound it saw."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_align_ref as ar  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402

DEV = "cuda:0"
GUARD, MARK = 16, 0x5A5A5A5A


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, dtype):
    """a device buffer of n words between two runs of GUARD marked words -> (whole buffer as int32, the view of the n words)"""
    buf = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int32, device=DEV)
    buf[GUARD:GUARD + n] = 0x7F7F7F7F
    return buf, buf[GUARD:GUARD + n].view(dtype)


def flat_targets(ys):
    tl = np.asarray([len(y) for y in ys], np.int32)
    off = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int32)
    return np.asarray([t for y in ys for t in y] or [0], np.int32), off, tl


def run(z, lens, tgt, off, tl, Cn, blank, maxL, junk=0x7F):
    """z [B, Tp, ld] fp32 numpy; lens, tgt, off, tl int32 numpy -> frames [B, Tp], start / end [B, maxL], score [B] numpy"""
    B, Tp, ld = z.shape
    l = lib()
    d = lambda a, t=np.int32: torch.from_numpy(np.ascontiguousarray(a, t)).to(DEV)
    zd, ld_, tg, of, tld = d(z, np.float32), d(lens), d(tgt), d(off), d(tl)
    nb = int(l.masr_ctc_align_work_bytes(B, Tp, maxL))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), junk, dtype=torch.uint8, device=DEV)
    bufs = [guarded(B * Tp, torch.int32), guarded(B * maxL, torch.int32), guarded(B * maxL, torch.int32), guarded(B, torch.float32)]
    rc = l.masr_ctc_align(p(zd), ld, p(ld_), p(tg), p(of), p(tld), B, Tp, Cn, blank, maxL, p(work), nb, *[p(v) for _, v in bufs], stream())
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    for whole, _ in bufs:
        g = whole.cpu().numpy()
        assert (g[:GUARD] == MARK).all() and (g[-GUARD:] == MARK).all(), "a guard word was written"
    fr, st, en, sc = (v.cpu().numpy() for _, v in bufs)
    return fr.reshape(B, Tp), st.reshape(B, maxL), en.reshape(B, maxL), sc


def align(z, lens, ys, Cn, blank=0, maxL=None, **kw):
    tgt, off, tl = flat_targets(ys)
    return run(z, np.asarray(lens, np.int32), tgt, off, tl, Cn, blank, int(tl.max()) if maxL is None else maxL, **kw)


def grid_logits(rng, B, Tp, Cn, ld, lens):
    z = np.full((B, Tp, ld), np.nan, np.float32)
    z[..., :Cn] = np.round(rng.standard_normal((B, Tp, Cn)) * 3 * 2) / 2
    for b, n in enumerate(lens):
        z[b, max(int(n), 0):] = np.nan
    return z


def check(name, z, lens, ys, Cn, blank, out, maxL=None, refs=None):
    """every utterance's frames / start / end / score against the restatement and the fp64 references -> the restatement's results"""
    fr, st, en, sc = out
    B, Tp = fr.shape
    maxL = st.shape[1] if maxL is None else maxL
    worst = worst_opt = 0.0
    refs = refs or [ar.align_f32(z[b, :, :Cn], lens[b], ys[b], blank, Tp, maxL) for b in range(B)]
    for b, r in enumerate(refs):
        n = min(max(int(lens[b]), 0), Tp)
        assert np.array_equal(fr[b], r["frames"]), (name, b, fr[b], r["frames"])
        assert np.array_equal(st[b], r["start"]) and np.array_equal(en[b], r["end"]), (name, b, st[b], r["start"], en[b], r["end"])
        if r["states"] is None:
            assert np.isnan(sc[b]) if np.isnan(r["score"]) else np.isneginf(sc[b]), (name, b, sc[b])
            assert (fr[b] == -2).all() and (st[b] == -1).all() and (en[b] == -1).all()
            continue
        assert ar.collapse(fr[b], ys[b]) == list(ys[b]) and all(en[b, i] > st[b, i] for i in range(len(ys[b]))), (name, b)
        lp, _ = ar.path_logprob_f64(z[b, :, :Cn], n, ys[b], blank, fr[b])
        best, M = ar.viterbi_f64(z[b, :, :Cn], n, ys[b], blank)
        bound = ar.score_bound(z[b, :, :Cn], n, M)
        err = abs(float(sc[b]) - lp)
        if n == 0:
            assert sc[b] == 0.0
            continue
        worst, worst_opt = max(worst, err / bound), max(worst_opt, (best - lp) / (2 * n * 2.0 ** -24 * M))
        assert err <= bound, (name, b, float(sc[b]), lp, bound)
        assert lp >= best - 2 * n * 2.0 ** -24 * M, (name, b, lp, best)
    print(f"{name}: worst |score - lp| / bound = {worst:.3f}, worst (optimum - lp) / allowance = {worst_opt:.3g}")
    return refs


# B = 6, Tp = 24, C = 9, ld = 12, maxL = 12: a plain one, no tokens, no tokens and no frames, the unique path (5 distinct tokens in 5 frames),
# infeasible (7 tokens and three adjacent repeats need 10 frames, it has 9), 11 tokens with repeats
SMALL_LENS = [24, 17, 0, 5, 9, 24]
SMALL_YS = [[3, 1, 4, 1, 5], [], [], [2, 7, 1, 8, 3], [1, 1, 2, 2, 3, 3, 4], [1, 2, 2, 3, 4, 4, 5, 6, 7, 8, 8]]


@pytest.fixture(scope="module")
def small():
    z = grid_logits(np.random.default_rng(0), 6, 24, 9, 12, SMALL_LENS)
    refs = [ar.align_f32(z[b, :, :9], SMALL_LENS[b], SMALL_YS[b], 0, 24, 12) for b in range(6)]
    return z, refs


def test_small(small):
    z, refs = small
    out = align(z, SMALL_LENS, SMALL_YS, 9, maxL=12)
    check("small", z, SMALL_LENS, SMALL_YS, 9, 0, out, refs=refs)
    assert np.isneginf(out[3][4]) and out[3][2] == 0.0 and refs[3]["states"] == [1, 3, 5, 7, 9]
    assert (out[0][1, :17] == -1).all()                          # no tokens: every frame blank


def test_all_zero_logits_the_tie_rule_alone():
    z = grid_logits(np.random.default_rng(0), 6, 24, 9, 12, SMALL_LENS)
    z[..., :9] = np.where(np.isnan(z[..., :9]), np.nan, 0.0)
    out = align(z, SMALL_LENS, SMALL_YS, 9, maxL=12)
    refs = check("zeros", z, SMALL_LENS, SMALL_YS, 9, 0, out)
    # the end prefers the last blank and every step back the smaller back-pointer, so the path stays in the last blank for as long as that
    # state can be reached: the tokens sit as early as they can
    assert refs[0]["states"][-1] == 10 and out[1][0, 4] == 4 and out[2][0, 4] == 5


def blank_in_the_middle(z, ys):
    z2 = z.copy()
    z2[..., [0, 2]] = z[..., [2, 0]]
    return z2, [[{2: 0}.get(t, t) for t in y] for y in ys]


def test_blank_not_class_0(small):
    z, _ = small
    ys = [[t for t in y] for y in SMALL_YS]
    z2, ys2 = blank_in_the_middle(z, ys)                         # class 2 becomes the blank, what was class 2 is class 0
    a = align(z, SMALL_LENS, ys, 9, maxL=12)
    b = align(z2, SMALL_LENS, ys2, 9, blank=2, maxL=12)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    # (the log-sum adds the classes in another order: the scores agree to its rounding, not bit for bit)
    assert np.array_equal(np.isfinite(a[3]), np.isfinite(b[3])) and np.allclose(a[3][np.isfinite(a[3])], b[3][np.isfinite(b[3])], rtol=0, atol=1e-4)


def test_wide_lattices():
    # S = 63, 65 (around one wave), 255 (one state per thread, the back-pointers in the work buffer) and 301 (more than one state per thread)
    rng = np.random.default_rng(1)
    B, Tp, Cn = 4, 330, 40
    lens = [330, 300, 330, 317]
    ys = [[int(t) for t in rng.integers(1, Cn, L)] for L in (31, 32, 127, 150)]
    ys[2][10:14] = [7, 7, 7, 9]                                  # adjacent repeats
    ys[0][3] = ys[0][2]
    z = grid_logits(rng, B, Tp, Cn, 48, lens)
    check("wide", z, lens, ys, Cn, 0, align(z, lens, ys, Cn))


def test_widest_lattice():
    # L = 1023: S = 2047, the bound, 8 states per thread; with repeats the 1100 frames are barely enough
    rng = np.random.default_rng(2)
    Tp, Cn, L = 1100, 40, 1023
    ys = [[int(t) for t in rng.integers(1, Cn, L)]]
    assert L + sum(a == b for a, b in zip(ys[0], ys[0][1:])) <= Tp
    z = grid_logits(rng, 1, Tp, Cn, 40, [Tp])
    check("widest", z, [Tp], ys, Cn, 0, align(z, [Tp], ys, Cn))


@pytest.mark.parametrize("what", ["blank token", "token >= C", "negative token", "tgt_len > maxL", "tgt_len < 0"])
def test_device_refusals(small, what):
    z, refs = small
    tgt, off, tl = flat_targets(SMALL_YS)
    good = run(z, np.asarray(SMALL_LENS, np.int32), tgt, off, tl, 9, 0, 12)
    tgt, tl = tgt.copy(), tl.copy()
    for victim in (0, 5):                                        # the first and the last utterance
        t2, l2 = tgt.copy(), tl.copy()
        if what == "blank token":
            t2[off[victim] + 2] = 0
        elif what == "token >= C":
            t2[off[victim] + len(SMALL_YS[victim]) - 1] = 9
        elif what == "negative token":
            t2[off[victim]] = -1
        elif what == "tgt_len > maxL":
            l2[victim] = 13
        else:
            l2[victim] = -1
        fr, st, en, sc = run(z, np.asarray(SMALL_LENS, np.int32), t2, off, l2, 9, 0, 12, junk=0xA5)
        assert np.isnan(sc[victim]) and (fr[victim] == -2).all() and (st[victim] == -1).all() and (en[victim] == -1).all(), (what, victim)
        for b in range(6):
            if b != victim:
                for x, y in zip(good, (fr, st, en, sc)):
                    assert np.array_equal(x[b].view(np.uint32), y[b].view(np.uint32)), (what, victim, b)


def test_length_clamps(small):
    z, _ = small
    z = np.nan_to_num(z, nan=0.0)
    lens = [-3, 1000, 24, 24, 24, 24]
    ys = [[], [1, 2], [1], [2], [3], [4]]
    fr, st, en, sc = align(z, lens, ys, 9, maxL=12)
    assert sc[0] == 0.0 and (fr[0] == -2).all() and np.isfinite(sc[1]) and (fr[1] != -2).all()


def test_host_refusals():
    l = lib()
    B, Tp, Cn, maxL = 2, 8, 6, 3
    z = torch.zeros(B, Tp, Cn, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    lens, tgt = torch.full((B,), Tp, **i32), torch.ones(6, **i32)
    off, tl = torch.tensor([0, 3], **i32), torch.tensor([3, 3], **i32)
    nb = int(l.masr_ctc_align_work_bytes(B, Tp, maxL))
    work = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    fr, st, en = torch.full((B, Tp), MARK, **i32), torch.full((B, maxL), MARK, **i32), torch.full((B, maxL), MARK, **i32)
    sc = torch.full((B,), 7.0, device=DEV)

    def call(**kw):
        a = dict(logits=p(z), ld=Cn, enc=p(lens), tgt=p(tgt), off=p(off), tl=p(tl), B=B, Tp=Tp, C=Cn, blank=0, maxL=maxL, work=p(work), wb=nb, fr=p(fr),
                 st=p(st), en=p(en), sc=p(sc))
        a.update(kw)
        return l.masr_ctc_align(a["logits"], a["ld"], a["enc"], a["tgt"], a["off"], a["tl"], a["B"], a["Tp"], a["C"], a["blank"], a["maxL"], a["work"],
                                a["wb"], a["fr"], a["st"], a["en"], a["sc"], None)

    bad = [(dict(B=0), "B >= 1"), (dict(Tp=0), "Tp >= 1"), (dict(C=1), "2 <= C <= 4096"), (dict(C=4097, ld=4097), "2 <= C <= 4096"),
           (dict(ld=Cn - 1), "ld >= C"), (dict(blank=-1), "blank must be in [0, C)"), (dict(blank=Cn), "blank must be in [0, C)"),
           (dict(maxL=-1), "maxL >= 0"), (dict(maxL=1024), "2 * maxL + 1 <= 2048"), (dict(wb=nb - 1), "work buffer too small")]
    bad += [(dict(**{k: None}), "null pointer") for k in ("logits", "enc", "tgt", "off", "tl", "work", "fr", "st", "en", "sc")]
    for kw, text in bad:
        assert call(**kw) == -1, kw
        assert text in l.masr_last_error().decode(), (kw, l.masr_last_error())
    torch.cuda.synchronize()
    assert (fr == MARK).all() and (st == MARK).all() and (en == MARK).all() and (sc == 7.0).all()      # nothing was launched
    assert l.masr_ctc_align_work_bytes(0, Tp, maxL) < 0 and l.masr_ctc_align_work_bytes(B, 0, maxL) < 0
    assert l.masr_ctc_align_work_bytes(B, Tp, -1) < 0 and l.masr_ctc_align_work_bytes(B, Tp, 1024) < 0
    assert l.masr_ctc_align_work_bytes(B, Tp, 1023) > 0 and l.masr_ctc_align_work_bytes(B, Tp, 0) > 0
    assert call() == 0 and call(maxL=3, wb=nb) == 0
    torch.cuda.synchronize()
    assert (fr != MARK).all() and torch.isfinite(sc).all()


def test_permuted_batch_bit_for_bit(small):
    z, _ = small
    perm = np.random.default_rng(5).permutation(6)
    a = align(z, SMALL_LENS, SMALL_YS, 9, maxL=12)
    b = align(np.ascontiguousarray(z[perm]), [SMALL_LENS[i] for i in perm], [SMALL_YS[i] for i in perm], 9, maxL=12, junk=0xA5)
    for x, y in zip(a, b):
        assert np.array_equal(x[perm].view(np.uint32), y.view(np.uint32))


def test_no_trace_hook_gives_the_same_scores(small):
    # include/masr_test.h masr_test_ctc_align_no_trace, the benchmark's leg: the same scores, nothing else written for a feasible utterance
    z, refs = small
    l = lib()
    full = align(z, SMALL_LENS, SMALL_YS, 9, maxL=12)
    tgt, off, tl = flat_targets(SMALL_YS)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    zd, ln, tg, of, tld = d(z), d(np.asarray(SMALL_LENS, np.int32)), d(tgt), d(off), d(tl)
    nb = int(l.masr_ctc_align_work_bytes(6, 24, 12))
    work = torch.empty(nb, dtype=torch.uint8, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    fr, st, en, sc = torch.full((6, 24), MARK, **i32), torch.full((6, 12), MARK, **i32), torch.full((6, 12), MARK, **i32), torch.zeros(6, device=DEV)
    assert l.masr_test_ctc_align_no_trace(p(zd), 12, p(ln), p(tg), p(of), p(tld), 6, 24, 9, 0, 12, p(work), nb, p(fr), p(st), p(en), p(sc), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), full[3].view(np.uint32))
    for b, r in enumerate(refs):
        assert (fr[b] == (MARK if r["states"] is not None else -2)).all()


def test_against_ctc_loss(small):
    """the best path's probability is at most the sum over all paths, masr_ctc_loss's exp(-nll), and equal to it where there is one path:
    the unique-path utterance and the two without tokens.  tol = the score's bound above + what masr_ctc_loss's own kernel test
    (test_hip_misc.py) allows its loss, 2e-5 relative."""
    z, refs = small
    l = lib()
    fr, st, en, sc = align(z, SMALL_LENS, SMALL_YS, 9, maxL=12)
    B, Tp, Cn, maxS = 6, 24, 9, 25
    tgt, off, tl = flat_targets(SMALL_YS)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lg = d(z[..., :Cn].transpose(1, 0, 2))                       # [T][B][C]
    work = torch.zeros(int(l.masr_ctc_work_floats(Tp, B, maxS)), device=DEV)
    nll, loss, grad = torch.zeros(B, device=DEV), torch.zeros(1, device=DEV), torch.zeros_like(lg)
    tg, of, il, tld = d(tgt), d(off), d(np.asarray(SMALL_LENS, np.int32)), d(tl)          # (named: alive until the launch has read them)
    rc = l.masr_ctc_loss(p(lg), p(tg), p(of), p(il), p(tld), Tp, B, Cn, 0, p(nll), p(loss), p(grad), p(work), maxS, stream())
    assert rc == 0, l.masr_last_error()
    nll = nll.cpu().numpy()
    for b in range(B):
        if refs[b]["states"] is None:
            continue
        n = SMALL_LENS[b]
        _, M = ar.viterbi_f64(z[b, :, :Cn], n, SMALL_YS[b], 0)
        tol = ar.score_bound(z[b, :, :Cn], n, M) + 2e-5 * abs(float(nll[b]))
        print(f"b={b}: score {float(sc[b]):.6f} -nll {-float(nll[b]):.6f} tol {tol:.3g}")
        assert float(sc[b]) <= -float(nll[b]) + tol, b
        if b in (1, 2, 3):
            assert abs(float(sc[b]) + float(nll[b])) <= tol, b
