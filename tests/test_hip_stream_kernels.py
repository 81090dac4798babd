"""The two kernels of the streaming first pass alone (csrc/stream.hip), through masr_test_attention_stream and
masr_test_ctc_greedy_stream.

The attention is compared with an fp64 restatement at test_attention's forward tolerances (tests/test_hip_kernels.py: o rtol 2e-2, atol 2e-2;
the products are bf16, the sums fp32, the output bf16).  B = 3 utterances with ragged klens: one at or below lo (a row without a key: exactly
0), one inside the step's new rows, one full."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from masr_amd import _cabi  # noqa: E402

B_, H = 3, 2
RTOL = ATOL = 2e-2


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def lo_of(kind, pos):
    return {"zero": 0, "pos": pos, "inside": pos // 2 + 3 if pos > 8 else pos // 2}[kind]


def inputs(hd, R, pos, lo, seed=0):
    """q / knew / vnew bf16 [B, R, H, hd], a cache of pos + R + 5 rows filled with a finite pattern, klens as the module docstring says"""
    g = torch.Generator(device="cuda").manual_seed(1000 * hd + 37 * R + pos + seed)
    q, kn, vn = (torch.randn(B_, R, H, hd, device="cuda", generator=g).bfloat16() for _ in range(3))
    cap = pos + R + 5
    kc, vc = (torch.randn(B_, cap, H, hd, device="cuda", generator=g).bfloat16() for _ in range(2))
    klens = torch.tensor([lo, pos + (R + 1) // 2, pos + R], dtype=torch.int32, device="cuda")
    return q, kn, vn, kc, vc, klens, cap


def run(q, kn, vn, kc, vc, klens, pos, lo, cap=None, hd=None, R=None, expect=0, fill=7.0):
    o = torch.full_like(q, fill)
    rc = _cabi.lib().masr_test_attention_stream(P(q), P(kn), P(vn), P(kc), P(vc), P(o), P(klens), B_, H, q.shape[3] if hd is None else hd,
                                                q.shape[1] if R is None else R, pos, lo, kc.shape[1] if cap is None else cap, S())
    torch.cuda.synchronize()
    assert rc == expect, _cabi.lib().masr_last_error()
    return o


def reference(q, kn, vn, kc, vc, klens, pos, lo):
    """fp64: every row attends the keys [lo, min(pos + R, klen_b)) of cache[:pos] | new; a row without a key is 0"""
    R, hd = q.shape[1], q.shape[3]
    k = torch.cat([kc[:, :pos], kn], 1).double().cpu(); v = torch.cat([vc[:, :pos], vn], 1).double().cpu(); qd = q.double().cpu()
    o = torch.zeros(B_, R, H, hd, dtype=torch.float64)
    for b in range(B_):
        hi = min(pos + R, int(klens[b]))
        if hi <= lo:
            continue
        s = torch.einsum("ihd,jhd->hij", qd[b], k[b, lo:hi]) / hd ** 0.5
        o[b] = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), v[b, lo:hi])
    return o


SHAPES = [(64, 1), (64, 3), (64, 16), (64, 24), (32, 8), (16, 8)]          # (24 = two query tiles)
POS = [0, 5, 48, 60, 127, 300]                                              # pos + R crosses the 64- and 128-key borders; a wave without a block


@pytest.mark.parametrize("lo_kind", ["zero", "pos", "inside"])
@pytest.mark.parametrize("pos", POS)
@pytest.mark.parametrize("hd,R", SHAPES)
def test_stream_attention_matches_fp64_and_appends_its_rows(hd, R, pos, lo_kind):
    lo = lo_of(lo_kind, pos)
    q, kn, vn, kc, vc, klens, cap = inputs(hd, R, pos, lo)
    kc0, vc0 = kc.clone(), vc.clone()
    o = run(q, kn, vn, kc, vc, klens, pos, lo)
    ref = reference(q, kn, vn, kc0, vc0, klens, pos, lo)
    got = o.double().cpu()
    assert bool(torch.isfinite(got).all())
    worst = float(((got - ref).abs() - RTOL * ref.abs()).max())
    print(f"hd {hd} R {R} pos {pos} lo {lo}: o misses rtol by {worst:.3g} (atol {ATOL})")
    assert worst <= ATOL
    assert bool((o[0] == 0).all())                                           # klens[0] <= lo: the empty-row rule, exactly 0
    # the cache: rows [pos, pos + R) are the new rows bit for bit, for every utterance (padding rows included); nothing else moved
    for c, c0, new in ((kc, kc0, kn), (vc, vc0, vn)):
        assert torch.equal(bits(c[:, pos:pos + R]), bits(new))
        assert torch.equal(bits(c[:, :pos]), bits(c0[:, :pos])) and torch.equal(bits(c[:, pos + R:]), bits(c0[:, pos + R:]))


@pytest.mark.parametrize("pos", POS)
@pytest.mark.parametrize("hd,R", SHAPES)
def test_full_left_context_agrees_with_the_forward_kernel(hd, R, pos):
    """lo = 0: the same attention as masr_test_attention with Tq = R, Tk = pos + R (utterances with at least one key)"""
    q, kn, vn, kc, vc, klens, cap = inputs(hd, R, pos, 0, seed=1)
    klens[0] = max(1, pos)
    k = torch.cat([kc[:, :pos], kn], 1).contiguous(); v = torch.cat([vc[:, :pos], vn], 1).contiguous()
    o = run(q, kn, vn, kc, vc, klens, pos, 0)
    o2 = torch.zeros_like(q); lse = torch.zeros(B_, H, R, device="cuda")
    _cabi.check(_cabi.lib().masr_test_attention(P(q), P(k), P(v), None, P(o2), None, None, None, P(lse), None, P(klens), B_, H, R, pos + R, hd, 0, S()))
    torch.cuda.synchronize()
    a, r = o.double().cpu(), o2.double().cpu()
    assert bool(torch.isfinite(a).all())
    assert float(((a - r).abs() - RTOL * r.abs()).max()) <= ATOL


def test_refusals_leave_the_output_and_the_cache_unwritten():
    q, kn, vn, kc, vc, klens, cap = inputs(64, 8, 20, 0, seed=2)
    kc0, vc0 = kc.clone(), vc.clone()
    for kw, word in ((dict(R=0), "R >= 1"), (dict(cap=27), "pos + R <= cap"), (dict(hd=48), "16/32/64")):
        o = run(q, kn, vn, kc, vc, klens, 20, 0, expect=-1, **kw)
        assert word in _cabi.lib().masr_last_error().decode()
        assert bool((o == 7.0).all()) and torch.equal(bits(kc), bits(kc0)) and torch.equal(bits(vc), bits(vc0))
    o = run(q, kn, vn, kc, vc, klens, 20, 21, expect=-1)
    assert "lo <= pos" in _cabi.lib().masr_last_error().decode()
    assert bool((o == 7.0).all()) and torch.equal(bits(kc), bits(kc0)) and torch.equal(bits(vc), bits(vc0))


# ---------------------------------------------------------------------------- greedy CTC with carry
def best_path(z, C_, klen):
    """one-shot best path of z [T, ld]: arg-max over the C valid columns (the first maximal index), repeats merged, blanks dropped"""
    am = np.argmax(z[:klen, :C_], axis=1)
    tok, frm, prev = [], [], 0
    for t, a in enumerate(am.tolist()):
        if a != 0 and a != prev:
            tok.append(a); frm.append(t)
        prev = a
    return tok, frm


@pytest.mark.parametrize("R", [1, 4, 7])
@pytest.mark.parametrize("C_", [11, 53])
def test_streamed_greedy_equals_the_one_shot_best_path(C_, R):
    T, ld = 29, 64
    g = torch.Generator().manual_seed(C_ * 10 + R)
    z = torch.randn(B_, T, ld, generator=g)
    z[:, :, C_:] = 50.0                                                      # columns behind C are not valid, whatever they hold
    for b in range(B_):
        for t in range(0, T, 3):                                             # planted ties: two classes share the maximum, the lower index wins
            c1, c2 = sorted(torch.randperm(C_, generator=g)[:2].tolist())
            z[b, t, c1] = z[b, t, c2] = 9.0
        for t0 in (3, 6, 13, 20):                                            # the same token on both sides of a step border (R = 4: 3|4, R = 7: 6|7, 13|14, 20|21)
            tok = 1 + (b + t0) % (C_ - 1)
            z[b, t0, :C_] = -1.0; z[b, t0 + 1, :C_] = -1.0
            z[b, t0, tok] = z[b, t0 + 1, tok] = 12.0
    klens = torch.tensor([T, 17, 0], dtype=torch.int32)
    zd = z.cuda()
    state = torch.zeros(2, B_, dtype=torch.int32, device="cuda")
    tokens = torch.full((B_, T), -1, dtype=torch.int32, device="cuda"); frames = tokens.clone()
    for pos in range(0, T, R):
        step = zd[:, pos:pos + R].contiguous()
        _cabi.check(_cabi.lib().masr_test_ctc_greedy_stream(P(step), ld, P(klens.cuda()), B_, step.shape[1], C_, pos, P(state), P(tokens), P(frames), T, S()))
    torch.cuda.synchronize()
    lens = state[1].cpu().tolist()
    emitted = 0
    for b in range(B_):
        tok, frm = best_path(z[b].numpy(), C_, int(klens[b]))
        assert tokens[b, :lens[b]].cpu().tolist() == tok and frames[b, :lens[b]].cpu().tolist() == frm, (b, R, C_)
        assert bool((tokens[b, lens[b]:] == -1).all())
        emitted += len(tok)
    assert emitted > 10 and lens[2] == 0
