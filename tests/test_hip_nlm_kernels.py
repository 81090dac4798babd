"""The LSTM LM's step kernels alone (csrc/nlm.hip) through masr_test_nlm_step, and masr_nlm_score on top of them.

The step is checked in fp64 on the values the kernel itself read: its bf16 weights and embedding rows (the host builder rounds to nearest
even, as torch's .bfloat16() does), the caller's bf16 parent h and fp32 parent c, and for layer l > 0 the kernel's OWN new h of layer l - 1.
Bounds, per class, derived as tests/lstm_ref.py check_fwd derives them:
    z      an fp32 sum of INp + Hp exact products and the bias in any grouping: (INp + Hp + 2) 2^-24 (sum |x W| + |b|)
    gates  z's bound through the largest derivative nearby + GPU_EXP_ALLOWANCE ulps (_sig_bound, _tanh_bound)
    c      the gates' bounds through the two products, three fp32 roundings
    h      c's bound through tanh, the allowance, one product, then one rounding to bf16 (bf16_half_ulp of the largest magnitude possible)
    logits an fp32 sum of Hp exact products and the bias: (Hp + 2) 2^-24 (sum |h lo| + |lo_b|)
    logp   (y - mx) - log_s from the kernel's own logits: one rounding of y - mx, __expf's allowance and scaled argument, C additions, __logf's
           allowance on |log_s|, two roundings of the result
The worst err / bound per class is printed."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import nlm_ref  # noqa: E402
from lstm_ref import GPU_EXP_ALLOWANCE, TINY32, U24, ULP32, Worst, _sig_bound, _tanh_bound, bf16_half_ulp  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.nlm import LstmLM  # noqa: E402

F64 = torch.float64
DEV = "cuda:0"
NAN16 = 0x7FC0
GUARD = 3                                                      # NaN rows in front of and behind every array the kernels write


def pad32(n):
    return (n + 31) // 32 * 32


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def guarded(rows, cols, dtype):
    """a NaN-filled [rows + 2 GUARD][cols] device tensor and its interior view"""
    full = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + rows]


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def parents(R, K, kind):
    """shared: two rows of an utterance share a parent; perm: a permutation of each utterance's rows without a fixed point (K > 1)"""
    u0 = torch.arange(R) // K * K
    i = torch.arange(R) % K
    return (u0 + i // 2 if kind == "shared" else u0 + (i + 1) % K).to(torch.int32)


def run_step(lm, m, R, K, t, par_kind, seed, dead=()):
    """one masr_test_nlm_step call on random previous states -> everything the check needs, on the host"""
    L, H, Hp, Cn = lm.L, lm.H, pad32(lm.H), lm.C
    g = torch.Generator().manual_seed(seed)
    cur, prv = t & 1, (t - 1) & 1
    hfull, hs = guarded(2 * L * R, Hp, torch.bfloat16)
    cfull, cs = guarded(2 * L * R, Hp, torch.float32)
    hs, cs = hs.view(2, L, R, Hp), cs.view(2, L, R, Hp)
    h_prev = torch.zeros(L, R, Hp); c_prev = torch.zeros(L, R, Hp)
    h_prev[..., :H] = torch.rand(L, R, H, generator=g) * 2 - 1
    c_prev[..., :H] = (torch.rand(L, R, H, generator=g) * 2 - 1) * 1.5
    h_prev = h_prev.bfloat16()
    if t > 1:                                                   # (t = 1 reads no previous state: it stays NaN)
        hs[prv] = h_prev.to(DEV); cs[prv] = c_prev.to(DEV)
    tok = torch.randint(0, Cn, (R,), generator=g, dtype=torch.int32)
    par = parents(R, K, par_kind)
    score = torch.zeros(R)
    score[list(dead)] = float("-inf")
    ld = Cn + 5
    lfull, logits = guarded(R, ld, torch.float32)
    pfull, logp = guarded(R, ld, torch.float32)
    before_h, before_c = hfull.clone(), cfull.clone()
    tok_d, par_d, score_d = tok.to(DEV), par.to(DEV), score.to(DEV)       # (named: they must outlive the call)
    rc = lib().masr_test_nlm_step(lm.h, R, K, t, ptr(tok_d), ptr(par_d), ptr(score_d), ptr(hs), ptr(cs), ptr(logits), ld, ptr(logp), None)
    assert rc == 0, lib().masr_last_error()
    # nothing outside the new parity's interior was touched: guards, and the previous parity bit for bit (no update in place)
    assert all_nan(hfull[:GUARD]) and all_nan(hfull[-GUARD:]) and all_nan(cfull[:GUARD]) and all_nan(cfull[-GUARD:])
    assert torch.equal(hs[prv].view(torch.int16), before_h[GUARD:-GUARD].view(2, L, R, Hp)[prv].view(torch.int16))
    assert torch.equal(cs[prv].view(torch.int32), before_c[GUARD:-GUARD].view(2, L, R, Hp)[prv].view(torch.int32))
    assert all_nan(lfull[:GUARD]) and all_nan(lfull[-GUARD:]) and all_nan(logits[:, Cn:]) and all_nan(pfull[:GUARD]) and all_nan(logp[:, Cn:])
    return dict(t=t, tok=tok.long(), par=par.long(), live=torch.isfinite(score), h_prev=h_prev.to(F64), c_prev=c_prev.to(F64),
                h_new=hs[cur].cpu(), c_new=cs[cur].cpu(), logits=logits[:, :Cn].cpu(), logp=logp[:, :Cn].cpu())


def check_step(m, o, worst, what):
    L, H = len(m["w_ih"]), m["w_hh"][0].shape[1]
    Hp = pad32(H)
    live, t = o["live"], o["t"]
    R = live.numel()
    bf = lambda a: torch.from_numpy(a).bfloat16().to(F64)      # noqa: E731
    tok = o["tok"] if t > 1 else torch.full((R,), m["start_id"], dtype=torch.long)
    par = o["par"] if t > 1 else torch.arange(R)
    x = bf(m["embed"])[tok]
    for l in range(L):
        Wi, Wh = bf(m["w_ih"][l]), bf(m["w_hh"][l])
        b = torch.from_numpy((m["b_ih"][l] + m["b_hh"][l]).astype(np.float32)).to(F64)
        hp = o["h_prev"][l][par][:, :H] if t > 1 else torch.zeros(R, H, dtype=F64)
        cp = o["c_prev"][l][par][:, :H] if t > 1 else torch.zeros(R, H, dtype=F64)
        KT = pad32(x.shape[1]) + Hp
        z = (x @ Wi.t() + hp @ Wh.t() + b).view(R, 4, H)
        zb = ((KT + 2) * U24 * (x.abs() @ Wi.abs().t() + hp.abs() @ Wh.abs().t() + b.abs())).view(R, 4, H)
        sig = lambda v: 1.0 / (1.0 + torch.exp(-v))              # noqa: E731
        i64, f64, g64, o64 = sig(z[:, 0]), sig(z[:, 1]), torch.tanh(z[:, 2]), sig(z[:, 3])
        bi, bff, bg, bo = (_sig_bound(z[:, 0], zb[:, 0], i64), _sig_bound(z[:, 1], zb[:, 1], f64), _tanh_bound(z[:, 2], zb[:, 2], g64),
                           _sig_bound(z[:, 3], zb[:, 3], o64))
        c64 = f64 * cp + i64 * g64
        cb = cp.abs() * bff + g64.abs() * bi + (i64 + bi) * bg + 3.0 * U24 * ((f64 * cp).abs() + (i64 * g64).abs()) + TINY32
        got_c, got_h = o["c_new"][l].to(F64), o["h_new"][l].to(F64)
        worst.within((got_c[:, :H] - c64).abs()[live], cb[live], "c", (what, l))
        tc = torch.tanh(c64)
        tb = _tanh_bound(c64, cb, tc)
        h64 = o64 * tc
        hb = o64 * tb + (tc.abs() + tb) * bo + U24 * h64.abs()
        yb = hb + bf16_half_ulp(h64.abs() + hb) + TINY32
        worst.within((got_h[:, :H] - h64).abs()[live], yb[live], "h", (what, l))
        # padded units: exactly +0; dead rows: never written
        assert (o["c_new"][l][live][:, H:].view(torch.int32) == 0).all() and (o["h_new"][l][live][:, H:].view(torch.int16) == 0).all(), (what, l)
        assert all_nan(o["c_new"][l][~live]) and all_nan(o["h_new"][l][~live]), ("a dead row wrote its state", what, l)
        x = got_h[:, :H]                                         # the next layer read the kernel's own bf16 h
    lo, lob = bf(m["lo_w"]), torch.from_numpy(m["lo_b"]).to(F64)
    y64 = x @ lo.t() + lob
    yb = (Hp + 2) * U24 * (x.abs() @ lo.abs().t() + lob.abs()) + TINY32
    y = o["logits"].to(F64)
    worst.within((y - y64).abs()[live], yb[live], "logits", what)
    d = y - y.max(dim=1, keepdim=True).values
    log_s = torch.log(torch.exp(d).sum(dim=1, keepdim=True))
    lp64 = d - log_s
    Cn = y.shape[1]
    rel_s = GPU_EXP_ALLOWANCE * ULP32 + (d.abs().max(dim=1, keepdim=True).values + 1.0) * U24 + Cn * U24
    lb = U24 * d.abs() + rel_s + GPU_EXP_ALLOWANCE * ULP32 * log_s.abs() + 2.0 * U24 * lp64.abs() + TINY32
    worst.within((o["logp"].to(F64) - lp64).abs()[live], lb.expand_as(lp64)[live], "logp", what)
    assert (o["logp"][live] <= 0).all()


#        E     H    L  R   K     what the shape is for
SHAPES = [(16, 24, 2, 5, 5),     # padding on both dims, fewer rows than a tile
          (64, 96, 1, 33, 11),   # three row tiles, ragged
          (40, 200, 2, 20, 5),   # padded reduction 64 + 224 = 288, ragged across the waves' 128-wide split
          (1024, 1024, 1, 17, 17)]   # reduction 2048: the unrolled loop

_LMS = {}


def model(E, H, L, Cn=20, seed=3, start_id=0):
    key = (E, H, L, Cn, seed, start_id)
    if key not in _LMS:
        m = nlm_ref.toy_nlm(Cn, E, H, L, seed, start_id)
        _LMS[key] = (m, LstmLM.from_state_dict(nlm_ref.to_state_dict(m), start_id=start_id))
    return _LMS[key]


@pytest.mark.parametrize("E, H, L, R, K", SHAPES)
def test_nlm_step_against_fp64(E, H, L, R, K):
    m, lm = model(E, H, L)
    worst = Worst()
    n = 0
    for t, kind in ((2, "shared"), (3, "shared"), (2, "perm"), (3, "perm"), (1, "perm")):
        dead = (1, R - 1) if kind == "perm" else ()
        o = run_step(lm, m, R, K, t, kind, seed=100 * t + n, dead=dead)
        check_step(m, o, worst, (E, H, L, R, t, kind))
        n += 1
    print(f"  (E, H, L, R) = {(E, H, L, R)}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_own_slot_or_in_place_would_fail():
    """the check tells the parent's state from the row's own: with a fixed-point-free parent table, a reference that reads the row's own slot
    is far outside the bounds for the kernel's output"""
    m, lm = model(16, 24, 2)
    o = run_step(lm, m, 5, 5, 2, "perm", seed=7)
    check_step(m, o, Worst(), "as it is")
    wrong = dict(o, par=torch.arange(5))
    with pytest.raises(AssertionError):
        check_step(m, wrong, Worst(), "own slot")


def test_start_token_is_the_handles():
    """start_id = C - 1 (LMs trained with sos = eos): step 1 feeds that row of the embedding"""
    m, lm = model(16, 24, 1, start_id=19)
    o = run_step(lm, m, 5, 5, 1, "perm", seed=9)
    check_step(m, o, Worst(), "start = eos")
    m0 = dict(m, start_id=0)
    with pytest.raises(AssertionError):
        check_step(m0, o, Worst(), "start = sos")


# ---------------------------------------------------------------- masr_nlm_score
def chain_score(lm, token_lists):
    """the same position-by-position chain through masr_test_nlm_step, every row its own parent, fp32 additions in position order"""
    R, L, Hp, Cn = len(token_lists), lm.L, pad32(lm.H), lm.C
    ld = (Cn + 127) // 128 * 128
    hs = torch.zeros(2, L, R, Hp, dtype=torch.bfloat16, device=DEV)
    cs = torch.zeros(2, L, R, Hp, dtype=torch.float32, device=DEV)
    logits = torch.zeros(R, ld, device=DEV); logp = torch.zeros(R, ld, device=DEV)
    acc = np.zeros(R, dtype=np.float32)
    mx = max(len(t) for t in token_lists)
    for i in range(mx + 1):
        tok = torch.tensor([t[i - 1] if 0 < i <= len(t) else 0 for t in token_lists], dtype=torch.int32, device=DEV)
        assert lib().masr_test_nlm_step(lm.h, R, 1, i + 1, ptr(tok), None, None, ptr(hs), ptr(cs), ptr(logits), ld, ptr(logp), None) == 0
        rows = logp.cpu().numpy()
        for r, t in enumerate(token_lists):
            if i <= len(t):
                acc[r] = np.float32(acc[r] + rows[r, t[i] if i < len(t) else Cn - 1])
    return acc


@pytest.mark.parametrize("Cn, E, H, L", [(12, 16, 24, 2), (367, 40, 72, 1)])
def test_nlm_score(Cn, E, H, L):
    m, lm = model(E, H, L, Cn=Cn, seed=5)
    rng = np.random.RandomState(Cn)
    lists = [[int(t) for t in rng.randint(1, Cn - 1, size=n)] for n in (0, 1, 7, 12, 3)]
    got = lm.score(lists).numpy()
    chain = chain_score(lm, lists)
    assert got.view(np.int32).tolist() == chain.view(np.int32).tolist(), (got, chain)      # same kernels, same order: bit for bit
    worst = 0.0
    for r, t in enumerate(lists):
        want = nlm_ref.score(m, t)
        print(f"  C = {Cn}, {len(t)} tokens: engine {got[r]:.4f}, restatement {want:.4f}, diff {abs(got[r] - want):.2e}, bound {0.02 + 2e-3 * abs(want):.4f}")
        worst = max(worst, abs(float(got[r]) - want))
        assert abs(float(got[r]) - want) <= 0.02 + 2e-3 * abs(want), (r, got[r], want)
    print(f"C = {Cn}: worst |engine - restatement| {worst:.2e}")
    assert (got < 0).all()


def test_nlm_score_refusals():
    m, lm = model(16, 24, 2, Cn=12, seed=5)
    l = lib()
    tok = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    lens = torch.tensor([2, 4], dtype=torch.int32, device=DEV)
    out = torch.zeros(2, device=DEV)
    need = l.masr_nlm_score_work_bytes(lm.h, 2, 4)
    assert need > 0
    work = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = (work.data_ptr() + 255) // 256 * 256
    call = lambda h, t, n, R, ld, o, w, nb: l.masr_nlm_score(h, ptr(t), ptr(n), R, ld, ptr(o), C.c_void_p(w) if w else None, nb, None)  # noqa: E731
    assert call(lm.h, tok, lens, 2, 4, out, base, need) == 0
    assert call(None, tok, lens, 2, 4, out, base, need) != 0 and b"null language model" in l.masr_last_error()
    assert call(lm.h, tok, None, 2, 4, out, base, need) != 0 and b"null pointer" in l.masr_last_error()
    assert call(lm.h, tok, lens, 0, 4, out, base, need) != 0 and b"1 <= R" in l.masr_last_error()
    assert call(lm.h, tok, lens, 2, 4, out, base, need - 1) != 0 and b"masr_nlm_score_work_bytes" in l.masr_last_error()
    assert call(lm.h, tok, lens, 2, 4, out, base + 16, need) != 0 and b"aligned" in l.masr_last_error()
    assert call(lm.h, tok, torch.tensor([2, 5], dtype=torch.int32, device=DEV), 2, 4, out, base, need) != 0 and b"lens" in l.masr_last_error()
    bad = tok.clone(); bad[1, 3] = 12
    assert call(lm.h, bad, lens, 2, 4, out, base, need) != 0 and b"tokens must lie in [0, C - 1]" in l.masr_last_error()
    assert l.masr_nlm_score_work_bytes(None, 2, 4) < 0 and l.masr_nlm_score_work_bytes(lm.h, 2, 5000) < 0


def test_nlm_create_refusals():
    m = nlm_ref.toy_nlm(12, 16, 24, 2, 1)
    sd = nlm_ref.to_state_dict(m)
    assert LstmLM.from_state_dict(sd).device_bytes > 0
    for start in (-1, 12):
        with pytest.raises(MasrError, match="start_id"):
            LstmLM.from_state_dict(sd, start_id=start)
    bad = dict(sd); bad["rnn.weight_hh_l1"] = sd["rnn.weight_hh_l1"].clone(); bad["rnn.weight_hh_l1"][3, 3] = float("nan")
    with pytest.raises(MasrError, match="not finite"):
        LstmLM.from_state_dict(bad)
    bad = dict(sd); bad["lo.bias"] = sd["lo.bias"].clone(); bad["lo.bias"][0] = float("-inf")
    with pytest.raises(MasrError, match="not finite"):
        LstmLM.from_state_dict(bad)
    one = nlm_ref.to_state_dict(nlm_ref.toy_nlm(1, 4, 4, 1, 1))
    with pytest.raises(MasrError, match=r"\[2, 65535\]"):
        LstmLM.from_state_dict(one)
    l = lib()
    P = C.c_void_p * 1
    e = np.zeros((4, 4), dtype=np.float32)
    assert not l.masr_nlm_create(4, 4, 4, 1, 0, None, P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), e.ctypes.data, e.ctypes.data)
    assert b"null pointer" in l.masr_last_error()
    assert not l.masr_nlm_create(4, 4, 4, 1, 0, e.ctypes.data, P(None), P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), e.ctypes.data, e.ctypes.data)
    assert b"null pointer" in l.masr_last_error()
    assert not l.masr_nlm_create(4, 4, 4, 5, 0, e.ctypes.data, P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), e.ctypes.data, e.ctypes.data)
    assert b"layers" in l.masr_last_error()
    assert not l.masr_nlm_create(4, 4, 2049, 1, 0, e.ctypes.data, P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), P(e.ctypes.data), e.ctypes.data, e.ctypes.data)
    assert b"[1, 2048]" in l.masr_last_error()
