"""masr_ctc_beam_search_nlm alone (include/masr.h, DESIGN 5.12: ctc_beam_frames, then per frame ctc_beam_frame and the LM's carry step, then
ctc_beam_tail), model-free, and the carry form of the LM step alone through masr_test_nlm_step_carry.

The search is compared with the restatement of tests/ctc_nlm_beam_ref.py fed with an LM oracle that returns the DEVICE's log-softmax row of a
prefix (chained through masr_test_nlm_step from the zero state, cached per prefix), so the LM's own rounding is not in the comparison and
DESIGN 5.6's slack rule applies unchanged: where the restatement's slack is positive the N-best token lists and lengths are equal and am is
within ctc_beam_ref.tol.  With or without slack every returned score is fl(fl(am + lmacc(tokens)) + fl(lm_w * lm(eos | tokens))) recomputed
from the returned tokens, am and the oracle's rows, bit for bit.  A case fails if more than a quarter of its utterances are left out.  Outputs
and work buffers start filled with junk; padded frames and columns are NaN and never read."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_beam_ref as cr  # noqa: E402
import ctc_nlm_beam_ref as nr  # noqa: E402
import lm_ref  # noqa: E402
import nlm_ref  # noqa: E402
from ctc_lm_beam_ref import final32  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402
from masr_amd.nlm import LstmLM  # noqa: E402
from test_hip_ctc_beam_kernel import search as plain_search  # noqa: E402
from test_hip_ctc_lm_beam_kernel import device_lm as device_ngram, search_lm as search_ngram  # noqa: E402

DEV = "cuda:0"
GUARD = 3


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def pad32(n):
    return (n + 31) // 32 * 32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_LMS = {}


def device_nlm(m):
    """the dict form of nlm_ref -> LstmLM, one per dict and process"""
    if id(m) not in _LMS:
        _LMS[id(m)] = (m, LstmLM(m["embed"], m["w_ih"], m["w_hh"], m["b_ih"], m["b_hh"], m["lo_w"], m["lo_b"], start_id=m["start_id"]))
    return _LMS[id(m)][1]


def toy(Cn, dims=nr.NLM_DIMS, seed=0):
    key = (Cn, dims, seed)
    if key not in _LMS:
        m = nlm_ref.toy_nlm(Cn, *dims, seed)
        _LMS[key] = (m, device_nlm(m))
    return _LMS[key]


# ---------------------------------------------------------------- the carry form alone
def nan_guarded(rows, cols, dtype):
    full = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + rows]


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


#              E   H   L  R   K   live per utterance      what the shape is for
CARRY_SHAPES = [(16, 24, 1, 5, 5, [4]),                  # a partial tile with a dead row, Hp 32
                (16, 24, 2, 33, 11, [11, 9, 11]),        # a tile that straddles utterances; rows 16 .. 31 are one all-stay tile
                (24, 40, 2, 33, 11, [11, 9, 11]),        # Hp 64
                (24, 40, 1, 5, 5, [5])]


@pytest.mark.parametrize("E,H,L,R,K,nlive", CARRY_SHAPES)
@pytest.mark.parametrize("t", [3, 4])
def test_carry_form(E, H, L, R, K, nlive, t):
    Cn = 23
    m, lm = toy(Cn, (E, H, L), 1)
    Hp, B, ld = pad32(H), R // K, Cn + 5
    cur, prv = t & 1, (t - 1) & 1
    g = torch.Generator().manual_seed(100 * R + t)
    live_rows = torch.tensor([r % K < nlive[r // K] for r in range(R)])
    stay = torch.rand(R, generator=g) < 0.5
    if R > 16:
        stay[16:32] = True                                    # one tile of stays and dead rows only
        stay[32] = False
    stay[0] = True; stay[1] = False
    tok = torch.randint(1, Cn - 1, (R,), generator=g, dtype=torch.int32)
    marks = torch.tensor([-1, 0, Cn - 1, 1 << 20, -7], dtype=torch.int32)          # everything outside [1, C - 2] marks a stay
    tok_c = torch.where(stay, marks[torch.arange(R) % len(marks)], tok)
    par = (torch.arange(R) // K * K + torch.randint(0, K, (R,), generator=g)).to(torch.int32)
    par_c = par.clone()
    tok_c[~live_rows] = 0x7F7F7F7F; par_c[~live_rows] = 0x7F7F7F7F                    # a dead row's records are junk
    h_prev = torch.zeros(L, R, Hp); c_prev = torch.zeros(L, R, Hp)
    h_prev[..., :H] = torch.rand(L, R, H, generator=g) * 2 - 1
    c_prev[..., :H] = (torch.rand(L, R, H, generator=g) * 2 - 1) * 1.5
    lp_prev = -torch.rand(R, ld, generator=g) * 5

    def states():
        hfull, hs = nan_guarded(2 * L * R, Hp, torch.bfloat16)
        cfull, cs = nan_guarded(2 * L * R, Hp, torch.float32)
        hs, cs = hs.view(2, L, R, Hp), cs.view(2, L, R, Hp)
        hs[prv] = h_prev.bfloat16().to(DEV); cs[prv] = c_prev.to(DEV)
        return hfull, hs, cfull, cs

    # the reference: the plain step on every row
    _, hs0, _, cs0 = states()
    _, lg0 = nan_guarded(R, ld, torch.float32)
    _, lp0 = nan_guarded(R, ld, torch.float32)
    tok_d, par_d = tok.to(DEV), par.to(DEV)
    assert lib().masr_test_nlm_step(lm.h, R, K, t, p(tok_d), p(par_d), None, p(hs0), p(cs0), p(lg0), ld, p(lp0), None) == 0, lib().masr_last_error()
    # the carry form
    hfull, hs, cfull, cs = states()
    lgfull, lg = nan_guarded(R, ld, torch.float32)
    lpfull, lp = nan_guarded(2 * R, ld, torch.float32)
    lp = lp.view(2, R, ld)
    lp[prv] = lp_prev.to(DEV)
    live = torch.full((2, B), 0x7F7F7F7F, dtype=torch.int32)
    live[cur] = torch.tensor(nlive, dtype=torch.int32)
    tokc_d, parc_d, live_d = tok_c.to(DEV), par_c.to(DEV), live.to(DEV)
    before_h, before_c, before_lp = hs.clone(), cs.clone(), lp.clone()
    rc = lib().masr_test_nlm_step_carry(lm.h, R, K, t, p(tokc_d), p(parc_d), p(live_d), p(hs), p(cs), p(lg), ld, p(lp), None)
    assert rc == 0, lib().masr_last_error()
    for t_ in (hfull, cfull, lgfull, lpfull):
        assert all_nan(t_[:GUARD]) and all_nan(t_[-GUARD:])
    assert torch.equal(hs[prv].view(torch.int16), before_h[prv].view(torch.int16)) and torch.equal(cs[prv].view(torch.int32), before_c[prv].view(torch.int32))
    assert torch.equal(lp[prv].view(torch.int32), before_lp[prv].view(torch.int32))
    assert all_nan(lp[cur][:, Cn:])
    i16, i32 = torch.int16, torch.int32
    for r in range(R):
        if not live_rows[r]:
            assert all_nan(hs[cur][:, r]) and all_nan(cs[cur][:, r]) and all_nan(lp[cur][r]), ("a dead row was written", r)
        elif stay[r]:
            q = int(par[r])
            assert torch.equal(hs[cur][:, r].view(i16), hs[prv][:, q].view(i16)) and torch.equal(cs[cur][:, r].view(i32), cs[prv][:, q].view(i32)), r
            assert torch.equal(lp[cur][r, :Cn].view(i32), lp[prv][q, :Cn].view(i32)), r
        else:
            assert torch.equal(hs[cur][:, r].view(i16), hs0[cur][:, r].view(i16)) and torch.equal(cs[cur][:, r].view(i32), cs0[cur][:, r].view(i32)), r
            assert torch.equal(lp[cur][r, :Cn].view(i32), lp0[r, :Cn].view(i32)), r


def test_carry_form_first_step_starts_the_live_rows():
    Cn, R, K = 23, 10, 5
    m, lm = toy(Cn, (16, 24, 2), 1)
    L, Hp, ld = 2, 32, Cn
    _, hs0 = nan_guarded(2 * L * R, Hp, torch.bfloat16); _, cs0 = nan_guarded(2 * L * R, Hp, torch.float32)
    _, lg0 = nan_guarded(R, ld, torch.float32); _, lp0 = nan_guarded(R, ld, torch.float32)
    assert lib().masr_test_nlm_step(lm.h, R, K, 1, None, None, None, p(hs0), p(cs0), p(lg0), ld, p(lp0), None) == 0, lib().masr_last_error()
    _, hs = nan_guarded(2 * L * R, Hp, torch.bfloat16); _, cs = nan_guarded(2 * L * R, Hp, torch.float32)
    _, lg = nan_guarded(R, ld, torch.float32); _, lp = nan_guarded(2 * R, ld, torch.float32)
    junk = torch.full((R,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    live = torch.tensor([[9, 9], [1, 1]], dtype=torch.int32, device=DEV)
    assert lib().masr_test_nlm_step_carry(lm.h, R, K, 1, p(junk), p(junk), p(live), p(hs), p(cs), p(lg), ld, p(lp), None) == 0, lib().masr_last_error()
    hs, cs, hs0, cs0, lp = hs.view(2, L, R, Hp), cs.view(2, L, R, Hp), hs0.view(2, L, R, Hp), cs0.view(2, L, R, Hp), lp.view(2, R, ld)
    for r in range(R):
        if r % K == 0:
            assert torch.equal(hs[1][:, r].view(torch.int16), hs0[1][:, r].view(torch.int16)) and torch.equal(cs[1][:, r].view(torch.int32), cs0[1][:, r].view(torch.int32))
            assert torch.equal(lp[1][r].view(torch.int32), lp0[r].view(torch.int32))
        else:
            assert all_nan(hs[1][:, r]) and all_nan(cs[1][:, r]) and all_nan(lp[1][r])
    assert all_nan(hs[0]) and all_nan(lp[0])


# ---------------------------------------------------------------- the search
def search_nlm(z, lens, Cn, K, nbest, dlm, lm_w, len_bonus, junk=0x7F):
    """z [B, Tp, ld] fp32 numpy, lens int32 [B] -> (tokens [B][nbest][Tp], lens [B][nbest], scores [B][nbest], am [B][nbest]) numpy"""
    B, Tp, ld = z.shape
    l = lib()
    zd = torch.from_numpy(z).to(DEV)
    ld_ = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    nb = int(l.masr_ctc_beam_nlm_work_bytes(dlm.h, B, Tp, Cn, K))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), junk, dtype=torch.uint8, device=DEV)
    assert work.data_ptr() % 256 == 0
    tok = torch.full((B, nbest, Tp), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    ln = torch.full((B, nbest), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    am = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    rc = l.masr_ctc_beam_search_nlm(p(zd), ld, p(ld_), B, Tp, Cn, K, nbest, 0, Cn - 1, dlm.h, lm_w, len_bonus, p(work), nb, p(tok), p(ln), p(sc),
                                    p(am), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), am.cpu().numpy()


class DeviceRows:
    """lm_row(h) = the device's fp32 log-softmax row after [start] + h, chained through masr_test_nlm_step from the zero state and cached per
    prefix with its (h, c).  prefetch() computes many prefixes of equal length in one call: a row's result does not depend on its index or on
    the rows around it."""

    def __init__(self, m, lm):
        self.m, self.lm, self.cache = m, lm, {}
        self.L, self.Hp, self.C = lm.L, pad32(lm.H), lm.C

    def _run(self, prefixes):
        n, R, L, Hp, Cn = len(prefixes[0]), len(prefixes), self.L, self.Hp, self.C
        t = n + 1
        hs = torch.zeros(2, L, R, Hp, dtype=torch.bfloat16)
        cs = torch.zeros(2, L, R, Hp, dtype=torch.float32)
        if n:
            for r, h in enumerate(prefixes):
                _, ph, pc = self.cache[h[:-1]]
                hs[(t - 1) & 1, :, r] = ph; cs[(t - 1) & 1, :, r] = pc
        hs, cs = hs.to(DEV), cs.to(DEV)
        tok = torch.tensor([h[-1] if h else 0 for h in prefixes], dtype=torch.int32, device=DEV)
        lg = torch.empty(R, Cn, device=DEV); lp = torch.empty(R, Cn, device=DEV)
        rc = lib().masr_test_nlm_step(self.lm.h, R, 1, t, p(tok), None, None, p(hs), p(cs), p(lg), Cn, p(lp), None)
        assert rc == 0, lib().masr_last_error()
        hn, cn, lp = hs[t & 1].cpu(), cs[t & 1].cpu(), lp.cpu().numpy()
        for r, h in enumerate(prefixes):
            self.cache[h] = (lp[r], hn[:, r].clone(), cn[:, r].clone())

    def prefetch(self, prefixes):
        need = set()
        for h in prefixes:
            for i in range(len(h) + 1):
                if tuple(h[:i]) not in self.cache:
                    need.add(tuple(h[:i]))
        for n in sorted({len(h) for h in need}):
            self._run(sorted(h for h in need if len(h) == n))

    def __call__(self, h):
        h = tuple(h)
        if h not in self.cache:
            self.prefetch([h])
        return self.cache[h][0]


def oracle_refs(name):
    """the restatement of every K of the case on the device's rows, and the oracle"""
    cs, z, lens, m = nr.make_nlm_case(name)
    rows = DeviceRows(m, device_nlm(m))
    seen = set()
    emu = nr.default_lm_row(m)

    def recording(h):
        seen.add(tuple(h))
        return emu(h)

    out = {}
    for K in cs["Ks"]:
        # a first pass on the emulated LM finds the prefixes the search asks for: they are computed on the device in a few batched calls
        nr.ctc_nlm_beam_ref_batch(z[..., :cs["C"]], lens, K, recording, cs["lm_w"], cs["len_bonus"], cs["nbest"])
        rows.prefetch(seen)
        out[K] = nr.ctc_nlm_beam_ref_batch(z[..., :cs["C"]], lens, K, rows, cs["lm_w"], cs["len_bonus"], cs["nbest"])
    print(f"{name}: {len(rows.cache)} distinct prefixes")
    return cs, z, lens, m, rows, out


def check_layout_and_scores(name, K, cs, rows, tok, ln, sc, am, nbest):
    for b in range(tok.shape[0]):
        live = ln[b] >= 0
        assert live[:live.sum()].all() and (ln[b][~live] == -1).all(), (name, K, b)
        assert np.isneginf(sc[b][~live]).all() and np.isneginf(am[b][~live]).all(), (name, K, b)
        for i in range(nbest):
            L = max(int(ln[b, i]), 0)
            assert (tok[b, i, L:] == -1).all() and ((tok[b, i, :L] > 0) & (tok[b, i, :L] < cs["C"] - 1)).all(), (name, K, b, i)
            if not live[i]:
                continue
            h = tuple(tok[b, i, :L].tolist())
            want = final32(am[b, i], nr.lmacc32(rows, h, cs["lm_w"], cs["len_bonus"]), nr.eos_term32(rows, h, cs["lm_w"], cs["C"] - 1))
            assert bits(sc[b, i:i + 1])[0] == bits(np.array([want], np.float32))[0], (name, K, b, i, h, float(sc[b, i]), float(want))
        assert (np.diff(sc[b][live]) <= 0).all(), (name, K, b)


@pytest.mark.parametrize("name", list(nr.NLM_CASES))
def test_against_restatement(name):
    cs, z, lens, m, rows, refs = oracle_refs(name)
    dlm = device_nlm(m)
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        tok, ln, sc, am = search_nlm(z, lens, cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"])
        check_layout_and_scores(name, K, cs, rows, tok, ln, sc, am, nbest)
        skipped = 0
        for b, r in enumerate(refs[K]):
            n, live = len(r["nbest"]), int((ln[b] >= 0).sum())
            print(f"{name} K={K} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} live {live}/{n} recreated {r['recreated']} max am err "
                  f"{max((abs(float(am[b, i]) - r['nbest'][i][2]) for i in range(min(n, live))), default=0.0):.3g}")
            if not r["slack"] > 0:
                skipped += 1
                continue
            assert live == n, (name, K, b, ln[b], n)
            for i, (pre, s, a, acc) in enumerate(r["nbest"]):
                assert tuple(tok[b, i, :ln[b, i]].tolist()) == pre, (name, K, b, i, tok[b, i, :ln[b, i]].tolist(), pre)
                assert abs(float(am[b, i]) - a) <= cr.tol(a), (name, K, b, i, float(am[b, i]), a)
        assert 4 * skipped <= len(refs[K]), (name, K, skipped)


def test_length_zero_returns_the_empty_prefix_with_the_eos_term():
    cs, z, lens, m = nr.make_nlm_case("few_classes")
    assert lens[3] == 0
    dlm = device_nlm(m)
    rows = DeviceRows(m, dlm)
    tok, ln, sc, am = search_nlm(z, lens, cs["C"], 8, 8, dlm, cs["lm_w"], cs["len_bonus"])
    assert ln[3, 0] == 0 and (ln[3, 1:] == -1).all() and (tok[3] == -1).all() and am[3, 0] == 0.0
    assert bits(sc[3, :1])[0] == bits(np.array([nr.eos_term32(rows, (), cs["lm_w"], cs["C"] - 1)], np.float32))[0]


@pytest.mark.parametrize("name", list(cr.CASES))
def test_zero_weight_is_the_ngram_search_at_zero_weight_bit_for_bit(name):
    # (both LM searches need eos = C - 1: the case without an eos runs them with the last class as eos)
    cs, z, lens = cr.make_case(name)
    Cn = cs["C"]
    _, dlm = toy(Cn, (8, 8, 1), 0) if name == "wide_4096" else toy(Cn)
    dng = device_ngram(lm_ref.toy_lm(Cn, 2, 0))
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        for bonus in (0.0, 0.4, -0.25):
            want = search_ngram(z, lens, Cn, K, nbest, dng, 0.0, bonus)
            got = search_nlm(z, lens, Cn, K, nbest, dlm, 0.0, bonus, junk=0xA5)
            for w, g in zip(want, got):
                assert np.array_equal(bits(w), bits(g)), (name, K, bonus)
        tok0, ln0, sc0 = plain_search(z, lens, Cn, K, nbest, 0, Cn - 1)
        tok, ln, sc, am = search_nlm(z, lens, Cn, K, nbest, dlm, 0.0, 0.0)
        assert np.array_equal(tok, tok0) and np.array_equal(ln, ln0), (name, K)
        assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(bits(am), bits(sc)), (name, K)


def test_permuted_batch_bit_for_bit():
    for name, K in (("basic", 8), ("peaky_merge", 3), ("wide", 20)):
        cs, z, lens, m = nr.make_nlm_case(name)
        dlm = device_nlm(m)
        reps = 3 if cs["B"] < 4 else 1
        z, lens = np.concatenate([z] * reps), np.concatenate([lens] * reps)
        perm = np.random.default_rng(5).permutation(len(lens))
        a = search_nlm(z, lens, cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"])
        b = search_nlm(np.ascontiguousarray(z[perm]), lens[perm], cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"], junk=0xA5)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x[perm]), bits(y)), name


def test_junk_in_the_work_buffer_does_not_show():
    for name, K in (("basic", 8), ("few_classes", 8), ("neg_inf", 8)):
        cs, z, lens, m = nr.make_nlm_case(name)
        dlm = device_nlm(m)
        outs = [search_nlm(z, lens, cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"], junk=j) for j in (0x7F, 0xA5, 0xFF)]
        for o in outs[1:]:
            for x, y in zip(outs[0], o):
                assert np.array_equal(bits(x), bits(y)), name


def test_nan_padding_is_never_read():
    cs, z, lens, m = nr.make_nlm_case("basic")
    assert np.isnan(z[0, lens[0]:]).all()
    dlm = device_nlm(m)
    z0 = np.nan_to_num(z, nan=3.0)
    zw = np.full(z.shape[:2] + (z.shape[2] + 3,), np.nan, np.float32)       # NaN columns behind the classes as well
    zw[..., :cs["C"]] = z[..., :cs["C"]]
    a = search_nlm(z, lens, cs["C"], 8, 8, dlm, cs["lm_w"], cs["len_bonus"])
    for other in (z0, zw):
        for x, y in zip(a, search_nlm(other, lens, cs["C"], 8, 8, dlm, cs["lm_w"], cs["len_bonus"])):
            assert np.array_equal(bits(x), bits(y))
    assert np.isfinite(a[2][a[1] >= 0]).all() and np.isfinite(a[3][a[1] >= 0]).all()


def test_refusals():
    l = lib()
    B, Tp, Cn, K = 2, 8, 6, 4
    _, dlm = toy(Cn)
    _, dlm7 = toy(Cn + 1)
    z = torch.zeros(B, Tp, Cn + 1, device=DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_beam_nlm_work_bytes(dlm.h, B, Tp, Cn, K))
    assert nb > int(l.masr_ctc_beam_work_bytes(B, Tp, Cn, K)) > 0 and nb % 256 == 0
    work = torch.zeros(nb + 256, dtype=torch.uint8, device=DEV)
    out = dict(tok=torch.full((B, K, Tp), 77, dtype=torch.int32, device=DEV), ln=torch.full((B, K), 77, dtype=torch.int32, device=DEV),
               sc=torch.full((B, K), 77.0, device=DEV), am=torch.full((B, K), 77.0, device=DEV))

    def call(**kw):
        a = dict(C=Cn, blank=0, eos=Cn - 1, lm=dlm.h, lm_w=0.5, bonus=0.1, work=p(work), wb=nb, am=p(out["am"]), K=K, nbest=K)
        a.update(kw)
        return l.masr_ctc_beam_search_nlm(p(z), Cn + 1, p(lens), B, Tp, a["C"], a["K"], a["nbest"], a["blank"], a["eos"], a["lm"], a["lm_w"], a["bonus"],
                                          a["work"], a["wb"], p(out["tok"]), p(out["ln"]), p(out["sc"]), a["am"], None)

    bad = [(dict(blank=1), b"blank must be 0"), (dict(eos=Cn - 2), b"eos must be C - 1"), (dict(eos=-1), b"eos must be C - 1"),
           (dict(lm=dlm7.h), b"classes differ"), (dict(lm_w=-0.5), b"lm_w"), (dict(lm_w=float("nan")), b"lm_w"),
           (dict(lm_w=float("inf")), b"lm_w"), (dict(bonus=float("nan")), b"len_bonus"), (dict(bonus=float("-inf")), b"len_bonus"),
           (dict(wb=nb - 1), b"work buffer too small"), (dict(lm=None), b"null language model"), (dict(am=None), b"null pointer"),
           (dict(work=C.c_void_p(work.data_ptr() + 4)), b"misaligned"), (dict(K=65), b"beam size K"), (dict(nbest=K + 1), b"nbest"),
           (dict(work=None), b"null pointer")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in l.masr_last_error(), (kw, l.masr_last_error())
    torch.cuda.synchronize()
    for t in out.values():                                          # nothing was launched: the outputs still hold their fill
        assert (t == 77).all()
    assert call() == 0 and call(bonus=-2.0) == 0 and call(lm_w=0.0) == 0
    torch.cuda.synchronize()
    assert (out["ln"][:, 0] >= 0).all()
    assert l.masr_ctc_beam_nlm_work_bytes(dlm.h, B, Tp, Cn, 65) < 0 and l.masr_ctc_beam_nlm_work_bytes(dlm.h, B, Tp, 4097, K) < 0
    assert l.masr_ctc_beam_nlm_work_bytes(None, B, Tp, Cn, K) < 0 and b"null language model" in l.masr_last_error()
