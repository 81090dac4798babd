"""The phrase-biased step kernels alone through include/masr_test.h:
  masr_test_beam_bias_rows          the biased row stage, top-K and pre-beam, with and without the n-gram LM, on random logits: the state out
                                    equals bias_ref exactly; g and the score equal numpy bit for bit from the kernel's own lp / LM term (pre-beam:
                                    pre_b bit for bit from the state alone); the ranking equals numpy's wherever neighbours are more than 1e-4
                                    apart; hand-made states cover a phrase that is a proper prefix of another, a state 63 tokens deep in a
                                    64-token phrase (dn = -63), the t >= maxlen step, class 0 and eos; at bias_w = 0 the lists are
                                    masr_test_beam_lm_topk's / masr_test_joint_lm_prebeam's bit for bit
  masr_test_beam_select_bias        the attention beam's select with the stop bound of bias_w
  masr_test_beam_select_nbest_bias  the N-best select with the bound of max(len_bonus, 0) + bias_w
The selects do integer and compare work only, so they equal a Python restatement exactly; their cases include utterances that the new bound
keeps running where the old rule would have finished them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_ref  # noqa: E402
import lm_ref  # noqa: E402
from decode_util import C_SMALL  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402
from test_hip_joint_lm_kernels import random_lists  # noqa: E402
from test_hip_lm_kernels import _hyp, toy  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
EOS = C_SMALL - 1
LONG = [1 + (i * 5) % (C_SMALL - 2) for i in range(64)]      # one 64-token phrase
# [3, 4] is a proper prefix of [3, 4, 5, 6]; [4, 5] starts inside it; the long phrase shares no first token with the others
PHRASES = [[3, 4], [3, 4, 5, 6], [4, 5], [7], [8, 9, 10], LONG]
assert LONG[0] == 1 and all(p[0] != 1 for p in PHRASES[:-1])


@pytest.fixture(scope="module")
def L():
    return _cabi.lib()


@pytest.fixture(scope="module")
def trie():
    return bias_ref.build(PHRASES)


@pytest.fixture(scope="module")
def bias():
    return ContextBias(C_SMALL, PHRASES)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def node_of(trie, h):
    return bias_ref.state_of(trie, h)[0]


def row_inputs(trie, B, K, t, seed, minlen_on, at_maxlen):
    """random logits (a pad column that would win every list), scores with one dead row, minlen, maxlen, histories whose last tokens are drawn
    from the phrases' tokens and the other classes alike, and the parents' states: reachable ones of random hypotheses, and in fixed rows the
    hand-set ones -- inside [3, 4, 5, 6] behind the finished [3, 4], and 63 tokens deep in the 64-token phrase"""
    rng = np.random.RandomState(seed)
    R = B * K
    ld = 128
    z = np.full((R, ld), 100.0, dtype=F32)
    z[:, :C_SMALL] = (3.0 * rng.randn(R, C_SMALL)).astype(F32)
    score = (-20.0 * rng.rand(R)).astype(F32)
    dead = 3 + int(rng.randint(R - 3)) if R > 3 else -1       # (rows 0 .. 2 carry the hand-set states)
    if dead >= 0:
        score[dead] = -np.inf
    minlen = np.full(B, t + 1 if minlen_on else 0, dtype=np.int32)
    minlen[0] = 0 if minlen_on else t + 1                    # one utterance the other way
    maxlen = np.full(B, t if at_maxlen else t + 5, dtype=np.int32)
    maxlen[B - 1] = t + 5 if at_maxlen else t                # and one the other way here
    n = max(t - 1, 1)
    tok_hist = rng.randint(0, C_SMALL, size=(n, R)).astype(np.int32)       # class 0 and eos occur as last tokens too
    par_hist = ((np.arange(R) // K * K)[None, :] + rng.randint(K, size=(n, R))).astype(np.int32)
    state_in = np.zeros((R, 2), np.int32)
    if t > 1:
        for r in range(R):                                   # the state of parent row r: a random hypothesis of t - 2 tokens made of phrase pieces
            h = []
            while len(h) < t - 2:
                h += PHRASES[rng.randint(len(PHRASES) - 1)] if rng.rand() < 0.7 else [int(rng.randint(1, EOS))]
            state_in[r] = bias_ref.state_of(trie, h[:t - 2])
        # the hand-set rows, each its own parent (only the step's own arithmetic is under test: a state need not match the row's history)
        hand = {0: ([3, 4], 5, 2),                           # -> inside [3, 4, 5, 6] behind the finished [3, 4]: revoke 1
                1: (LONG[:62], LONG[62], 70)}                # -> 63 tokens deep in the 64-token phrase: revoke 63, dn = -63 on a break
        if R > 2:
            hand[2] = ([3], 4, 1)                            # -> a finished phrase that may go on: revoke 0
        for r, (h, c, n_cred) in hand.items():
            state_in[r] = (node_of(trie, h), n_cred)
            tok_hist[t - 2, r], par_hist[t - 2, r] = c, r
    return z, score, dead, minlen, maxlen, tok_hist, par_hist, state_in


def dn_ref(trie, st, c, ends):
    nst = bias_ref.step(trie, st, c)
    return nst[1] - st[1] - (trie["revoke"][nst[0]] if ends and c != EOS else 0)


def run_rows(L, bias, trie, lm_pair, B, K, t, lm_w, bias_w, seed, minlen_on, at_maxlen, pre):
    """-> the kernel's outputs and the numpy expectation's pieces, after asserting state, terms and bits"""
    z, score, dead, minlen, maxlen, tok_hist, par_hist, state_in = row_inputs(trie, B, K, t, seed, minlen_on, at_maxlen)
    d, lm = lm_pair if lm_pair else (None, None)
    R, Pw = B * K, max(1, 3 * K // 2)
    W = Pw if pre else K
    hist = (dev(tok_hist), dev(par_hist), dev(state_in)) if t > 1 else (None, None, None)
    so = torch.full((R, 2), -9, dtype=torch.int32, device=DEV)
    lt = torch.full((R, W), -7, dtype=torch.int32, device=DEV)
    f1, f2, f3 = (torch.full((R, W), float("nan"), device=DEV) for _ in range(3))
    d_min, d_max, d_z, d_score = dev(minlen), dev(maxlen), dev(z), dev(score)      # (kept alive over the call)
    args = (lm.h if lm else None, bias.h, float(lm_w), float(bias_w), B, K, t, P(d_min), P(d_max), P(d_z), z.shape[1], P(d_score),
            P(hist[0]), P(hist[1]), P(hist[2]), P(so))
    outs = (None, None, P(lt), P(f1), P(f2), P(f3)) if pre else (P(lt), P(f1), None, None, None, None)
    _cabi.check(L.masr_test_beam_bias_rows(*args, *outs, S()), "masr_test_beam_bias_rows")
    so, lt, f1, f2, f3 = (x.cpu().numpy() for x in (so, lt, f1, f2, f3))
    seen = {"dn": set(), "cls": set(), "pos": 0, "clear": 0}
    for r in range(R):
        u = r // K
        if r == dead:
            assert (so[r] == 0).all()                        # nothing is stored for a dead row (the entry's buffer starts as zero)
            if pre:
                assert (lt[r] == -7).all()
            else:
                assert (lt[r] == -1).all() and np.isneginf(f1[r]).all()
            continue
        if t > 1:
            par, tok = int(par_hist[t - 2, r]), int(tok_hist[t - 2, r])
            st = bias_ref.step(trie, tuple(int(v) for v in state_in[par]), tok)
        else:
            st = bias_ref.ROOT
        assert tuple(so[r]) == st, (r, so[r], st)
        last = t >= maxlen[u]
        dn = np.array([dn_ref(trie, st, c, last) for c in range(C_SMALL)])
        b = (F32(bias_w) * dn.astype(F32)).astype(F32)
        zr = z[r, :C_SMALL].astype(np.float64)
        lp64 = zr - (zr.max() + math.log(np.exp(zr - zr.max()).sum()))
        lm32 = lm_ref.lm_row32(d, lm_ref.lm_context(d, _hyp(tok_hist, par_hist, r, t))) if d else np.zeros(C_SMALL, F32)
        g64 = lp64 + float(F32(lm_w)) * lm32.astype(np.float64) + b.astype(np.float64)
        no_eos = minlen[u] > t - 1
        if pre:
            g64[0] = -np.inf
        if no_eos:
            g64[EOS] = -np.inf
        order = np.lexsort((np.arange(C_SMALL), -g64))[:W]
        n_live = min(W, int(np.isfinite(g64).sum()))
        assert (lt[r, n_live:] == -1).all(), (r, lt[r])
        gs = g64[order]
        for i in range(n_live):
            c = int(lt[r, i])
            assert 0 <= c < C_SMALL and not (pre and c == 0) and not (c == EOS and no_eos), (r, i, c)
            seen["dn"].add(int(dn[c])); seen["cls"].add(c); seen["pos"] += 1
            if pre:                                          # lp, the LM term and the bias term, each as the prefix kernel will read it
                assert abs(float(f1[r, i]) - lp64[c]) <= 1e-5 + 1e-6 * abs(lp64[c]), (r, i, c)
                assert bits(f2[r, i]) == bits(F32(F32(lm_w) * lm32[c]) if d else F32(0)), (r, i, c, f2[r, i])
                assert bits(f3[r, i]) == bits(b[c]), (r, i, c, f3[r, i], b[c], dn[c])
            else:                                            # score = fl(ps + g), g = fl(f + b): g is recovered from the lists at bias_w = 0 below;
                f = lp64[c] + float(F32(lm_w)) * float(lm32[c])      # here to the rounding of lp
                assert abs(float(f1[r, i]) - (float(score[r]) + f + float(b[c]))) <= 2e-5 + 2e-6 * abs(float(f1[r, i])), (r, i, c, f1[r, i])
            if (i == 0 or gs[i - 1] - gs[i] > 1e-4) and (i + 1 >= len(gs) or gs[i] - gs[i + 1] > 1e-4):
                seen["clear"] += 1
                assert c == int(order[i]), (r, i, c, int(order[i]), gs[max(i - 1, 0):i + 2])
        assert len(set(lt[r, :n_live].tolist())) == n_live
    return dict(z=z, score=score, dead=dead, minlen=minlen, maxlen=maxlen, tok_hist=tok_hist, par_hist=par_hist, state_in=state_in, state_out=so,
                tok=lt, f1=f1, f2=f2, f3=f3, seen=seen)


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("pre", [False, True])
def test_biased_row_stage(L, bias, trie, with_lm, pre):
    lm_pair = toy(C_SMALL, 3) if with_lm else None
    dns, classes, pos, clear = set(), set(), 0, 0
    for K in (1, 3, 4):
        for t in (1, 2, 5):
            for minlen_on, at_maxlen in ((False, False), (True, True)):
                o = run_rows(L, bias, trie, lm_pair, 2, K, t, 0.5 if with_lm else 0.0, 1.5, 1000 * K + 10 * t + minlen_on, minlen_on, at_maxlen, pre)
                s = o["seen"]
                dns |= s["dn"]; classes |= s["cls"]; pos += s["pos"]; clear += s["clear"]
    print(f"lm {with_lm}, pre-beam {pre}: {pos} list positions, {clear} with clear neighbours; dn values met {sorted(dns)}")
    assert clear >= 0.8 * pos
    assert 1 in dns and 0 in dns and -1 in dns and min(dns) <= -62, sorted(dns)
    assert EOS in classes and (pre or 0 in classes)


def test_hand_set_states_step_by_step(L, bias, trie):
    """every class from the hand-set states, K = 12 so that no class falls off the list: dn of the proper-prefix state, of the deep state (-63 on a
    break, -62 on a break that restarts a phrase, +1 on the 64th token), and what the t >= maxlen step takes off as well"""
    K, B, t = C_SMALL, 1, 3
    for at_max in (False, True):
        z = np.zeros((K, 128), F32)
        z[:, C_SMALL:] = 100.0
        score = np.zeros(K, F32)
        tok_hist = np.zeros((2, K), np.int32)
        par_hist = np.arange(K, dtype=np.int32)[None, :].repeat(2, 0)
        state_in = np.zeros((K, 2), np.int32)
        cases = {0: ([3, 4], 5, 2), 1: (LONG[:62], LONG[62], 70), 2: ([3], 4, 1), 3: ([8, 9], 10, 2), 4: ([8], 0, 1), 5: ([8], EOS, 1)}
        for r, (h, c, n) in cases.items():
            state_in[r] = (node_of(trie, h), n)
            tok_hist[1, r] = c
        so = torch.zeros((K, 2), dtype=torch.int32, device=DEV)
        lt = torch.full((K, K), -7, dtype=torch.int32, device=DEV)
        ls = torch.full((K, K), float("nan"), device=DEV)
        maxlen = np.array([t if at_max else t + 4], np.int32)
        d_in = [dev(a) for a in (np.zeros(1, np.int32), maxlen, z, score, tok_hist, par_hist, state_in)]      # (kept alive over the call)
        _cabi.check(L.masr_test_beam_bias_rows(None, bias.h, 0.0, 2.0, B, K, t, P(d_in[0]), P(d_in[1]), P(d_in[2]), 128, P(d_in[3]),
                                               P(d_in[4]), P(d_in[5]), P(d_in[6]), P(so), P(lt), P(ls), None, None, None, None, S()),
                    "masr_test_beam_bias_rows")
        so, lt, ls = so.cpu().numpy(), lt.cpu().numpy(), ls.cpu().numpy()
        lp = F32(-math.log(C_SMALL))
        for r, (h, c, n) in cases.items():
            st = bias_ref.step(trie, (node_of(trie, h), n), c)
            assert tuple(so[r]) == st, (r, so[r], st)
            got = {int(cl): sc for cl, sc in zip(lt[r], ls[r])}
            assert sorted(got) == list(range(C_SMALL))
            for cl in range(C_SMALL):
                dn = dn_ref(trie, st, cl, at_max)
                # uniform logits: lp is one value up to its rounding, the bias term an exact multiple of 2
                assert abs(float(got[cl]) - (float(lp) + 2.0 * dn)) <= 1e-5, (at_max, r, cl, got[cl], dn)
        # the deep state: row 1 sits 63 tokens into the 64-token phrase
        st = tuple(so[1])
        assert trie["revoke"][st[0]] == 63
        assert dn_ref(trie, st, LONG[63], False) == 1 and dn_ref(trie, st, 0, False) == -63 and dn_ref(trie, st, EOS, at_max) == -63
        assert dn_ref(trie, st, 3, False) == -62 and dn_ref(trie, st, 3, True) == -63       # restarts [3, ..]; at maxlen that token goes back too
        assert dn_ref(trie, tuple(so[0]), 6, False) == 1 and dn_ref(trie, tuple(so[0]), 2, False) == -1      # [3, 4] stays earned


@pytest.mark.parametrize("pre", [False, True])
def test_bias_weight_zero_is_the_lm_row_stage(L, bias, trie, pre):
    lm_pair = toy(C_SMALL, 3)
    for K, t in ((1, 1), (3, 2), (4, 5)):
        o = run_rows(L, bias, trie, lm_pair, 2, K, t, 0.5, 0.0, 77 + K, t == 2, t == 5, pre)
        R, W = 2 * K, max(1, 3 * K // 2) if pre else K
        dz, ds, dm = dev(o["z"]), dev(o["score"]), dev(o["minlen"])
        dt, dp = (dev(o["tok_hist"]), dev(o["par_hist"])) if t > 1 else (None, None)
        lt = torch.full((R, W), -7, dtype=torch.int32, device=DEV)
        f1, f2 = (torch.full((R, W), float("nan"), device=DEV) for _ in range(2))
        if pre:
            _cabi.check(L.masr_test_joint_lm_prebeam(lm_pair[1].h, 0.5, 2, K, t, P(dm), P(dz), 128, P(ds), P(dt), P(dp), P(lt), P(f1), P(f2), S()),
                        "masr_test_joint_lm_prebeam")
        else:
            _cabi.check(L.masr_test_beam_lm_topk(lm_pair[1].h, 0.5, 2, K, t, P(dm), P(dz), 128, P(ds), P(dt), P(dp), P(lt), P(f1), S()),
                        "masr_test_beam_lm_topk")
        assert (lt.cpu().numpy() == o["tok"]).all()
        assert (bits(f1.cpu().numpy()) == bits(o["f1"])).all()
        if pre:
            assert (bits(f2.cpu().numpy()) == bits(o["f2"])).all()
            live = o["tok"] >= 0
            assert (np.abs(o["f3"][live]) == 0).all()        # fl(0 * dn): a zero of either sign


def test_score_bits_from_the_unbiased_lists(L, bias, trie):
    """top-K at K = C: every class is listed, so the biased score of class c is fl(ps + fl(f(c) + b)) bit for bit with f(c) recovered exactly
    from the bias_w = 0 run of the same inputs -- no multiply-add, one rounding per term"""
    lm_pair = toy(C_SMALL, 3)
    K, t = C_SMALL, 2
    for with_lm in (False, True):
        pair = lm_pair if with_lm else None
        lw = 0.5 if with_lm else 0.0
        o0 = run_rows(L, bias, trie, pair, 1, K, t, lw, 0.0, 5, False, False, True)      # the pre-beam gives lp and the LM term themselves
        o1 = run_rows(L, bias, trie, pair, 1, K, t, lw, 1.5, 5, False, False, False)
        o2 = run_rows(L, bias, trie, pair, 1, K, t, lw, 1.5, 5, False, False, True)
        n = 0
        for r in range(K):
            if r == o1["dead"]:
                continue
            lp = {int(c): v for c, v in zip(o0["tok"][r], o0["f1"][r]) if c >= 0}
            lmt = {int(c): v for c, v in zip(o0["tok"][r], o0["f2"][r]) if c >= 0}
            b = {int(c): v for c, v in zip(o2["tok"][r], o2["f3"][r]) if c >= 0}
            for c, sc in zip(o1["tok"][r], o1["f1"][r]):
                c = int(c)
                if c not in lp or c not in b:                # (class 0 is no pre-beam candidate)
                    continue
                f = F32(lp[c] + lmt[c]) if with_lm else lp[c]
                want = F32(o1["score"][r] + F32(f + b[c]))
                assert bits(sc) == bits(want), (with_lm, r, c, sc, want)
                n += 1
        assert n >= 8 * (K - 1)


# ---------------------------------------------------------------- the selects
def bound32(run_best, left, gain):
    return F32(F32(run_best) + F32(F32(left) * F32(gain)))


def select_att_ref(B, K, Cn, t, maxlen, bias_w, lt, ls, st):
    eos = Cn - 1
    for u in range(B):
        if st["fin"][u]:
            continue
        r0 = u * K
        cands = []
        for k in range(K):
            for h in range(K):
                if lt[r0 + k, h] < 0 or ls[r0 + k, h] == -np.inf:
                    break
                cands.append((ls[r0 + k, h], k, h))
        cands.sort(key=lambda e: (-float(e[0]), e[1], e[2]))
        j, run_best = 0, None
        for sc, k, h in cands[:K]:
            r = r0 + k
            if lt[r, h] == eos:
                if sc > st["best_score"][u]:
                    st["best_score"][u], st["best_len"][u], st["best_row"][u] = sc, t - 1, r
                continue
            row = r0 + j
            j += 1
            st["tok"][row], st["par"][row], st["score"][row] = lt[r, h], r, sc
            run_best = sc if run_best is None else run_best
            if t >= maxlen[u] and sc > st["best_score"][u]:
                st["best_score"][u], st["best_len"][u], st["best_row"][u] = sc, t, row
        for k in range(j, K):
            st["tok"][r0 + k], st["par"][r0 + k], st["score"][r0 + k] = 0, r0 + k, -np.inf
        old = j == 0 or t >= maxlen[u] or st["best_score"][u] >= run_best
        new = j == 0 or t >= maxlen[u] or st["best_score"][u] >= bound32(run_best, maxlen[u] - t, bias_w)
        st["kept"] += int(old and not new)
        if new:
            st["fin"][u] = 1


def att_lists(rng, B, K, Cn, p_eos):
    R = B * K
    lt = np.full((R, K), -1, np.int32)
    ls = np.full((R, K), -np.inf, F32)
    for r in range(R):
        sc = np.sort((-0.25 * rng.randint(0, 24, size=K)).astype(F32))[::-1]
        tok = rng.randint(0, Cn - 1, size=K)
        tok[rng.rand(K) < p_eos] = Cn - 1
        lt[r], ls[r] = tok, sc
    return lt, ls


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("bias_w", [0.0, 0.25, 1.5])
def test_select_with_the_bias_bound(L, K, bias_w):
    Cn, B, t0 = 9, 6, 3
    rng = np.random.RandomState(10 * K + int(4 * bias_w))
    R = B * K
    maxlen = np.array([9, t0 + 1, 9, 30, 30, 5], np.int32)
    st = {"fin": np.array([1, 0, 0, 0, 0, 0], np.int32), "tok": np.full(R, -5, np.int32), "par": np.full(R, -5, np.int32),
          "score": np.full(R, 7.0, F32), "best_score": np.full(B, -np.inf, F32), "best_len": np.zeros(B, np.int32),
          "best_row": (np.arange(B) * K).astype(np.int32), "kept": 0}
    for step in range(4):
        t = t0 + step
        lt, ls = att_lists(rng, B, K, Cn, 0.35)
        d = {k: dev(v.copy()) for k, v in st.items() if k != "kept"}
        step_out = torch.zeros(2, dtype=torch.int32, device=DEV)
        d_max, d_lt, d_ls = dev(maxlen), dev(lt), dev(ls)
        _cabi.check(L.masr_test_beam_select_bias(B, K, Cn, t, P(d_max), float(bias_w), P(d_lt), P(d_ls), P(d["score"]), P(d["fin"]),
                                                 P(d["best_score"]), P(d["best_len"]), P(d["best_row"]), P(d["tok"]), P(d["par"]), P(step_out), S()),
                    "masr_test_beam_select_bias")
        select_att_ref(B, K, Cn, t, maxlen, bias_w, lt, ls, st)
        assert step_out.cpu().tolist() == [t + 1, 0]
        for k, v in st.items():
            if k == "kept":
                continue
            got = d[k].cpu().numpy()
            assert (bits(got) == bits(v)).all() if v.dtype == F32 else (got == v).all(), (K, bias_w, step, k, got, v)
    print(f"K = {K}, bias_w = {bias_w}: {st['kept']} utterance steps kept running by the bound, finished {int(st['fin'].sum())} of {B}")
    assert st["fin"][0] == 1 and st["fin"][1] == 1
    if bias_w == 0.0:
        assert st["kept"] == 0                               # today's comparison
    if bias_w == 1.5 and K >= 3:                             # (K = 1: one candidate a step, an ended one is never overtaken here)
        assert st["kept"] >= 1


def select_nbest_ref(B, K, N, Cn, t, maxlen, bonus, bias_w, lt, ls, lpsi, lslot, st):
    Pw, eos = lt.shape[1], Cn - 1
    for u in range(B):
        if st["fin"][u]:
            continue
        r0 = u * K
        cands = []
        for k in range(K):
            for h in range(Pw):
                if lt[r0 + k, h] < 0 or ls[r0 + k, h] == -np.inf:
                    break
                cands.append((ls[r0 + k, h], k, h))
        cands.sort(key=lambda e: (-float(e[0]), e[1], e[2]))
        old = [(st["nb_score"][u, i], st["nb_len"][u, i], st["nb_row"][u, i]) for i in range(N) if st["nb_len"][u, i] >= 0]
        new, j, run_best = [], 0, None
        for sc, k, h in cands[:K]:
            r = r0 + k
            if lt[r, h] == eos:
                new.append((sc, t - 1, r))
                continue
            row = r0 + j
            j += 1
            st["tok"][row], st["par"][row], st["score"][row] = lt[r, h], r, sc
            st["psi"][row], st["src"][row] = lpsi[r, h], r * Pw + lslot[r, h]
            run_best = sc if run_best is None else run_best
            if t >= maxlen[u]:
                new.append((sc, t, row))
        for k in range(j, K):
            st["tok"][r0 + k], st["par"][r0 + k], st["score"][r0 + k] = 0, r0 + k, -np.inf
        merged = sorted([(e, 0, i) for i, e in enumerate(old)] + [(e, 1, i) for i, e in enumerate(new)], key=lambda m: (-float(m[0][0]), m[1], m[2]))[:N]
        for i, (e, _, _) in enumerate(merged):
            st["nb_score"][u, i], st["nb_len"][u, i], st["nb_row"][u, i] = e
        done = was = j == 0 or t >= maxlen[u]
        if not done and len(merged) == N:
            gain = F32(max(bonus, 0.0))
            was = bool(merged[N - 1][0][0] >= bound32(run_best, maxlen[u] - t, gain))
            done = bool(merged[N - 1][0][0] >= bound32(run_best, maxlen[u] - t, F32(gain + F32(bias_w))))
        st["kept"] += int(was and not done)
        if done:
            st["fin"][u] = 1


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("bonus, bias_w", [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (-0.5, 1.5), (0.5, 1.5)])
def test_select_nbest_with_the_bias_bound(L, K, bonus, bias_w):
    Cn, B, t0 = 9, 6, 3
    for N in sorted({1, K}):
        rng = np.random.RandomState(100 * K + 10 * N + int(2 * bias_w))
        R = B * K
        maxlen = np.array([9, t0 + 1, 9, 30, 30, 5], np.int32)
        st = {"fin": np.array([1, 0, 0, 0, 0, 0], np.int32), "tok": np.full(R, -5, np.int32), "par": np.full(R, -5, np.int32),
              "score": np.full(R, 7.0, F32), "psi": np.full(R, 7.0, F32), "src": np.full(R, -5, np.int32),
              "nb_score": np.full((B, N), -np.inf, F32), "nb_len": np.full((B, N), -1, np.int32),
              "nb_row": (np.arange(B) * K)[:, None].repeat(N, 1).astype(np.int32), "kept": 0}
        for step in range(4):
            t = t0 + step
            live = [K, K, max(1, K // 3) if step else K, K, K, K]
            lt, ls, lpsi, lslot = random_lists(rng, B, K, Cn, live, p_eos=0.3 if step < 3 else 0.9, fill=1.0 if step != 2 else 0.2)
            d = {k: dev(v.copy()) for k, v in st.items() if k != "kept"}
            step_out = torch.zeros(2, dtype=torch.int32, device=DEV)
            d_in = [dev(a) for a in (maxlen, lt, ls, lpsi, lslot)]
            _cabi.check(L.masr_test_beam_select_nbest_bias(B, K, N, Cn, t, P(d_in[0]), float(bonus), float(bias_w), P(d_in[1]), P(d_in[2]), P(d_in[3]),
                                                           P(d_in[4]), P(d["score"]), P(d["psi"]), P(d["src"]), P(d["fin"]), P(d["nb_score"]),
                                                           P(d["nb_len"]), P(d["nb_row"]), P(d["tok"]), P(d["par"]), P(step_out), S()),
                        "masr_test_beam_select_nbest_bias")
            select_nbest_ref(B, K, N, Cn, t, maxlen, bonus, bias_w, lt, ls, lpsi, lslot, st)
            assert step_out.cpu().tolist() == [t + 1, 0]
            for k, v in st.items():
                if k == "kept":
                    continue
                got = d[k].cpu().numpy()
                assert (bits(got) == bits(v)).all() if v.dtype == F32 else (got == v).all(), (K, N, bonus, bias_w, step, k, got, v)
        print(f"K = {K}, N = {N}, bonus {bonus}, bias_w {bias_w}: {st['kept']} utterance steps kept running by the bias term of the bound")
        assert st["fin"][0] == 1 and st["fin"][1] == 1 and (st["nb_len"][0] == -1).all()
        if bias_w == 0.0:
            assert st["kept"] == 0
        if bias_w == 1.5 and N == 1 and K >= 3:
            assert st["kept"] >= 1
