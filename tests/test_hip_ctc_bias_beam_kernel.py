"""masr_ctc_beam_search_bias alone (include/masr.h, DESIGN 5.13: ctc_beam_frames + ctc_beam_sweep<LM, BIAS>) on random logits, toy LMs and
phrase lists against the restatement of tests/ctc_bias_beam_ref.py, with and without an LM.  An utterance is compared where the restatement's
slack is positive; there the N-best token lists and lengths must be equal and the acoustic totals and scores within ctc_beam_ref.tol.  With or
without slack, every returned entry's nbias must be n_final of its tokens exactly and its score the final recomputed in fp32 from the returned
tokens, am and nbias, bit for bit.  A case fails if more than a quarter of its utterances are left out (the CPU test asserts that the
restatement leaves out no more).  Outputs and the work buffer start filled with junk; padded frames and columns are NaN and never read."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_ref  # noqa: E402
import ctc_beam_ref as cr  # noqa: E402
import ctc_bias_beam_ref as br  # noqa: E402
import ctc_lm_beam_ref as lr  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from test_hip_ctc_beam_kernel import search as plain_search  # noqa: E402
from test_hip_ctc_lm_beam_kernel import search_lm  # noqa: E402

DEV = "cuda:0"
JUNK_I = 0x7F7F7F7F


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_lm(lm):
    return None if lm is None else NGramLM(lm["order"], lm["C"], *lm_ref.to_arrays(lm))


def search_bias(z, lens, Cn, K, nbest, dlm, lm_w, len_bonus, dbias, bias_w, junk=0x7F):
    """z [B, Tp, ld] fp32 numpy, lens int32 [B] -> (tokens [B][nbest][Tp], lens, scores, am, nbias [B][nbest]) numpy"""
    B, Tp, ld = z.shape
    l = lib()
    zd = torch.from_numpy(z).to(DEV)
    ld_ = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    nb = int(l.masr_ctc_beam_bias_work_bytes(B, Tp, Cn, K))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), junk, dtype=torch.uint8, device=DEV)
    tok = torch.full((B, nbest, Tp), JUNK_I, dtype=torch.int32, device=DEV)
    ln = torch.full((B, nbest), JUNK_I, dtype=torch.int32, device=DEV)
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    am = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    nbias = torch.full((B, nbest), JUNK_I, dtype=torch.int32, device=DEV)
    rc = l.masr_ctc_beam_search_bias(p(zd), ld, p(ld_), B, Tp, Cn, K, nbest, 0, Cn - 1, dlm.h if dlm is not None else None, lm_w, len_bonus, dbias.h,
                                     bias_w, p(work), nb, p(tok), p(ln), p(sc), p(am), p(nbias), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (tok, ln, sc, am, nbias))


def check_layout_and_scores(name, K, cs, lm, trie, bias_w, tok, ln, sc, am, nbias, nbest):
    """what holds for every utterance, compared or not: the layout, nbias from the returned tokens, and the score from tokens, am and nbias"""
    for b in range(tok.shape[0]):
        live = ln[b] >= 0
        assert live[:live.sum()].all() and (ln[b][~live] == -1).all() and (nbias[b][~live] == -1).all(), (name, K, b)
        assert np.isneginf(sc[b][~live]).all() and np.isneginf(am[b][~live]).all(), (name, K, b)
        for i in range(nbest):
            L = max(int(ln[b, i]), 0)
            assert (tok[b, i, L:] == -1).all() and ((tok[b, i, :L] > 0) & (tok[b, i, :L] < cs["C"] - 1)).all(), (name, K, b, i)
            if not live[i]:
                continue
            h = tuple(tok[b, i, :L].tolist())
            assert int(nbias[b, i]) == bias_ref.count(trie, h), (name, K, b, i, h, int(nbias[b, i]))
            if lm is None:
                want = br.final32(am[b, i], None, None, bias_w, int(nbias[b, i]))
            else:
                want = br.final32(am[b, i], lr.lmacc32(lm, h, cs["lm_w"], cs["len_bonus"]), lr.eos_term32(lm, h, cs["lm_w"], cs["C"] - 1), bias_w,
                                  int(nbias[b, i]))
            assert bits(sc[b, i:i + 1])[0] == bits(np.array([want], np.float32))[0], (name, K, b, i, h, float(sc[b, i]), float(want))
        s = sc[b][live]
        assert (np.diff(s) <= 0).all(), (name, K, b)               # re-ranked by its own finals


@pytest.mark.parametrize("name", list(br.BIAS_CASES))
def test_against_restatement(name):
    cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
    refs = br.case_refs(name)
    dlm, dbias = device_lm(lm), ContextBias(cs["C"], phrases)
    assert dbias.nodes == trie["nodes"]
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        tok, ln, sc, am, nbias = search_bias(z, lens, cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"], dbias, cs["bias_w"])
        check_layout_and_scores(name, K, cs, lm, trie, cs["bias_w"], tok, ln, sc, am, nbias, nbest)
        skipped = 0
        for b, r in enumerate(refs[K]):
            n, live = len(r["nbest"]), int((ln[b] >= 0).sum())
            print(f"{name} K={K} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} live {live}/{n} revocations {r['revocations']} max am err "
                  f"{max((abs(float(am[b, i]) - r['nbest'][i][2]) for i in range(min(n, live))), default=0.0):.3g}")
            if not r["slack"] > 0:
                skipped += 1
                continue
            assert live == n, (name, K, b, ln[b], n)
            for i, (pre, s, a, acc, nf) in enumerate(r["nbest"]):
                assert tuple(tok[b, i, :ln[b, i]].tolist()) == pre, (name, K, b, i, tok[b, i, :ln[b, i]].tolist(), pre)
                assert int(nbias[b, i]) == nf, (name, K, b, i)
                assert abs(float(am[b, i]) - a) <= cr.tol(a), (name, K, b, i, float(am[b, i]), a)
                assert abs(float(sc[b, i]) - s) <= cr.tol(max(abs(a), abs(s))), (name, K, b, i, float(sc[b, i]), s)
        assert 4 * skipped <= len(refs[K]), (name, K, skipped)


@pytest.mark.parametrize("with_lm", [False, True])
def test_length_zero_returns_the_empty_prefix(with_lm):
    cs, z, lens, lm, phrases, trie = br.make_bias_case("few_classes_lm" if with_lm else "few_classes")
    assert lens[3] == 0
    tok, ln, sc, am, nbias = search_bias(z, lens, cs["C"], 8, 8, device_lm(lm), cs["lm_w"], cs["len_bonus"], ContextBias(cs["C"], phrases), cs["bias_w"])
    assert ln[3, 0] == 0 and (ln[3, 1:] == -1).all() and (tok[3] == -1).all() and am[3, 0] == 0.0
    assert nbias[3, 0] == 0 and (nbias[3, 1:] == -1).all()
    want = lr.eos_term32(lm, (), cs["lm_w"], cs["C"] - 1) if with_lm else np.float32(0.0)
    assert bits(sc[3, :1])[0] == bits(np.array([want], np.float32))[0]


@pytest.mark.parametrize("name", ["basic", "few_classes", "peaky_merge", "full_buffer", "wide_367", "neg_inf"])
def test_zero_weight_is_the_unbiased_search_bit_for_bit(name):
    # fl(0 * n) = +0 for every count n >= 0 and s + +0 = s for every score the searches produce (none is -0), so the ranking and the finals
    # are the unbiased ones; nbias is still n_final of the returned tokens
    cs, z, lens, lm = lr.make_lm_case(name)
    phrases = br.make_bias_case(name)[4]
    trie, dbias, dlm = bias_ref.build(phrases), ContextBias(cs["C"], phrases), device_lm(lm)
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        want = search_lm(z, lens, cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"])
        got = search_bias(z, lens, cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"], dbias, 0.0, junk=0xA5)
        for w, g in zip(want, got[:4]):
            assert np.array_equal(bits(w), bits(g)), (name, K)
        tok0, ln0, sc0 = plain_search(z, lens, cs["C"], K, nbest, 0, cs["C"] - 1)
        tok, ln, sc, am, nbias = search_bias(z, lens, cs["C"], K, nbest, None, 123.0, float("nan"), dbias, 0.0, junk=0xA5)   # (lm_w, len_bonus ignored)
        assert np.array_equal(tok, tok0) and np.array_equal(ln, ln0) and np.array_equal(bits(sc), bits(sc0)) and np.array_equal(bits(am), bits(sc)), (name, K)
        for b in range(tok.shape[0]):
            for i in range(nbest):
                if ln[b, i] >= 0:
                    assert int(nbias[b, i]) == bias_ref.count(trie, tok[b, i, :ln[b, i]].tolist()), (name, K, b, i)
                    assert int(got[4][b, i]) == bias_ref.count(trie, got[0][b, i, :got[1][b, i]].tolist()), (name, K, b, i)


def test_permuted_batch_bit_for_bit():
    for name, K in (("basic", 8), ("basic_lm", 8), ("peaky_merge_lm", 3), ("wide_367", 20)):
        cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
        dlm, dbias = device_lm(lm), ContextBias(cs["C"], phrases)
        reps = 3 if cs["B"] < 4 else 1
        z, lens = np.concatenate([z] * reps), np.concatenate([lens] * reps)
        perm = np.random.default_rng(5).permutation(len(lens))
        a = search_bias(z, lens, cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"], dbias, cs["bias_w"])
        b = search_bias(np.ascontiguousarray(z[perm]), lens[perm], cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"], dbias, cs["bias_w"], junk=0xA5)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x[perm]), bits(y)), name


def test_refusals():
    l = lib()
    B, Tp, Cn, K = 2, 8, 6, 4
    dlm, dlm7 = device_lm(lm_ref.toy_lm(Cn, 3, 0)), device_lm(lm_ref.toy_lm(Cn + 1, 2, 0))
    dbias, dbias7 = ContextBias(Cn, [[1, 2], [3]]), ContextBias(Cn + 1, [[1, 2]])
    z = torch.zeros(B, Tp, Cn + 1, device=DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_beam_bias_work_bytes(B, Tp, Cn, K))
    assert nb == int(l.masr_ctc_beam_work_bytes(B, Tp, Cn, K))             # the state lives on chip
    work = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = dict(tok=torch.full((B, K, Tp), 77, dtype=torch.int32, device=DEV), ln=torch.full((B, K), 77, dtype=torch.int32, device=DEV),
               sc=torch.full((B, K), 77.0, device=DEV), am=torch.full((B, K), 77.0, device=DEV),
               nbias=torch.full((B, K), 77, dtype=torch.int32, device=DEV))

    def call(**kw):
        a = dict(C=Cn, K=K, N=K, blank=0, eos=Cn - 1, lm=dlm.h, lm_w=0.5, bonus=0.1, bias=dbias.h, bias_w=2.0, work=p(work), wb=nb, am=p(out["am"]),
                 nbias=p(out["nbias"]), tok=p(out["tok"]), ld=Cn + 1)
        a.update(kw)
        return l.masr_ctc_beam_search_bias(p(z), a["ld"], p(lens), B, Tp, a["C"], a["K"], a["N"], a["blank"], a["eos"], a["lm"], a["lm_w"], a["bonus"],
                                           a["bias"], a["bias_w"], a["work"], a["wb"], a["tok"], p(out["ln"]), p(out["sc"]), a["am"], a["nbias"], None)

    bad = [(dict(bias=None), b"null phrase list"), (dict(bias=None, lm=None), b"null phrase list"),
           (dict(bias=dbias7.h), b"phrase list's classes differ"), (dict(bias_w=-0.5), b"bias_w"), (dict(bias_w=float("nan")), b"bias_w"),
           (dict(bias_w=float("inf")), b"bias_w"), (dict(nbias=None), b"null pointer"), (dict(am=None), b"null pointer"),
           (dict(am=None, lm=None), b"null pointer"), (dict(tok=None), b"null pointer"),
           # blank 0 and eos C - 1 are required with or without an LM
           (dict(blank=1), b"blank must be 0"), (dict(eos=Cn - 2), b"eos must be C - 1"), (dict(eos=-1), b"eos must be C - 1"),
           (dict(lm=None, blank=1), b"blank must be 0 with a phrase list"), (dict(lm=None, eos=Cn - 2), b"eos must be C - 1 with a phrase list"),
           (dict(lm=None, eos=-1), b"eos must be C - 1 with a phrase list"),
           # everything the underlying searches refuse
           (dict(lm=dlm7.h), b"language model's classes differ"), (dict(lm_w=-0.5), b"lm_w"), (dict(lm_w=float("nan")), b"lm_w"),
           (dict(bonus=float("nan")), b"len_bonus"), (dict(wb=nb - 1), b"work buffer too small"), (dict(K=0), b"beam size K"), (dict(K=65), b"beam size K"),
           (dict(N=0), b"nbest"), (dict(N=K + 1), b"nbest"), (dict(C=4097), b"C <= 4096"), (dict(ld=Cn - 1), b"ld >= C")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in l.masr_last_error(), (kw, l.masr_last_error())
    torch.cuda.synchronize()
    for t in out.values():                                          # nothing was launched: the outputs still hold their fill
        assert (t == 77).all()
    # without an LM lm_w and len_bonus are ignored, whatever they hold
    assert call() == 0 and call(bias_w=0.0) == 0 and call(lm=None, lm_w=-1.0, bonus=float("nan")) == 0
    torch.cuda.synchronize()
    assert (out["ln"][:, 0] >= 0).all() and (out["nbias"][:, 0] >= 0).all()
    assert l.masr_ctc_beam_bias_work_bytes(B, Tp, Cn, 65) < 0 and l.masr_ctc_beam_bias_work_bytes(B, Tp, 4097, K) < 0
