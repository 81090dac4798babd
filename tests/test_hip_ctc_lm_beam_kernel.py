"""masr_ctc_beam_search_lm alone (include/masr.h, DESIGN 5.6: ctc_beam_frames + ctc_beam_sweep<LM>) on random logits and toy LMs against the
restatement of tests/ctc_lm_beam_ref.py.  An utterance is compared where the restatement's slack is positive; there the N-best token lists
and lengths must be equal and the acoustic totals within 1e-4 + 2e-5 |am|.  With or without slack, every returned entry's fused score must
be fl(fl(am + lmacc(tokens)) + fl(lm_w * lm(eos | tokens))) bit for bit, recomputed in fp32 from the returned tokens and am.  A case fails
if more than a quarter of its utterances are left out (the CPU test asserts that the restatement leaves out no more).  Outputs and the
work buffer start filled with junk; padded frames and columns are NaN and never read."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_beam_ref as cr  # noqa: E402
import ctc_lm_beam_ref as lr  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from test_hip_ctc_beam_kernel import search as plain_search  # noqa: E402

DEV = "cuda:0"


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def device_lm(lm):
    return NGramLM(lm["order"], lm["C"], *lm_ref.to_arrays(lm))


def search_lm(z, lens, Cn, K, nbest, dlm, lm_w, len_bonus, junk=0x7F):
    """z [B, Tp, ld] fp32 numpy, lens int32 [B] -> (tokens [B][nbest][Tp], lens [B][nbest], scores [B][nbest], am [B][nbest]) numpy"""
    B, Tp, ld = z.shape
    l = lib()
    zd = torch.from_numpy(z).to(DEV)
    ld_ = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    nb = int(l.masr_ctc_beam_lm_work_bytes(B, Tp, Cn, K))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), junk, dtype=torch.uint8, device=DEV)
    tok = torch.full((B, nbest, Tp), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    ln = torch.full((B, nbest), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    am = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    rc = l.masr_ctc_beam_search_lm(p(zd), ld, p(ld_), B, Tp, Cn, K, nbest, 0, Cn - 1, dlm.h, lm_w, len_bonus, p(work), nb, p(tok), p(ln), p(sc),
                                   p(am), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), am.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_layout_and_scores(name, K, cs, lm, tok, ln, sc, am, nbest):
    """what holds for every utterance, compared or not: the layout, and the fused score from the returned tokens and am, bit for bit"""
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
            want = lr.final32(am[b, i], lr.lmacc32(lm, h, cs["lm_w"], cs["len_bonus"]), lr.eos_term32(lm, h, cs["lm_w"], cs["C"] - 1))
            assert bits(sc[b, i:i + 1])[0] == bits(np.array([want], np.float32))[0], (name, K, b, i, h, float(sc[b, i]), float(want))
        s = sc[b][live]
        assert (np.diff(s) <= 0).all(), (name, K, b)               # re-ranked by its own finals


@pytest.mark.parametrize("name", list(lr.LM_CASES))
def test_against_restatement(name):
    cs, z, lens, lm = lr.make_lm_case(name)
    refs = lr.case_refs(name)
    dlm = device_lm(lm)
    if name == "wide_367":
        assert lib().masr_test_lm_max_probe(dlm.h) >= 2
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        tok, ln, sc, am = search_lm(z, lens, cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"])
        check_layout_and_scores(name, K, cs, lm, tok, ln, sc, am, nbest)
        skipped = 0
        for b, r in enumerate(refs[K]):
            n, live = len(r["nbest"]), int((ln[b] >= 0).sum())
            print(f"{name} K={K} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} live {live}/{n} max am err "
                  f"{max((abs(float(am[b, i]) - r['nbest'][i][2]) for i in range(min(n, live))), default=0.0):.3g}")
            if not r["slack"] > 0:
                skipped += 1
                continue
            assert live == n, (name, K, b, ln[b], n)
            for i, (pre, s, a, acc) in enumerate(r["nbest"]):
                assert tuple(tok[b, i, :ln[b, i]].tolist()) == pre, (name, K, b, i, tok[b, i, :ln[b, i]].tolist(), pre)
                assert abs(float(am[b, i]) - a) <= cr.tol(a), (name, K, b, i, float(am[b, i]), a)
                assert abs(float(sc[b, i]) - s) <= cr.tol(max(abs(a), abs(s))), (name, K, b, i, float(sc[b, i]), s)
        assert 4 * skipped <= len(refs[K]), (name, K, skipped)


def test_length_zero_returns_the_empty_prefix_with_the_eos_term():
    cs, z, lens, lm = lr.make_lm_case("few_classes")
    assert lens[3] == 0
    tok, ln, sc, am = search_lm(z, lens, cs["C"], 8, 8, device_lm(lm), cs["lm_w"], cs["len_bonus"])
    assert ln[3, 0] == 0 and (ln[3, 1:] == -1).all() and (tok[3] == -1).all() and am[3, 0] == 0.0
    assert bits(sc[3, :1])[0] == bits(np.array([lr.eos_term32(lm, (), cs["lm_w"], cs["C"] - 1)], np.float32))[0]


@pytest.mark.parametrize("name", list(cr.CASES))
def test_zero_weight_is_the_plain_search_bit_for_bit(name):
    # fl(0 * x) = -0 for the LM's x <= 0, -0 + +0 = +0, so lmacc stays +0 and s + 0 = s; the eos term is -0 and s + -0 = s
    # (the LM search needs eos = C - 1: the case without an eos runs both searches with the last class as eos)
    cs, z, lens = cr.make_case(name)
    dlm = device_lm(lm_ref.toy_lm(cs["C"], 3, 0))
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        tok0, ln0, sc0 = plain_search(z, lens, cs["C"], K, nbest, 0, cs["C"] - 1)
        tok, ln, sc, am = search_lm(z, lens, cs["C"], K, nbest, dlm, 0.0, 0.0, junk=0xA5)
        assert np.array_equal(tok, tok0) and np.array_equal(ln, ln0), (name, K)
        assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(bits(am), bits(sc)), (name, K)


def test_permuted_batch_bit_for_bit():
    for name, K in (("basic", 8), ("peaky_merge", 3), ("wide_367", 20)):
        cs, z, lens, lm = lr.make_lm_case(name)
        dlm = device_lm(lm)
        reps = 3 if cs["B"] < 4 else 1
        z, lens = np.concatenate([z] * reps), np.concatenate([lens] * reps)
        perm = np.random.default_rng(5).permutation(len(lens))
        a = search_lm(z, lens, cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"])
        b = search_lm(np.ascontiguousarray(z[perm]), lens[perm], cs["C"], K, K, dlm, cs["lm_w"], cs["len_bonus"], junk=0xA5)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x[perm]), bits(y)), name


def test_refusals():
    l = lib()
    B, Tp, Cn, K = 2, 8, 6, 4
    dlm, dlm7 = device_lm(lm_ref.toy_lm(Cn, 3, 0)), device_lm(lm_ref.toy_lm(Cn + 1, 2, 0))
    z = torch.zeros(B, Tp, Cn + 1, device=DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_beam_lm_work_bytes(B, Tp, Cn, K))
    work = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = dict(tok=torch.full((B, K, Tp), 77, dtype=torch.int32, device=DEV), ln=torch.full((B, K), 77, dtype=torch.int32, device=DEV),
               sc=torch.full((B, K), 77.0, device=DEV), am=torch.full((B, K), 77.0, device=DEV))

    def call(**kw):
        a = dict(C=Cn, blank=0, eos=Cn - 1, lm=dlm.h, lm_w=0.5, bonus=0.1, work=p(work), wb=nb, am=p(out["am"]))
        a.update(kw)
        return l.masr_ctc_beam_search_lm(p(z), Cn + 1, p(lens), B, Tp, a["C"], K, K, a["blank"], a["eos"], a["lm"], a["lm_w"], a["bonus"], a["work"],
                                         a["wb"], p(out["tok"]), p(out["ln"]), p(out["sc"]), a["am"], None)

    bad = [(dict(blank=1), b"blank must be 0"), (dict(eos=Cn - 2), b"eos must be C - 1"), (dict(eos=-1), b"eos must be C - 1"),
           (dict(lm=dlm7.h), b"classes differ"), (dict(lm_w=-0.5), b"lm_w"), (dict(lm_w=float("nan")), b"lm_w"),
           (dict(lm_w=float("inf")), b"lm_w"), (dict(bonus=float("nan")), b"len_bonus"), (dict(bonus=float("-inf")), b"len_bonus"),
           (dict(wb=nb - 1), b"work buffer too small"), (dict(lm=None), b"null language model"), (dict(am=None), b"null pointer")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in l.masr_last_error(), (kw, l.masr_last_error())
    torch.cuda.synchronize()
    for t in out.values():                                          # nothing was launched: the outputs still hold their fill
        assert (t == 77).all()
    assert call() == 0 and call(bonus=-2.0) == 0 and call(lm_w=0.0) == 0
    torch.cuda.synchronize()
    assert (out["ln"][:, 0] >= 0).all()
    assert l.masr_ctc_beam_lm_work_bytes(B, Tp, Cn, 65) < 0 and l.masr_ctc_beam_lm_work_bytes(B, Tp, 4097, K) < 0
