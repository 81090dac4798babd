"""masr_ctc_beam_search alone (include/masr.h, DESIGN 5.3: ctc_beam_frames + ctc_beam_sweep) on random logits against the fp64 restatement
of tests/ctc_beam_ref.py.  An utterance is compared where the restatement's slack is positive (every decisive comparison has a margin above
DELTA, ctc_beam_ref.py); there the N-best token lists must be equal and the scores within 1e-4 + 2e-5 |s|.  A case fails if more than a
quarter of its utterances are left out.  Outputs and the work buffer start filled with junk, so a position the kernels leave unwritten shows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_beam_ref as cr  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402

DEV = "cuda:0"


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def search(z, lens, Cn, K, nbest, blank, eos, junk=0x7F):
    """z [B, Tp, ld] fp32 numpy, lens int32 [B] -> (tokens [B][nbest][Tp], lens [B][nbest], scores [B][nbest]) numpy"""
    B, Tp, ld = z.shape
    l = lib()
    zd = torch.from_numpy(z).to(DEV)
    ld_ = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    nb = int(l.masr_ctc_beam_work_bytes(B, Tp, Cn, K))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), junk, dtype=torch.uint8, device=DEV)
    tok = torch.full((B, nbest, Tp), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    ln = torch.full((B, nbest), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
    rc = l.masr_ctc_beam_search(p(zd), ld, p(ld_), B, Tp, Cn, K, nbest, blank, eos, p(work), nb, p(tok), p(ln), p(sc),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def compare(name, K, rs, tok, ln, sc, nbest):
    skipped = 0
    for b, r in enumerate(rs):
        n = len(r["nbest"])
        # the layout holds for every utterance, compared or not
        live = ln[b] >= 0
        assert live[:live.sum()].all() and np.isneginf(sc[b][~live]).all() and (ln[b][~live] == -1).all(), (name, K, b)
        for i in range(nbest):
            L = max(int(ln[b, i]), 0)
            assert (tok[b, i, L:] == -1).all() and (tok[b, i, :L] >= 0).all(), (name, K, b, i)
        print(f"{name} K={K} b={b}: min_gap {r['min_gap']:.3g} slack {r['slack']:.3g} live {int(live.sum())}/{n} "
              f"max score err {max((abs(float(sc[b, i]) - r['nbest'][i][1]) for i in range(min(n, int(live.sum())))), default=0.0):.3g}")
        if not r["slack"] > 0:
            skipped += 1
            continue
        assert int(live.sum()) == n, (name, K, b, ln[b], n)
        for i, (pre, s) in enumerate(r["nbest"]):
            assert tuple(tok[b, i, :ln[b, i]].tolist()) == pre, (name, K, b, i, tok[b, i, :ln[b, i]].tolist(), pre)
            assert abs(float(sc[b, i]) - s) <= cr.tol(s), (name, K, b, i, float(sc[b, i]), s)
    assert 4 * skipped <= len(rs), (name, K, skipped)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in cr.CASES:
        cs, z, lens = cr.make_case(name)
        out[name] = (cs, z, lens, {K: cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, K, 0, cs["eos"], cs["nbest"]) for K in cs["Ks"]})
    return out


@pytest.mark.parametrize("name", list(cr.CASES))
def test_against_restatement(cases, name):
    cs, z, lens, refs = cases[name]
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        tok, ln, sc = search(z, lens, cs["C"], K, nbest, 0, cs["eos"])
        compare(name, K, refs[K], tok, ln, sc, nbest)
        for b in range(cs["B"]):                                 # blank and eos never appear
            t = tok[b][tok[b] >= 0]
            assert (t != 0).all() and (cs["eos"] < 0 or (t != cs["eos"]).all())


def test_full_buffer_all_64_slots_as_a_set(cases):
    # K = 64 with the whole final beam returned.  Adjacent scores of a 64-long list are nearly always closer than DELTA somewhere, so the
    # rank order is not compared; which 64 prefixes survive depends on the kept/dropped comparisons alone, which the case's slack covers:
    # the set of token lists is equal, and each list's score is within the tolerance of the restatement's score for that list.
    cs, z, lens, refs = cases["full_buffer"]
    tok, ln, sc = search(z, lens, cs["C"], 64, 64, 0, cs["eos"])
    full = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, 64, 0, cs["eos"], 64)
    skipped = 0
    for b, (r4, r) in enumerate(zip(refs[64], full)):
        if not r4["slack"] > 0:
            skipped += 1
            continue
        want = dict(r["nbest"])
        got = {tuple(tok[b, i, :ln[b, i]].tolist()): float(sc[b, i]) for i in range(64) if ln[b, i] >= 0}
        assert len(got) == int((ln[b] >= 0).sum()) == len(want) and set(got) == set(want), (b, set(got) ^ set(want))
        assert all(abs(got[pre] - s) <= cr.tol(s) for pre, s in want.items()), b
        assert (np.diff(sc[b][ln[b] >= 0]) <= 0).all()          # in rank order by its own scores
    assert 4 * skipped <= len(full)


def test_blank_in_the_middle():
    # blank = 2: nothing in the kernels assumes class 0
    cs, z, lens = cr.make_case("basic")
    z2 = z.copy()
    z2[..., [0, 2]] = z[..., [2, 0]]
    tok, ln, sc = search(z, lens, cs["C"], 4, 4, 0, cs["eos"])
    tok2, ln2, sc2 = search(z2, lens, cs["C"], 4, 4, 2, cs["eos"])
    assert np.array_equal(ln, ln2)
    assert np.allclose(sc, sc2, rtol=0, atol=1e-3)
    swap = np.where(tok == 2, 0, tok)                           # (class 0 is the blank on the left: never in tok)
    assert np.array_equal(swap, tok2)


def test_length_zero_and_out_of_range_lens():
    cs, z, _ = cr.make_case("few_classes")
    z = np.nan_to_num(z, nan=0.0)
    lens = np.asarray([0, -5, 1000, 24], np.int32)              # clamped to [0, Tp]
    tok, ln, sc = search(z, lens, cs["C"], 8, 8, 0, cs["eos"])
    for b in (0, 1):
        assert ln[b, 0] == 0 and sc[b, 0] == 0.0 and (ln[b, 1:] == -1).all() and np.isneginf(sc[b, 1:]).all() and (tok[b] == -1).all()
    assert ln[2, 0] >= 0 and ln[3, 0] >= 0 and np.isfinite(sc[2, 0]) and np.isfinite(sc[3, 0])


def test_permuted_batch_bit_for_bit():
    for name, K in (("basic", 8), ("peaky_merge", 3), ("wide_367", 20)):
        cs, z, lens = cr.make_case(name)
        B = cs["B"]
        reps = 3 if B < 4 else 1
        z, lens = np.concatenate([z] * reps), np.concatenate([lens] * reps)
        perm = np.random.default_rng(5).permutation(len(lens))
        a = search(z, lens, cs["C"], K, K, 0, cs["eos"])
        b = search(np.ascontiguousarray(z[perm]), lens[perm], cs["C"], K, K, 0, cs["eos"], junk=0xA5)
        for x, y in zip(a, b):
            assert np.array_equal(x[perm].view(np.uint32), y.view(np.uint32)), name


def test_argument_errors():
    l = lib()
    B, Tp, Cn, K = 2, 8, 6, 4
    z = torch.zeros(B, Tp, Cn, device=DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_beam_work_bytes(B, Tp, Cn, K))
    work = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    tok = torch.zeros(B, K, Tp, dtype=torch.int32, device=DEV)
    ln = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    sc = torch.zeros(B, K, dtype=torch.float32, device=DEV)

    def call(**kw):
        a = dict(logits=p(z), ld=Cn, enc=p(lens), B=B, Tp=Tp, C=Cn, K=K, nbest=K, blank=0, eos=Cn - 1, work=p(work), wb=nb, tok=p(tok), ln=p(ln),
                 sc=p(sc))
        a.update(kw)
        return l.masr_ctc_beam_search(a["logits"], a["ld"], a["enc"], a["B"], a["Tp"], a["C"], a["K"], a["nbest"], a["blank"], a["eos"], a["work"],
                                      a["wb"], a["tok"], a["ln"], a["sc"], None)

    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(K=0), dict(K=65), dict(nbest=0), dict(nbest=K + 1), dict(C=1), dict(C=4097, ld=4097), dict(blank=-1), dict(blank=Cn), dict(eos=Cn),
           dict(eos=-2), dict(eos=0), dict(Tp=0), dict(wb=nb - 1), dict(logits=None), dict(enc=None), dict(work=None), dict(tok=None), dict(ln=None),
           dict(sc=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert l.masr_last_error(), kw
    assert l.masr_ctc_beam_work_bytes(B, Tp, Cn, 65) < 0 and l.masr_ctc_beam_work_bytes(B, 0, Cn, K) < 0
    assert l.masr_ctc_beam_work_bytes(B, Tp, 4097, K) < 0 and l.masr_ctc_beam_work_bytes(B, Tp, 1, K) < 0
    assert call(eos=-1) == 0 and call(nbest=1) == 0
    torch.cuda.synchronize()
