"""The resumable CTC prefix beam alone (include/masr.h masr_ctc_beam_run_*, DESIGN 5.17: ctc_beam_frames over a row range, ctc_beam_kernel<0|1,
BIAS, PH_RANGE | PH_TAIL>) against the one-shot searches masr_ctc_beam_search, _lm and _bias on the same fp32 logits.  Both sides are the
same kernel text, so every comparison is bit for bit: tokens, lens, scores, am and nbias.  The final result must not depend on how [0, Tp) was
cut into calls; the partial result after advance(t) is the one-shot search with enc_lens = min(enc_lens, t).  Outputs and the work buffer
start filled with junk; padded frames and columns are NaN."""
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
from test_hip_ctc_bias_beam_kernel import search_bias  # noqa: E402

DEV = "cuda:0"
JUNK_I = 0x7F7F7F7F


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """two result tuples, bit for bit"""
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def device_lm(lm):
    return None if lm is None else NGramLM(lm["order"], lm["C"], *lm_ref.to_arrays(lm))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Run:
    """a masr_ctc_beam_run over z [B, Tp, ld] fp32 numpy (or a device tensor that the caller goes on writing) and lens int32 [B]"""

    def __init__(self, z, lens, Cn, K, eos, dlm=None, lm_w=0.0, len_bonus=0.0, dbias=None, bias_w=0.0, junk=0x7F, guard=0):
        self.l = lib()
        self.zd = z if torch.is_tensor(z) else torch.from_numpy(z).to(DEV)
        self.B, self.Tp, self.ld = self.zd.shape
        self.lens_d = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
        self.K, self.Cn, self.with_lm, self.with_bias = K, Cn, dlm is not None, dbias is not None
        self.keep = (dlm, dbias)
        nb = int(self.l.masr_ctc_beam_run_work_bytes(self.B, self.Tp, Cn, K))
        assert nb > int(self.l.masr_ctc_beam_work_bytes(self.B, self.Tp, Cn, K)) > 0, self.l.masr_last_error()
        self.nb = nb
        self.work = torch.full((nb + guard,), junk, dtype=torch.uint8, device=DEV)      # (guard bytes behind the buffer the run is told of)
        self.h = self.l.masr_ctc_beam_run_open(p(self.zd), self.ld, p(self.lens_d), self.B, self.Tp, Cn, K, 0, eos, dlm.h if dlm is not None else None,
                                               lm_w, len_bonus, dbias.h if dbias is not None else None, bias_w, p(self.work), nb, stream())
        assert self.h, self.l.masr_last_error()

    def advance(self, t):
        assert self.l.masr_ctc_beam_run_advance(self.h, int(t), stream()) == 0, self.l.masr_last_error()
        return self

    def result(self, nbest):
        """what the matching one-shot helper returns: (tokens, lens, scores[, am[, nbias]]) numpy"""
        B, Tp = self.B, self.Tp
        tok = torch.full((B, nbest, Tp), JUNK_I, dtype=torch.int32, device=DEV)
        ln = torch.full((B, nbest), JUNK_I, dtype=torch.int32, device=DEV)
        sc = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV)
        am = torch.full((B, nbest), float("nan"), dtype=torch.float32, device=DEV) if self.with_lm or self.with_bias else None
        nbias = torch.full((B, nbest), JUNK_I, dtype=torch.int32, device=DEV) if self.with_bias else None
        assert self.l.masr_ctc_beam_run_result(self.h, nbest, p(tok), p(ln), p(sc), p(am), p(nbias), stream()) == 0, self.l.masr_last_error()
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (tok, ln, sc, am, nbias) if t is not None)

    def close(self):
        torch.cuda.synchronize()
        self.l.masr_ctc_beam_run_close(self.h)
        self.h = None


def cuts_of(Tp):
    """name -> the t_end of every advance call"""
    return {"one call": [Tp], "frame by frame": list(range(1, Tp + 1)), "7 frames": list(range(7, Tp, 7)) + [Tp],
            "edges": [0, 1, 2, Tp - 1, Tp], "repeated": [0, 0, 5, 5, Tp, Tp]}


PARTIAL_AT = lambda Tp: [0, 1, 5, Tp // 2, Tp]  # noqa: E731

PLAIN = [("basic", [1, 4, 8]), ("few_classes", None), ("peaky_merge", None), ("full_buffer", [64]), ("no_eos", None), ("neg_inf", None),
         ("wide_367", None)]


def run_cuts(z, lens, Cn, K, nbest, eos, one_shot, **fused):
    """every cut's final result equals the one-shot's (hence each other's)"""
    Tp = z.shape[1]
    for name, ts in cuts_of(Tp).items():
        r = Run(z, lens, Cn, K, eos, **fused)
        for t in ts:
            r.advance(t)
        got = r.result(nbest)
        r.close()
        assert same(got, one_shot), (name, K)


def run_partials(z, lens, Cn, K, nbest, eos, one_shot_at, final, **fused):
    """after advance(t) the result is the one-shot search on min(lens, t), twice the same; the queries do not disturb the final result"""
    Tp = z.shape[1]
    r = Run(z, lens, Cn, K, eos, junk=0xA5, **fused)
    assert same(r.result(nbest), one_shot_at(0))                   # before any advance: the empty prefix
    for t in sorted(set(PARTIAL_AT(Tp))):
        r.advance(t)
        got = r.result(nbest)
        assert same(got, one_shot_at(t)), ("partial", K, t)
        assert same(r.result(nbest), got), ("asked twice", K, t)
    assert same(r.result(nbest), final), ("final after partial queries", K)
    r.close()


@pytest.mark.parametrize("name,Ks", PLAIN, ids=[n for n, _ in PLAIN])
def test_cuts_and_partials_plain(name, Ks):
    cs, z, lens = cr.make_case(name)
    for K in Ks or cs["Ks"]:
        nbest = cs["nbest"] or K
        one = plain_search(z, lens, cs["C"], K, nbest, 0, cs["eos"])
        run_cuts(z, lens, cs["C"], K, nbest, cs["eos"], one)
        run_partials(z, lens, cs["C"], K, nbest, cs["eos"], lambda t: plain_search(z, np.minimum(lens, t), cs["C"], K, nbest, 0, cs["eos"]), one)


def frame_slices(work, B, Tp, Cn, K):
    """the frame statistics in the work buffer (ctc_beam.hip ctc_beam_carve: lse | xb | s_cls | s_lp, each rounded up to 256 bytes) as
    [B, Tp, n] uint8 views"""
    rows, P = B * Tp, min(K, Cn - 1)
    al = lambda v: (v + 255) & ~255  # noqa: E731
    out, off = [], 0
    for per_row in (4, 4, 4 * P, 4 * P):
        out.append(work[off:off + rows * per_row].view(B, Tp, per_row))
        off += al(rows * per_row)
    return out


@pytest.mark.parametrize("name,K", [("basic", 8), ("wide_367", 20)])
def test_causality_and_untouched_rows(name, K):
    cs, z, lens = cr.make_case(name)
    nbest, Tp = cs["nbest"] or K, cs["Tp"]
    one = plain_search(z, lens, cs["C"], K, nbest, 0, cs["eos"])
    full = torch.from_numpy(z).to(DEV)
    zd = torch.full_like(full, float("nan"))
    r = Run(zd, lens, cs["C"], K, cs["eos"])
    t0 = 0
    for t1 in list(range(7, Tp, 7)) + [Tp]:
        zd[:, t0:t1] = full[:, t0:t1]                               # rows t >= t1 still hold NaN when advance(t1) runs
        before = [s.clone() for s in frame_slices(r.work, r.B, Tp, cs["C"], K)]
        r.advance(t1)
        torch.cuda.synchronize()
        after = frame_slices(r.work, r.B, Tp, cs["C"], K)
        for x, y in zip(before, after):
            assert torch.equal(x[:, :t0], y[:, :t0]) and torch.equal(x[:, t1:], y[:, t1:]), (name, t0, t1)
        # inside the range the valid rows were written (the junk was 0x7F bytes), the rows past an utterance's length were not
        for b, n in enumerate(lens.tolist()):
            lo, hi = min(t0, n), min(t1, n)
            assert not (after[0][b, lo:hi] == 0x7F).all(dim=1).any(), (name, b, t0, t1)
            assert torch.equal(before[0][b, max(t0, hi):t1], after[0][b, max(t0, hi):t1]), (name, b, t0, t1)
        t0 = t1
    assert same(r.result(nbest), one)
    r.close()


def test_lengths_as_a_stream_gives_them():
    # enc_lens on the device is t_end for every utterance until it ends: 7 ends inside a range, 16 at a range border, one has length 0
    cs, z, lens = cr.make_case("few_classes")
    assert lens.tolist() == [24, 7, 16, 0]
    K = 8
    one = plain_search(z, lens, cs["C"], K, K, 0, cs["eos"])
    r = Run(z, np.zeros_like(lens), cs["C"], K, cs["eos"])
    for t in (8, 16, 24):
        r.lens_d.copy_(torch.from_numpy(np.minimum(lens, t)))
        r.advance(t)
        assert same(r.result(K), plain_search(z, np.minimum(lens, t), cs["C"], K, K, 0, cs["eos"])), t
    assert same(r.result(K), one)
    r.close()


@pytest.mark.parametrize("fused", ["plain", "lm", "lm_bias"])
def test_a_length_that_grows_behind_a_short_range_leaves_the_utterance_stopped(fused):
    """against the rule for enc_lens: utterance 1 says 3 frames while advance(8) runs and 20, then 40, afterwards.  The rows 3 .. 7 of its
    frame statistics were never computed, so no later call may run them: the utterance stays at frame 3 (the one-shot search on 3 frames),
    its unwritten rows stay junk, nothing behind the work buffer moves, and the other utterances are untouched by it."""
    cs, z, lens, lm, phrases, trie = br.make_bias_case("basic_lm")
    assert lens.tolist() == [1, 40, 23]
    K, Tp, Cn = 8, cs["Tp"], cs["C"]
    dlm = device_lm(lm) if fused != "plain" else None
    dbias = ContextBias(Cn, phrases) if fused == "lm_bias" else None
    kw = dict(dlm=dlm, lm_w=cs["lm_w"], len_bonus=cs["len_bonus"], dbias=dbias, bias_w=cs["bias_w"])
    stopped = np.asarray([1, 3, 23], np.int32)
    if fused == "plain":
        want = plain_search(z, stopped, Cn, K, K, 0, cs["eos"])
    elif fused == "lm":
        want = search_lm(z, stopped, Cn, K, K, dlm, cs["lm_w"], cs["len_bonus"])
    else:
        want = search_bias(z, stopped, Cn, K, K, dlm, cs["lm_w"], cs["len_bonus"], dbias, cs["bias_w"])
    r = Run(z, stopped, Cn, K, cs["eos"], guard=4096, **kw)
    r.advance(8)
    for t, n1 in ((16, 20), (24, 40), (Tp, 40)):
        r.lens_d.copy_(torch.from_numpy(np.asarray([1, n1, 23], np.int32)))
        r.advance(t)
        got = r.result(K)
        assert same([x[1] for x in got], [x[1] for x in want]), (fused, t)      # the stopped one, at every point
        assert t < Tp or same(got, want), fused                                # the others once they have run all their frames
        assert ((got[0] == -1) | ((got[0] > 0) & (got[0] < Cn - 1))).all()
    torch.cuda.synchronize()
    assert (r.work[r.nb:] == 0x7F).all()                           # nothing behind the buffer
    lse = frame_slices(r.work, r.B, Tp, Cn, K)[0]
    assert (lse[1, 3:8] == 0x7F).all() and not (lse[1, 8:40] == 0x7F).all(dim=1).any() and not (lse[1, :3] == 0x7F).all(dim=1).any()
    r.close()


@pytest.mark.parametrize("name", ["basic", "basic_bonus_neg", "full_buffer"])
def test_ngram_lm(name):
    cs, z, lens, lm = lr.make_lm_case(name)
    assert name != "basic" or cs["order"] >= 3
    assert name != "basic_bonus_neg" or cs["len_bonus"] != 0
    dlm = device_lm(lm)
    fused = dict(dlm=dlm, lm_w=cs["lm_w"], len_bonus=cs["len_bonus"])
    Tp = cs["Tp"]
    for K in cs["Ks"]:
        nbest = cs["nbest"] or K
        at = lambda t: search_lm(z, np.minimum(lens, t), cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"])  # noqa: E731
        one = at(Tp)
        assert len(one) == 4
        for ts in (list(range(1, Tp + 1)), list(range(7, Tp, 7)) + [Tp]):
            r = Run(z, lens, cs["C"], K, cs["eos"], **fused)
            for t in ts:
                r.advance(t)
            assert same(r.result(nbest), one), (name, K, len(ts))
            r.close()
        run_partials(z, lens, cs["C"], K, nbest, cs["eos"], at, one, **fused)


def straddles(cs, z, lens, lm, trie, K, cut_at):
    """on the CPU restatement: the (utterance, cut) pairs at which the best hypothesis of the frames in front of the cut ends inside a
    phrase match that the final best hypothesis continues behind the cut until it is earned (the automaton's revoke falls to 0 before the
    match breaks): a credited match that spans the call boundary, so its credit needs the automaton state carried in the state block"""
    out = []
    zc = z[..., :cs["C"]]
    final = br.ctc_bias_beam_ref_batch(zc, lens, K, lm, cs["lm_w"], cs["len_bonus"], trie, cs["bias_w"], nbest=1)
    for t in cut_at:
        part = br.ctc_bias_beam_ref_batch(zc, np.minimum(lens, t), K, lm, cs["lm_w"], cs["len_bonus"], trie, cs["bias_w"], nbest=1)
        for b, (pr, fr) in enumerate(zip(part, final)):
            if t >= lens[b] or not pr["nbest"] or not fr["nbest"]:
                continue
            pre, fin = pr["nbest"][0][0], fr["nbest"][0][0]
            if len(pre) >= len(fin) or fin[:len(pre)] != pre:
                continue
            u = bias_ref.state_of(trie, pre)[0]
            if u == 0 or trie["revoke"][u] == 0:                   # no match pending at the cut, or nothing of it unearned
                continue
            for c in fin[len(pre):]:
                u = trie["child"].get((u, c))
                if u is None:
                    break
                if trie["revoke"][u] == 0:
                    out.append((b, t))
                    break
    return out


@pytest.mark.parametrize("name", ["basic", "basic_lm"])
def test_bias(name):
    cs, z, lens, lm, phrases, trie = br.make_bias_case(name)
    assert cs["with_lm"] == (name == "basic_lm")
    dlm, dbias = device_lm(lm), ContextBias(cs["C"], phrases)
    fused = dict(dlm=dlm, lm_w=cs["lm_w"], len_bonus=cs["len_bonus"], dbias=dbias, bias_w=cs["bias_w"])
    Tp, K = cs["Tp"], max(cs["Ks"])
    nbest = cs["nbest"] or K
    cut7 = list(range(7, Tp, 7))
    found = straddles(cs, z, lens, lm, trie, K, cut7)
    print(f"{name}: credited matches that span a cut of the 7-frame run: {found}")
    assert found, "no credited match spans a call boundary: the case proves nothing about the carried automaton state"
    at = lambda t: search_bias(z, np.minimum(lens, t), cs["C"], K, nbest, dlm, cs["lm_w"], cs["len_bonus"], dbias, cs["bias_w"])  # noqa: E731
    one = at(Tp)
    assert len(one) == 5 and (one[4][one[1] >= 0] > 0).any()       # some returned entry carries credit
    for ts in (list(range(1, Tp + 1)), cut7 + [Tp]):
        r = Run(z, lens, cs["C"], K, cs["eos"], **fused)
        for t in ts:
            r.advance(t)
        assert same(r.result(nbest), one), (name, len(ts))
        r.close()
    run_partials(z, lens, cs["C"], K, nbest, cs["eos"], at, one, **fused)


def test_refusals():
    l = lib()
    B, Tp, Cn, K = 2, 8, 6, 4
    z = torch.randn(B, Tp, Cn, device=DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_beam_run_work_bytes(B, Tp, Cn, K))
    work = torch.full((nb + 8,), 0x5A, dtype=torch.uint8, device=DEV)
    lm = lm_ref.toy_lm(Cn, 3, 0)
    dlm, dlm7 = device_lm(lm), device_lm(lm_ref.toy_lm(Cn + 1, 2, 0))
    dbias, dbias7 = ContextBias(Cn, [[1, 2], [3]]), ContextBias(Cn + 1, [[1, 2]])

    def open_(**kw):
        a = dict(logits=p(z), ld=Cn, enc=p(lens), B=B, Tp=Tp, C=Cn, K=K, blank=0, eos=Cn - 1, lm=None, lm_w=0.5, bonus=0.0, bias=None, bias_w=1.0,
                 work=p(work), wb=nb)
        a.update(kw)
        return l.masr_ctc_beam_run_open(a["logits"], a["ld"], a["enc"], a["B"], a["Tp"], a["C"], a["K"], a["blank"], a["eos"], a["lm"], a["lm_w"],
                                        a["bonus"], a["bias"], a["bias_w"], a["work"], a["wb"], None)

    off4 = C.c_void_p(work.data_ptr() + 4)
    bad = [dict(K=0), dict(K=65), dict(C=1), dict(C=4097, ld=4097), dict(ld=Cn - 1), dict(blank=-1), dict(blank=Cn), dict(eos=Cn), dict(eos=-2),
           dict(eos=0), dict(Tp=0), dict(B=0), dict(logits=None), dict(enc=None), dict(work=None), dict(wb=nb - 1), dict(work=off4),
           # with an LM
           dict(lm=dlm.h, blank=1, eos=Cn - 1), dict(lm=dlm.h, eos=-1), dict(lm=dlm7.h), dict(lm=dlm.h, lm_w=-0.1), dict(lm=dlm.h, lm_w=float("nan")),
           dict(lm=dlm.h, bonus=float("inf")),
           # with a phrase list
           dict(bias=dbias.h, eos=-1), dict(bias=dbias.h, blank=1), dict(bias=dbias7.h), dict(bias=dbias.h, bias_w=-1.0),
           dict(bias=dbias.h, bias_w=float("nan")), dict(bias=dbias.h, lm=dlm.h, lm_w=-1.0)]
    for kw in bad:
        assert not open_(**kw), kw
        assert l.masr_last_error(), kw
    torch.cuda.synchronize()
    assert (work == 0x5A).all()                                    # no refusal wrote anything
    assert l.masr_ctc_beam_run_work_bytes(B, Tp, Cn, 65) < 0 and l.masr_ctc_beam_run_work_bytes(B, 0, Cn, K) < 0

    for fused in (dict(), dict(lm=dlm.h), dict(bias=dbias.h), dict(lm=dlm.h, bias=dbias.h)):
        h = open_(**fused)
        assert h, l.masr_last_error()
        assert l.masr_ctc_beam_run_advance(h, 5, None) == 0
        torch.cuda.synchronize()
        tok = torch.full((B, K, Tp), JUNK_I, dtype=torch.int32, device=DEV)
        ln = torch.full((B, K), JUNK_I, dtype=torch.int32, device=DEV)
        sc = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV)
        am = torch.full((B, K), 7.0, dtype=torch.float32, device=DEV)
        nbias = torch.full((B, K), JUNK_I, dtype=torch.int32, device=DEV)
        snap = work.clone()

        def result(run=h, nbest=K, **kw):
            a = dict(tok=p(tok), ln=p(ln), sc=p(sc), am=p(am), nbias=p(nbias))
            a.update(kw)
            return l.masr_ctc_beam_run_result(run, nbest, a["tok"], a["ln"], a["sc"], a["am"], a["nbias"], None)

        for t in (4, -1, Tp + 1):
            assert l.masr_ctc_beam_run_advance(h, t, None) == -1 and l.masr_last_error(), t
        assert l.masr_ctc_beam_run_advance(None, 6, None) == -1 and b"null run" in l.masr_last_error()
        refused = [dict(nbest=0), dict(nbest=K + 1), dict(run=None), dict(tok=None), dict(ln=None), dict(sc=None)]
        refused += [dict(am=None)] if fused else []
        refused += [dict(nbias=None)] if "bias" in fused else []
        for kw in refused:
            assert result(**kw) == -1 and l.masr_last_error(), (fused, kw)
        torch.cuda.synchronize()
        assert torch.equal(work, snap), fused                      # the state block and the records as they were
        assert (tok == JUNK_I).all() and (ln == JUNK_I).all() and (sc == 7.0).all() and (am == 7.0).all() and (nbias == JUNK_I).all()
        # what is allowed: no am without an LM and a phrase list, no nbias without a phrase list; and the run goes on
        assert result(nbest=1, **({} if fused else dict(am=None)), **({} if "bias" in fused else dict(nbias=None))) == 0, l.masr_last_error()
        assert l.masr_ctc_beam_run_advance(h, 5, None) == 0 and l.masr_ctc_beam_run_advance(h, Tp, None) == 0
        assert result() == 0
        torch.cuda.synchronize()
        assert (ln[:, 0] >= 0).all()
        l.masr_ctc_beam_run_close(h)
    l.masr_ctc_beam_run_close(None)
