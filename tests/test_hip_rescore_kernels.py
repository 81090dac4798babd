"""The two kernels of attention rescoring alone (rescore.hip) through include/masr_test.h: masr_test_rescore_score against an fp64
log-softmax sum at the project's log-sum-exp tolerance (ctc_beam_ref.tol, 1e-4 + 2e-5 |s|), masr_test_rescore_select against the order rule of
tests/rescore_ref.py with exact ties, entries without a list and exact copies."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_beam_ref as cr  # noqa: E402
import rescore_ref as rr  # noqa: E402
from masr_amd._cabi import lib  # noqa: E402

DEV = "cuda:0"


def _p(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# R hypotheses of L positions, C classes in rows of ld > C floats.  L = 1: only empty hypotheses (one term each); 41 > the 4 waves of a workgroup
@pytest.mark.parametrize("R,L,C,ld", [(5, 1, 12, 16), (6, 7, 367, 369), (9, 41, 12, 13), (3, 41, 367, 376), (4, 7, 12, 12 + 64)])
def test_score_kernel_vs_fp64(R, L, C, ld):
    rng = np.random.default_rng(100 * L + C)
    z = np.full((R, L, ld), np.nan, np.float32)                  # padding columns are never read
    z[..., :C] = rng.uniform(-30.0, 30.0, (R, L, C)).astype(np.float32)
    gold = np.full((R, L), -1, np.int32)
    lens = rng.integers(0, L, R)
    lens[0] = L - 1                                              # one hypothesis fills every position
    for r in range(R):
        gold[r, :lens[r]] = rng.integers(1, C - 1, lens[r])
        gold[r, lens[r]] = C - 1
    if R > 2:
        gold[R - 2] = -1                                         # an entry the first pass did not fill
    zd, gd = torch.from_numpy(z).to(DEV), torch.from_numpy(gold).to(DEV)
    row_lp = torch.full((R * L,), float("nan"), device=DEV)
    att = torch.full((R,), float("nan"), device=DEV)
    assert lib().masr_test_rescore_score(_p(zd), ld, _p(gd), R, L, C, _p(row_lp), _p(att), _stream()) == 0, lib().masr_last_error()
    got = att.cpu().numpy()
    z64 = z[..., :C].astype(np.float64)
    mx = z64.max(-1, keepdims=True)
    lp = z64 - (mx + np.log(np.exp(z64 - mx).sum(-1, keepdims=True)))
    worst = 0.0
    for r in range(R):
        terms = [lp[r, l, gold[r, l]] for l in range(L) if gold[r, l] >= 0]
        if not terms:
            assert got[r] == -np.inf, (r, got[r])
            continue
        want = float(np.sum(terms))
        worst = max(worst, abs(got[r] - want) / cr.tol(want))
        assert abs(got[r] - want) <= cr.tol(want), (r, got[r], want)
    print(f"R {R} L {L} C {C}: worst |diff| / tol = {worst:.3g}")
    # the same rows as another launch geometry (each hypothesis alone) give the same bits
    for r in (0, R - 1):
        a1 = torch.full((1,), float("nan"), device=DEV)
        assert lib().masr_test_rescore_score(_p(zd[r]), ld, _p(gd[r]), 1, L, C, _p(row_lp), _p(a1), _stream()) == 0
        assert a1.cpu().numpy()[0].tobytes() == got[r].tobytes()
    assert lib().masr_test_rescore_score(_p(zd), C - 1, _p(gd), R, L, C, _p(row_lp), _p(att), _stream()) != 0      # ld < C
    assert lib().masr_test_rescore_score(None, ld, _p(gd), R, L, C, _p(row_lp), _p(att), _stream()) != 0


@pytest.mark.parametrize("N,att_w,ctc_w", [(1, 1.0, 0.5), (3, 0.7, 0.3), (64, 1.0, 0.5), (64, 1.0, 0.0)])
def test_select_kernel_order_ties_and_copies(N, att_w, ctc_w):
    B, ld = 3, 9
    rng = np.random.default_rng(N)
    tok = rng.integers(-1, 11, (B, N, ld)).astype(np.int32)
    lens = rng.integers(0, ld + 1, (B, N)).astype(np.int32)
    # few distinct values: equal scores occur, exactly
    att = (-0.5 * rng.integers(1, 6, (B, N))).astype(np.float32)
    ctc = (-0.25 * rng.integers(1, 4, (B, N))).astype(np.float32)
    dead = rng.random((B, N)) < 0.2
    dead[0] = False
    if N > 1:
        dead[1, 0] = True                                        # a dead entry in front of live ones
        dead[2] = True                                           # an utterance with nothing at all
        if ctc_w == 0.0:
            ctc[0, 1] = -np.inf                                  # not read when ctc_w == 0
    lens[dead] = -1
    ctc[dead] = -np.inf
    att[dead] = np.nan                                           # what the score kernel left for them is not read
    t = lambda a: torch.from_numpy(a).to(DEV)
    tin, lin, cin, ain = t(tok), t(lens), t(ctc), t(att)
    otok, olen = torch.full_like(tin, -7), torch.full_like(lin, -7)
    osc, oatt, octc = (torch.full((B, N), float("nan"), device=DEV) for _ in range(3))
    oord = torch.full_like(lin, -7)
    rc = lib().masr_test_rescore_select(_p(tin), ld, _p(lin), _p(cin), _p(ain), B, N, att_w, ctc_w, _p(otok), _p(olen), _p(osc), _p(oatt), _p(octc),
                                        _p(oord), _stream())
    assert rc == 0, lib().masr_last_error()
    aw, cw = np.float32(att_w), np.float32(ctc_w)
    ties = 0
    for b in range(B):
        live = [not d for d in dead[b]]
        score = [np.float32(aw * att[b, n] + (cw * ctc[b, n] if ctc_w != 0 else np.float32(0))) if live[n] else np.float32(-np.inf) for n in range(N)]
        order = rr.order_rule([float(s) for s in score], live)
        ties += len(score) - len(set(score))
        assert oord[b].cpu().tolist() == order, (b, oord[b].cpu().tolist(), order)
        for j, n in enumerate(order):
            assert np.array_equal(otok[b, j].cpu().numpy(), tok[b, n])
            assert int(olen[b, j]) == (lens[b, n] if live[n] else -1)
            assert octc[b, j].cpu().numpy().tobytes() == ctc[b, n].tobytes()
            assert osc[b, j].cpu().numpy().tobytes() == score[n].tobytes(), (b, j, float(osc[b, j]), score[n])
            assert oatt[b, j].cpu().numpy().tobytes() == (att[b, n] if live[n] else np.float32(-np.inf)).tobytes()
    assert N == 1 or ties > 0
    assert lib().masr_test_rescore_select(_p(tin), ld, _p(lin), _p(cin), _p(ain), B, 65, att_w, ctc_w, _p(otok), _p(olen), _p(osc), _p(oatt), _p(octc),
                                          _p(oord), _stream()) != 0
