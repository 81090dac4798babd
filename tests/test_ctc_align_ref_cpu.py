"""The CPU restatements of masr_ctc_align (tests/ctc_align_ref.py) against each other, without a device: the fp32 Viterbi against brute-force
enumeration of every CTC path (logits on a 0.5 grid, so sums are exact and ties are common: the tie rule decides), against the fp64 optimum
on log_softmax, and the layout of frames / start / end in the special cases."""
import numpy as np
import pytest

import ctc_align_ref as ar

C, BLANK = 4, 0
TARGETS = ([], [1], [2, 2], [1, 2], [3, 3, 3], [1, 1, 2], [2, 1, 2], [1, 2, 3])


def grid_logits(rng, n, scale=3.0):
    return (np.round(rng.standard_normal((n, C)) * scale * 2) / 2).astype(np.float32)


def check_layout(r, n, y, Tp, maxL):
    fr, st, en = r["frames"], r["start"], r["end"]
    assert (fr[n:] == -2).all() and (st[len(y):] == -1).all() and (en[len(y):] == -1).all()
    assert ar.collapse(fr, y) == list(y)
    for i in range(len(y)):
        assert 0 <= st[i] < en[i] <= n and (fr[st[i]:en[i]] == i).all() and (fr == i).sum() == en[i] - st[i]
    assert all(st[i] >= en[i - 1] for i in range(1, len(y)))


@pytest.mark.parametrize("y", TARGETS, ids=str)
def test_restatement_equals_enumeration(y):
    rng = np.random.default_rng(len(y) * 7 + sum(y))
    ties = 0
    for n in range(0, 7):
        for trial in range(6):
            z = grid_logits(rng, 6, scale=1.0 if trial % 2 else 3.0)
            if trial == 5:
                z[:] = 0.0                                       # the tie rule alone decides
            r = ar.align_f32(z, n, y, BLANK, Tp=6, maxL=3)
            v, states = ar.brute_force(z, n, y, BLANK)
            if states is None:
                assert r["states"] is None and np.isneginf(r["score"]) and (r["frames"] == -2).all() and (r["start"] == -1).all() and (r["end"] == -1).all()
                continue
            assert r["states"] == states and r["v"].view(np.uint32) == np.float32(v).view(np.uint32), (n, y, trial)
            check_layout(r, n, y, 6, 3)
            ties += trial == 5
    assert ties


def test_infeasible_is_exactly_too_few_frames():
    rng = np.random.default_rng(3)
    for y in TARGETS:
        need = len(y) + sum(a == b for a, b in zip(y, y[1:]))
        for n in range(0, 7):
            r = ar.align_f32(grid_logits(rng, 6), n, y, BLANK)
            assert (r["states"] is None) == (n < need or (n == 0 and len(y) > 0)), (y, n)


def test_empty_cases():
    z = grid_logits(np.random.default_rng(1), 5)
    r = ar.align_f32(z, 0, [], BLANK, Tp=5, maxL=2)
    assert r["score"] == 0.0 and (r["frames"] == -2).all() and (r["start"] == -1).all()
    r = ar.align_f32(z, 4, [], BLANK, Tp=5, maxL=2)
    assert (r["frames"] == [-1, -1, -1, -1, -2]).all() and (r["start"] == -1).all() and np.isfinite(r["score"])
    lp, _ = ar.path_logprob_f64(z, 4, [], BLANK, r["frames"])
    assert abs(float(r["score"]) - ar.log_softmax_f64(z[:4])[:, BLANK].sum()) < 1e-5 and abs(lp - float(r["score"])) < 1e-5
    r = ar.align_f32(z, 0, [1], BLANK, Tp=5, maxL=2)
    assert np.isneginf(r["score"]) and (r["frames"] == -2).all()


@pytest.mark.parametrize("y,why", [([0], "blank"), ([4], ">= C"), ([-1], "negative"), ([1, 2, 3], "tgt_len > maxL")])
def test_refused(y, why):
    r = ar.align_f32(grid_logits(np.random.default_rng(2), 5), 5, y, BLANK, Tp=5, maxL=2)
    assert np.isnan(r["score"]) and (r["frames"] == -2).all() and (r["start"] == -1).all() and (r["end"] == -1).all()


def test_f32_path_is_the_f64_optimum():
    rng = np.random.default_rng(11)
    for trial in range(20):
        n, L = int(rng.integers(8, 40)), int(rng.integers(0, 8))
        Cn = 9
        z = (np.round(rng.standard_normal((n, Cn)) * 6) / 2).astype(np.float32)
        y = [int(t) for t in rng.integers(1, Cn, L)]
        r = ar.align_f32(z, n, y, BLANK)
        best, M = ar.viterbi_f64(z, n, y, BLANK)
        if r["states"] is None:
            assert np.isneginf(best)
            continue
        lp, Mp = ar.path_logprob_f64(z, n, y, BLANK, r["frames"])
        assert lp >= best - 2 * n * 2.0 ** -24 * max(M, Mp) and lp <= best + 1e-9
        assert abs(float(r["score"]) - lp) <= ar.score_bound(z, n, Mp), (float(r["score"]), lp)
        check_layout(r, n, y, n, L)
