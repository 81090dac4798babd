"""tests/ctc_loss_ref.py pinned (no GPU): against torch's CPU ctc_loss run in float64 through autograd on every case the device tests use and on
a few of its own (a lattice of 601 states, a blank in the middle, zero lengths), against oracle.ref_cpu.ctc_loss_np on the small ones, and
that every utterance the device tests call feasible has a finite nll here and every infeasible one has none -- so the device comparisons
cannot quietly turn into all-zero ones."""
import numpy as np
import pytest
import torch

import ctc_loss_ref as R
from oracle import ref_cpu

CASES = R.all_cases()
SMALL = [c for c in CASES if c.logits.shape[0] <= 13 and c.logits.shape[2] <= 65]


def torch_f64(case):
    z = torch.from_numpy(case.logits.astype(np.float64)).requires_grad_(True)
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(z, -1), torch.from_numpy(R.concatenated(case)), torch.from_numpy(case.in_len.astype(np.int64)),
                                        torch.from_numpy(case.tgt_len.astype(np.int64)), blank=case.blank, reduction="mean", zero_infinity=True)
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


def run(case):
    return R.ctc_loss(case.logits, case.targets, case.tgt_off, case.in_len, case.tgt_len, case.blank)


def own_case(seed, T, C, tgt_len, in_len, blank, scale=1.0):
    return R._make(f"own-{seed}", seed, T, C, tgt_len, in_len, blank, scale, [True] * len(tgt_len))


OWN = [own_case(1, 320, 11, [300, 40, 0], [320, 100, 0], 5),            # S = 601, a blank in the middle, an utterance without frames or labels
       own_case(2, 6, 5, [0, 2, 3, 1], [0, 0, 6, 1], 4),                # no frames with and without a target
       own_case(3, 40, 7, [12, 0, 30], [40, 17, 31], 0, 6.0)]           # peaked posteriors; 30 labels in 31 frames (infeasible with a repeat)


@pytest.mark.parametrize("case", CASES + OWN, ids=lambda c: c.name)
def test_matches_torch_float64(case):
    """the two are float64 evaluations of one recursion in different summation orders.  Loss: 1e-12 relative.  Gradient: a posterior is
    exp(alpha + beta - lp - ll), and alpha and beta are each the end of a chain of up to T additions of numbers as large as the nll, every one
    rounded to 2^-53 of it; if all of those roundings lined up the exponent would be off by 2 T 2^-53 nll in each of the two
    implementations, which is the relative error of a posterior <= 1 -- so 4 T 2^-53 max(nll, 1) (about 1e-9 for T = 640, nll = 7000; the
    difference seen is 1.4e-11) plus 1e-13 for the softmax and the class sums, of the gradient's largest element."""
    r = run(case)
    loss, grad = torch_f64(case)
    assert abs(r.loss - loss) <= 1e-12 * max(1.0, abs(loss)), (r.loss, loss)
    err = np.abs(r.grad - grad)
    bound = (4 * case.logits.shape[0] * 2.0 ** -53 * max(1.0, float(r.nll.max())) + 1e-13) * np.abs(grad).max()
    assert err.max() <= bound, (float(err.max()), bound)
    for b in range(len(case.in_len)):
        assert np.all(r.grad[int(case.in_len[b]):, b] == 0.0)
        if not np.isfinite(r.nll_raw[b]):
            assert r.nll[b] == 0.0 and np.all(r.grad[:, b] == 0.0)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_matches_oracle_ctc_loss_np(case):
    """oracle.ref_cpu.ctc_loss_np returns d loss / d log-probs g; through the softmax that is g - softmax * sum_c g"""
    r = run(case)
    lp = R.log_softmax(case.logits)
    keep = np.asarray(case.in_len) > 0                          # (the oracle's double loop has no frameless form)
    sub = R.Case(case.name, case.logits[:, keep], case.targets, case.tgt_off[keep], case.in_len[keep], case.tgt_len[keep], case.blank, None)
    loss, g = ref_cpu.ctc_loss_np(lp[:, keep], R.concatenated(sub), sub.in_len, sub.tgt_len, blank=case.blank)
    B, Bk = len(case.in_len), int(keep.sum())
    gz = (g - np.exp(lp[:, keep]) * g.sum(-1, keepdims=True)) * Bk / B
    assert abs(r.loss - loss * Bk / B) <= 1e-12 * max(1.0, abs(r.loss))
    np.testing.assert_allclose(r.grad[:, keep], gz, rtol=1e-9, atol=1e-13)


def test_offsets_need_not_be_concatenated_or_ordered():
    case = R.case_short(0)
    assert not np.array_equal(np.sort(case.tgt_off), case.tgt_off) or (np.diff(case.tgt_off) != case.tgt_len[:-1]).any()
    tight = R.concatenated(case).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(case.tgt_len)[:-1]]).astype(np.int32)
    a, b = run(case), R.ctc_loss(case.logits, tight, off, case.in_len, case.tgt_len, case.blank)
    assert np.array_equal(a.nll, b.nll) and np.array_equal(a.grad, b.grad)
    pt, po, Lmax = R.padded(case)
    c = R.ctc_loss(case.logits, pt, po, case.in_len, case.tgt_len, case.blank)
    assert Lmax == 3 and np.array_equal(a.nll, c.nll) and np.array_equal(a.grad, c.grad)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_device_cases_are_feasible_as_stated(case):
    r = run(case)
    assert len(case.feasible) == len(case.in_len)
    for b, ok in enumerate(case.feasible):
        assert bool(np.isfinite(r.nll_raw[b])) == ok, (case.name, b, r.nll_raw[b])
        if ok and case.in_len[b] > 0:
            assert np.abs(r.grad[:int(case.in_len[b]), b]).max() > 0.0
            assert r.nll[b] > 0.0
    # what the device tests rely on: class C - 1 is a target (vocabulary tail), the widths of the wide case, both skip decisions
    C = case.logits.shape[2]
    if case.name.startswith("vocab"):
        assert (R.concatenated(case) == C - 1).any()
    if case.name.startswith("wide"):
        assert [2 * int(l) + 1 for l in case.tgt_len] == [257, 601, 255, 513, 601]
        for b in range(len(case.tgt_len)):
            y = case.targets[int(case.tgt_off[b]):int(case.tgt_off[b]) + int(case.tgt_len[b])]
            assert (y[1:] == y[:-1]).any() and (y[1:] != y[:-1]).any()
    if case.name == "limit":
        assert 2 * int(case.tgt_len[0]) + 1 == 2047
    if case.name.startswith("short"):
        assert not (R.concatenated(case) == case.blank).any()
