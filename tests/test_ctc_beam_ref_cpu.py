"""Pins tests/ctc_beam_ref.py, the fp64 restatement of the CTC prefix beam search, on the CPU: against torch's CTC loss on an
exhaustive beam, that merging and re-creation occur in the GPU test's cases, and that the gap rule leaves at least 3/4 of every case's
utterances to be compared on the GPU."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_beam_ref as cr


def test_exhaustive_beam_equals_ctc_loss():
    # C = 3 without eos: labels over {1, 2}, T = 5 -> 2 + 4 + 8 + 16 + 32 = 62 non-empty prefixes + the empty one, K = 64 holds them all
    T, Cn, K = 5, 3, 64
    z = (np.random.default_rng(0).standard_normal((T, Cn)) * 2).astype(np.float32)
    r = cr.ctc_beam_ref(z, K, blank=0, eos=-1)
    lp = torch.log_softmax(torch.from_numpy(z).double(), dim=-1).unsqueeze(1)              # [T][1][C]
    want = {}
    for n in range(T + 1):
        for lab in itertools.product((1, 2), repeat=n):
            tgt = torch.tensor([lab], dtype=torch.long).reshape(1, n)
            nll = F.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([n]), blank=0, reduction="sum", zero_infinity=False)
            if math.isfinite(float(nll)):
                want[lab] = -float(nll)
    got = dict(r["nbest"])
    assert len(r["nbest"]) == len(got) == len(want) <= 63                                  # distinct prefixes, every feasible labelling
    for lab, s in want.items():
        assert abs(got[lab] - s) < 1e-9, (lab, got[lab], s)
    assert r["nbest"][0][0] == max(want, key=want.get)
    assert [s for _, s in r["nbest"]] == sorted((s for _, s in r["nbest"]), reverse=True)


def test_small_beam_is_the_top_of_a_larger_one_when_nothing_is_pruned():
    # K = 1 on a peaked row sequence is the greedy collapse
    z = np.full((6, 4), -8.0, np.float32)
    for t, c in enumerate([1, 1, 0, 1, 2, 2]):
        z[t, c] = 8.0
    r = cr.ctc_beam_ref(z, 1, blank=0, eos=3)
    assert r["nbest"][0][0] == (1, 1, 2)


def test_empty_and_excluded():
    z = np.zeros((0, 5), np.float32)
    assert cr.ctc_beam_ref(z, 4, 0, 4)["nbest"] == [((), 0.0)]
    z = (np.random.default_rng(1).standard_normal((12, 5))).astype(np.float32)
    z[:, 4] = 9.0                                                                           # eos towers over everything: still never emitted
    r = cr.ctc_beam_ref(z, 4, 0, 4)
    assert all(4 not in pre and 0 not in pre for pre, _ in r["nbest"])
    r = cr.ctc_beam_ref(z, 4, 0, -1)
    assert any(4 in pre for pre, _ in r["nbest"])


def test_merges_and_recreation_occur_in_the_peaky_case():
    cs, z, lens = cr.make_case("peaky_merge")
    assert (cs["C"], cs["Ks"], cs["Tp"], cs["scale"]) == (4, [3], 30, 4.0)
    rs = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, 3, 0, cs["eos"])
    assert all(r["merges"] > 0 for r in rs)
    assert sum(r["recreated"] for r in rs) >= 1


@pytest.mark.parametrize("name", list(cr.CASES))
def test_gap_rule_keeps_three_quarters(name):
    cs, z, lens = cr.make_case(name)
    for K in cs["Ks"]:
        rs = cr.ctc_beam_ref_batch(z[..., :cs["C"]], lens, K, 0, cs["eos"], cs["nbest"])
        safe = sum(r["slack"] > 0 for r in rs)
        assert 4 * safe >= 3 * len(rs), (name, K, [r["min_gap"] for r in rs])
        assert all(r["min_class_gap"] >= 0 for r in rs)
