"""The CPU restatement of the beam search (tests/beam_ref.py) against two independent facts: with K >= C^maxlen nothing is
pruned, so it must find the global optimum of an exhaustive enumeration; with K = 1 it is the reference's greedy decode
(ref_cpu.recog_greedy) cut at the first <eos>.  CPU only."""
import torch

import beam_ref
from oracle import ref_cpu
from oracle.make_goldens import TINY, ODIM, synth_batch


def test_beam_ref_is_exhaustive_search_when_nothing_is_pruned():
    C = 4                                                    # tokens 0 .. 3, eos = 3
    p = ref_cpu.leafify(ref_cpu.deterministic_state_dict(TINY, C, seed=5), TINY)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3: 4^3 = 64 hypotheses
    for minr in (0.0, 0.5):                                  # minlen 0 / 1
        got = beam_ref.beam_search(p, TINY, xs, il, K=64, min_step_ratio=minr)
        want = beam_ref.exhaustive(p, TINY, xs, il, min_step_ratio=minr)
        for g, (tok, sc) in zip(got, want):
            assert g["tokens"] == tok, (g, tok, sc)
            assert abs(g["score"] - sc) <= 1e-5 * max(1.0, abs(sc))
            if minr > 0:
                assert len(g["tokens"]) >= 1


def test_beam_ref_k1_is_trimmed_greedy():
    p = ref_cpu.leafify(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7), TINY)
    eos = ODIM - 1
    n = 0
    for seed, T in ((11, 64), (12, 48), (13, 37), (14, 52)):
        xs, il, _, _ = synth_batch(seed, [T], [3])
        with torch.no_grad():
            g = ref_cpu.recog_greedy(p, TINY, xs, il)[:, 0].tolist()
        if g[0] == eos:                                      # greedy keeps a leading eos (trim keeps position 0); beam ends empty
            continue
        cut = g.index(eos, 1) if eos in g[1:] else len(g)
        r = beam_ref.beam_search(p, TINY, xs, il, K=1)[0]
        assert r["tokens"] == g[:cut], (r["tokens"], g)
        n += 1
    assert n >= 2
