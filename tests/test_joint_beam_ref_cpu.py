"""The CPU restatement of the joint CTC/attention beam (tests/joint_beam_ref.py) against independent facts: psi(h + eos) is the CTC
log-likelihood of torch's ctc_loss, psi(h) is the summed probability of every frame path whose collapsed labelling starts with h, a beam
that prunes nothing finds the optimum of an exhaustive enumeration, and a vanishing CTC weight gives beam_ref's result.  CPU only."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

import beam_ref
import hybrid_ref
import joint_beam_ref as jr
from oracle import ref_cpu
from oracle.make_goldens import TINY, ODIM, synth_batch


def _rand_lp(T, C, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, C, generator=g) * scale, dim=-1).numpy().astype(np.float32)


def _collapse(path):
    out, prev = [], None
    for c in path:
        if c != prev and c != 0:
            out.append(c)
        prev = c
    return out


def test_eos_score_is_ctc_log_likelihood():
    for seed, T, C, h in ((1, 12, 6, [1, 2, 3]), (2, 9, 5, [2, 2, 1]), (3, 15, 7, [4, 4, 4, 1, 5]), (4, 5, 4, [1]), (5, 8, 5, [3, 1, 3, 1])):
        x = _rand_lp(T, C, seed)
        _, state = jr.prefix_score(x, h)
        got = float(jr.ctc_eos(state))
        want = -float(F.ctc_loss(torch.from_numpy(x)[:, None], torch.tensor([h]), torch.tensor([T]), torch.tensor([len(h)]),
                                 blank=0, reduction="none")[0])
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (seed, got, want)


def test_prefix_score_is_summed_path_probability():
    """full enumeration of the C^T frame paths (T <= 6, C <= 5), repeated tokens included"""
    for seed, T, C in ((11, 5, 4), (12, 6, 4), (13, 4, 5), (14, 6, 3)):
        x = _rand_lp(T, C, seed, scale=1.0)
        paths = list(itertools.product(range(C), repeat=T))
        logp = np.array([sum(float(x[t, c]) for t, c in enumerate(pth)) for pth in paths])
        labels = [_collapse(pth) for pth in paths]
        hyps = [h for n in (1, 2, 3) for h in itertools.product(range(1, C), repeat=n)]
        for h in hyps:
            h = list(h)
            sel = [lp for lp, lab in zip(logp, labels) if lab[:len(h)] == h]
            want = float(np.logaddexp.reduce(sel)) if sel else -math.inf
            got = float(jr.prefix_score(x, h)[0])
            if want == -math.inf:
                assert got == -math.inf, (seed, h, got)
            else:
                assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (seed, h, got, want)


def _hybrid_p(C, seed, head_scale=4.0):
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, C, seed=seed), C, seed=seed + 100)
    sd[hybrid_ref.HEAD[0]] = sd[hybrid_ref.HEAD[0]] * head_scale
    return hybrid_ref.leafify(sd, TINY)


def test_joint_beam_is_exhaustive_search_when_nothing_is_pruned():
    C = 4                                                    # blank 0, tokens 1 and 2, eos 3
    p = _hybrid_p(C, 5)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3
    n = 0
    for (aw, cw), minr in itertools.product(((0.5, 0.5), (0.7, 0.3), (0.0, 1.0)), (0.0, 0.5)):
        got = jr.joint_beam_search(p, TINY, xs, il, K=64, att_w=aw, ctc_w=cw, min_step_ratio=minr)
        want = jr.joint_exhaustive(p, TINY, xs, il, aw, cw, min_step_ratio=minr)
        for g, (tok, sc) in zip(got, want):
            if sc == -math.inf:
                assert g["score"] == -math.inf and g["tokens"] == []
                continue
            assert abs(g["score"] - sc) <= 1e-5 * max(1.0, abs(sc)), (aw, cw, g, tok, sc)
            if g["end_gap"] > 1e-5:
                assert g["tokens"] == tok, (aw, cw, g, tok, sc)
            n += 1
    assert n >= 12


def test_vanishing_ctc_weight_is_attention_beam():
    """a 12-class model with a spread output layer (as tests/test_hip_beam.py) that never favours token 0 (sos = blank): the attention
    beam's result wins again whenever it has a CTC alignment and every decision of the attention beam is well apart.  (The random
    decoder repeats one token; maxlen = 0.3 enc_len keeps such hypotheses alignable.)"""
    C = 12
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, C, seed=7), C, seed=107)
    sd["char_trans.weight"] = sd["char_trans.weight"] * 10.0
    sd["pre_embed.weight"] = sd["char_trans.weight"]
    sd["char_trans.bias"] = sd["char_trans.bias"].clone()
    sd["char_trans.bias"][0] = -30.0
    p = hybrid_ref.leafify(sd, TINY)
    pa = ref_cpu.leafify({k: v for k, v in sd.items() if k not in hybrid_ref.HEAD}, TINY)
    n = 0
    for seed, ilens in ((11, [64, 52, 40, 33]), (12, [48, 44, 60])):
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        ref = beam_ref.beam_search(pa, TINY, xs, il, K=4, max_step_ratio=0.3)
        got = jr.joint_beam_search(p, TINY, xs, il, K=4, att_w=1.0, ctc_w=1e-9, max_step_ratio=0.3)
        frames = jr.ctc_frames(p, TINY, xs, il)
        for r, g, x in zip(ref, got, frames):
            psi, state = jr.prefix_score(x, r["tokens"])
            if 0 in r["tokens"] or beam_ref.min_gap(r) <= 1e-4 or psi == jr.NEG or jr.ctc_eos(state) == jr.NEG:
                continue
            assert g["tokens"] == r["tokens"], (r, g)
            n += 1
    assert n >= 4, n
