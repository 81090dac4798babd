"""Pins tests/rescore_ref.py, the CPU restatement of attention rescoring, on the CPU: its attention score of a hypothesis is
the running score the attention beam's restatement (beam_ref) gives the same hypothesis ended by eos, built step by step from last_logits;
the order rule on hand-made ties; and, on the toy model the GPU tests use, that rescoring does move another hypothesis to rank 1."""
import math

import numpy as np
import torch

import beam_ref
import ctc_beam_ref as cr
import hybrid_ref
import rescore_ref as rr
from oracle import ref_cpu
from oracle.make_goldens import TINY, synth_batch

C = 12
BATCHES = ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60]))


def _joint_sd(seed=7):
    """decode_util.joint_state_dict(TINY, 7) without that module's GPU imports"""
    sd = ref_cpu.deterministic_state_dict(TINY, C, seed=seed)
    sd["char_trans.weight"] = sd["char_trans.weight"] * 10.0
    sd["pre_embed.weight"] = sd["char_trans.weight"]
    sd = hybrid_ref.with_head(sd, C, seed=seed + 100)
    sd[hybrid_ref.HEAD[0]] = sd[hybrid_ref.HEAD[0]] * 6.0
    sd["char_trans.bias"] = sd["char_trans.bias"].clone()
    sd["char_trans.bias"][0] = -30.0
    return sd


def _first_pass(p, xs, il, K, N):
    with torch.no_grad():
        lp, el = hybrid_ref.ctc_log_probs(p, TINY, xs, il)
    out = []
    for b in range(xs.shape[0]):
        r = cr.ctc_beam_ref(np.ascontiguousarray(lp[:int(el[b]), b].numpy().astype(np.float32)), K, 0, C - 1, N)
        out.append([(list(h), s) for h, s in r["nbest"]])
    return out


def test_att_score_is_the_attention_beams_running_score():
    p = hybrid_ref.leafify(_joint_sd(), TINY)
    xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
    lists = _first_pass(p, xs, il, 8, 4)
    lists[0].append(([], 0.0))                                   # the empty hypothesis: one term, eos after sos
    lists[1].append(([3, 3, 3, 5, 1, 10, 2], -1.0))
    with torch.no_grad():
        memory, pad_mask, _ = beam_ref.encode(p, TINY, xs, il)
        n = 0
        for b, ent in enumerate(lists):
            mb, kb = memory[:, b:b + 1], pad_mask[b:b + 1]
            got = rr.att_scores(p, TINY, mb, kb, [tuple(h) for h, _ in ent])
            for (h, _), g in zip(ent, got):
                s = torch.tensor(0.0)
                for t, tgt in enumerate(list(h) + [C - 1]):
                    s = s + beam_ref.log_softmax32(beam_ref.last_logits(p, TINY, mb, kb, [tuple(h[:t])]))[0, tgt]      # fp32, as beam_ref
                assert abs(g - float(s)) <= 1e-4 + 2e-5 * abs(float(s)), (b, h, g, float(s))
                n += 1
    assert n >= 16


def test_order_rule_on_ties_and_dead_entries():
    assert rr.order_rule([-1.0, -1.0, -0.5, -1.0], [True] * 4) == [2, 0, 1, 3]
    assert rr.order_rule([-math.inf, -2.0, -math.inf, -2.0, -1.0], [False, True, False, True, True]) == [4, 1, 3, 0, 2]
    assert rr.order_rule([-3.0], [True]) == [0] and rr.order_rule([-math.inf, -math.inf], [False, False]) == [0, 1]
    # a live entry with score -inf still sorts in front of the dead ones
    assert rr.order_rule([-math.inf, -math.inf, -1.0], [False, True, True]) == [2, 1, 0]
    assert rr.combine(-2.0, -math.inf, 1.0, 0.0) == -2.0 and rr.combine(-2.0, -4.0, 0.5, 0.25) == -2.0


def test_rescoring_moves_rank_one_on_the_toy_model():
    """(K, N) = (8, 8): top_gap / min_gap of every utterance are printed; another hypothesis than the first pass's best wins somewhere"""
    p = hybrid_ref.leafify(_joint_sd(), TINY)
    for aw, cw in ((1.0, 0.5), (1.0, 0.0)):
        moved = total = 0
        for seed, ilens in BATCHES:
            xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
            lists = _first_pass(p, xs, il, 8, 8)
            for b, r in enumerate(rr.rescore(p, TINY, xs, il, lists, aw, cw)):
                print(f"att_w {aw} ctc_w {cw} seed {seed} b {b}: order {r['order']} top_gap {r['top_gap']:.3g} min_gap {r['min_gap']:.3g}")
                assert sorted(r["order"]) == list(range(len(lists[b])))
                total += 1
                moved += r["order"][0] != 0
        assert moved >= 1, (aw, cw, moved, total)
