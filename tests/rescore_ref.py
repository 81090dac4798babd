"""CPU restatement of attention rescoring (include/masr.h masr_recog_rescore / masr_rescore_nbest) on the oracle (oracle.ref_cpu).

For an utterance and a hypothesis h (tokens, no sos / eos, length l) the decoder runs teacher-forced over [sos] + h; with z_i its fp32 logits
at position i and target = h + [eos],
    att(h) = sum_{i = 0 .. l} log_softmax32(z_i)[target_i]            (beam_ref.log_softmax32, summed in float64)
    score  = att_w * att + ctc_w * ctc                                (the ctc term is left out when ctc_w == 0)
and the list is ordered by score descending, first-pass rank ascending; entries without a list (None) stay last in their own order.
Under ref_cpu.bf16_emulation() the last projection reads bf16-rounded operands, as the engine's logits GEMM does (ref_cpu.model_forward).

rank() / rescore() also record how well defined the order is: top_gap = best - second score, min_gap = the smallest gap between neighbours of the
ordered live entries (inf where there are fewer than two)."""
import math

import torch

import beam_ref
from oracle import ref_cpu


def order_rule(scores, live):
    """the output order: indices of the entries, live ones by (score descending, index ascending), then the others by index"""
    alive = sorted((i for i in range(len(scores)) if live[i]), key=lambda i: (-scores[i], i))
    return alive + [i for i in range(len(scores)) if not live[i]]


def combine(att, ctc, att_w, ctc_w):
    return att_w * att + (ctc_w * ctc if ctc_w != 0 else 0.0)


@torch.no_grad()
def att_scores(p, cfg, memory_b, mask_b, hyps):
    """float64 attention scores of the hypotheses (token tuples) of ONE utterance (memory_b [T', 1, E], mask_b [1, T']).  The lists are padded
    with eos to one length: the target mask is causal, so a position never reads the padding behind it."""
    if not hyps:
        return []
    C = p["char_trans.weight"].shape[0]
    eos, n, L = C - 1, len(hyps), 1 + max(len(h) for h in hyps)
    tok = torch.full((L, n), eos, dtype=torch.int64)
    tok[0] = 0
    for k, h in enumerate(hyps):
        if len(h):
            tok[1:1 + len(h), k] = torch.tensor(list(h), dtype=torch.int64)
    y = p["pre_embed.weight"][tok] + p["pos_encoder.pe"][:L]
    causal = ref_cpu.generate_square_subsequent_mask(L)
    h = ref_cpu.decoder_forward(p, cfg, y, memory_b.expand(-1, n, -1), causal, mask_b.expand(n, -1))
    z = ref_cpu._q(h) @ ref_cpu._q(p["char_trans.weight"]).t() + p["char_trans.bias"]
    lp = beam_ref.log_softmax32(z).double()                          # [L, n, C]
    out = []
    for k, hyp in enumerate(hyps):
        tgt = list(hyp) + [eos]
        out.append(float(sum(lp[i, k, t] for i, t in enumerate(tgt))))
    return out


@torch.no_grad()
def att_lists(p, cfg, xs, ilens, lists):
    """lists[b] = first-pass entries of utterance b in rank order, each (tokens, ctc score) or None (no entry) -> per utterance the att
    score of every entry (None where there is none)"""
    memory, pad_mask, _ = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b, ent in enumerate(lists):
        it = iter(att_scores(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [tuple(e[0]) for e in ent if e is not None]))
        out.append([next(it) if e is not None else None for e in ent])
    return out


def rank(att, ent, att_w, ctc_w):
    """one utterance: att scores and first-pass entries -> dict(att, score per first-pass entry (-inf where there is none), order = first-pass
    ranks in output order, top_gap, min_gap)"""
    live = [e is not None for e in ent]
    score = [combine(a, e[1], att_w, ctc_w) if l else -math.inf for a, e, l in zip(att, ent, live)]
    order = order_rule(score, live)
    ranked = [score[i] for i in order if live[i]]
    gaps = [x - y for x, y in zip(ranked, ranked[1:])]
    return {"att": att, "score": score, "order": order, "top_gap": gaps[0] if gaps else math.inf, "min_gap": min(gaps, default=math.inf)}


def rescore(p, cfg, xs, ilens, lists, att_w, ctc_w):
    return [rank(a, ent, att_w, ctc_w) for a, ent in zip(att_lists(p, cfg, xs, ilens, lists), lists)]
