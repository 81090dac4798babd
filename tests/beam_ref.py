"""CPU restatement of the beam search of masr_recog_beam (include/masr.h) on the fp32 oracle (oracle.ref_cpu).

Every live hypothesis re-decodes its whole prefix (no cache), one utterance at a time.  Scores are fp32 sums of
log_softmax(z) = (z - max z) - log(sum exp(z - max z)) of the fp32 last projection, as the kernels compute them.
Candidate order: score descending, parent rank ascending, then logit descending, token ascending (inside one parent the
score is a monotone function of the logit; the logit only decides what fp32 rounding made equal).

Besides the result, the search records how well defined each of its decisions was:
  sel_gaps  per step, score of the K-th selected candidate minus the (K+1)-th (a near-tie here can swap the beam),
  stop_gaps per step with both an ended and a running hypothesis, |best ended - best running| (the stop rule),
  end_gap   best minus second-best ended score (which hypothesis is the result).
"""
import math

import torch

from oracle import ref_cpu


def beam_lengths(enc_len, min_step_ratio, max_step_ratio):
    rmax = float(torch.tensor(max_step_ratio, dtype=torch.float32))     # the library receives the ratios as fp32
    rmin = float(torch.tensor(min_step_ratio, dtype=torch.float32))
    maxlen = enc_len if rmax <= 0 else max(1, math.floor(rmax * enc_len))
    return min(maxlen, 3000), max(0, math.floor(rmin * enc_len))


def encode(p, cfg, xs, ilens):
    enc, enc_lens = ref_cpu.extract_feat(p, xs, ilens)
    enc = enc.transpose(0, 1)
    enc = enc + p["pos_encoder.pe"][:enc.shape[0]]
    pad_mask = ref_cpu.make_bool_pad_mask(enc_lens)
    return ref_cpu.encoder_forward(p, cfg, enc, pad_mask), pad_mask, enc_lens


def last_logits(p, cfg, memory_b, mask_b, prefixes):
    """fp32 logits of the last position of each prefix (sos + tokens; all of one length) -> [n, C]"""
    n = len(prefixes)
    tok = torch.tensor([[0] + list(h) for h in prefixes], dtype=torch.int64).t()        # [t, n]
    y = p["pre_embed.weight"][tok] + p["pos_encoder.pe"][:tok.shape[0]]
    causal = ref_cpu.generate_square_subsequent_mask(tok.shape[0])
    h = ref_cpu.decoder_forward(p, cfg, y, memory_b.expand(-1, n, -1), causal, mask_b.expand(n, -1))
    return h[-1] @ p["char_trans.weight"].t() + p["char_trans.bias"]


def log_softmax32(z):
    z = z.float()
    m = z.max(dim=-1, keepdim=True).values
    return (z - m) - torch.log(torch.exp(z - m).sum(dim=-1, keepdim=True))


def beam_search_one(p, cfg, memory_b, mask_b, K, maxlen, minlen):
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    running = [((), torch.tensor(0.0))]                     # (tokens, fp32 score) in rank order
    ended = []                                              # (score, step, rank, tokens)
    sel_gaps, stop_gaps = [], []
    for t in range(1, maxlen + 1):
        z = last_logits(p, cfg, memory_b, mask_b, [h for h, _ in running])
        lp = log_softmax32(z)
        cands = []
        for k, (h, ps) in enumerate(running):
            sc = ps + lp[k]                                 # fp32
            for c in range(C):
                if c == eos and len(h) < minlen:
                    continue
                cands.append((float(sc[c]), k, float(z[k, c]), c))
        cands.sort(key=lambda x: (-x[0], x[1], -x[2], x[3]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c) in enumerate(cands[:K]):
            h = running[k][0]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), torch.tensor(sc, dtype=torch.float32)))
                if t == maxlen:
                    ended.append((sc, t, i, h + (c,)))
        running = nxt
        best_end = max((e[0] for e in ended), default=-math.inf)
        if running and ended and t < maxlen:              # (at maxlen the stop is forced)
            stop_gaps.append(abs(best_end - float(running[0][1])))
        if not running or best_end >= float(running[0][1]):
            break
    ended.sort(key=lambda e: (-e[0], e[1], e[2]))
    end_gap = ended[0][0] - ended[1][0] if len(ended) > 1 else math.inf
    return {"tokens": list(ended[0][3]), "score": ended[0][0], "sel_gaps": sel_gaps, "stop_gaps": stop_gaps, "end_gap": end_gap}


@torch.no_grad()
def beam_search(p, cfg, xs, ilens, K, min_step_ratio=0.0, max_step_ratio=1.0):
    """one result dict per utterance (see beam_search_one); each utterance is searched on its own"""
    memory, pad_mask, enc_lens = encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(beam_search_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], K, maxlen, minlen))
    return out


def min_gap(r):
    """the smallest recorded decision gap of one result (inf when no decision was contested)"""
    return min(r["sel_gaps"] + r["stop_gaps"] + [r["end_gap"]], default=math.inf)


@torch.no_grad()
def exhaustive(p, cfg, xs, ilens, min_step_ratio=0.0, max_step_ratio=1.0):
    """the best complete hypothesis of every utterance by enumeration (tiny vocabularies only): ends in eos after n < maxlen tokens
    (n >= minlen), or has maxlen tokens.  -> [(tokens, score)]"""
    memory, pad_mask, enc_lens = encode(p, cfg, xs, torch.as_tensor(ilens))
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    res = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        best = (-math.inf, None)
        frontier = [((), torch.tensor(0.0))]
        for t in range(1, maxlen + 1):
            lp = log_softmax32(last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [h for h, _ in frontier]))
            nxt = []
            for k, (h, ps) in enumerate(frontier):
                sc = ps + lp[k]
                for c in range(C):
                    if c == eos:
                        if len(h) >= minlen and float(sc[c]) > best[0]:
                            best = (float(sc[c]), list(h))
                    elif t == maxlen:
                        if float(sc[c]) > best[0]:
                            best = (float(sc[c]), list(h) + [c])
                    else:
                        nxt.append((h + (c,), sc[c]))
            frontier = nxt
        res.append((best[1], best[0]))
    return res
