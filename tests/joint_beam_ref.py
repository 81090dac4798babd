"""CPU restatement of the joint CTC/attention beam search of masr_recog_beam_ctc (include/masr.h) on the fp32 oracle.

The attention side is beam_ref's (every live hypothesis re-decodes its whole prefix, fp32 log_softmax of the last projection); the CTC
side is the one-pass prefix score of Watanabe et al. (2017) over x = hybrid_ref.ctc_log_probs, restated literally (numpy fp32):
  empty hypothesis:  r^n_t = -inf, r^b_t = x_0(blank) + ... + x_t(blank), psi = 0
  h + c (c not blank, not eos), phi_t = logaddexp(r^n_t(h), r^b_t(h)), or r^b_t(h) when c is h's last token:
    r^n_0 = x_0(c) if h is empty else -inf,  r^b_0 = -inf
    r^n_t = logaddexp(r^n_{t-1}, phi_{t-1}) + x_t(c),  r^b_t = logaddexp(r^n_{t-1}, r^b_{t-1}) + x_t(blank)
    psi(h+c) = logsumexp(r^n_0, phi_{t-1} + x_t(c) for 1 <= t < T_b)
  psi(h + eos) = logaddexp(r^n_{T_b-1}(h), r^b_{T_b-1}(h))
Search step: each live hypothesis keeps its P = min(floor(3K/2), eligible) best tokens by logit (logit descending, token ascending; blank
never, eos from minlen tokens on); s(h+c) = s(h) + att_w * lp_att + ctc_w * (psi(h+c) - psi(h)) in fp32; the K best finite candidates
(score descending, parent rank ascending, logit descending, token ascending) go on; the rest as beam_ref.

Decision gaps, as beam_ref records them: sel_gaps (K-th minus (K+1)-th candidate score), stop_gaps, end_gap, and pre_gaps (the P-th
minus the (P+1)-th logit of a pre-beam that cut anything)."""
import math

import numpy as np
import torch

import beam_ref
import hybrid_ref

F32 = np.float32
NEG = F32(-np.inf)


def ctc_empty(x):
    """state (r^n, r^b) of the empty hypothesis over x [T][C] (fp32 log-probs of one utterance, T = T_b frames)"""
    rb = np.zeros(x.shape[0], F32)
    acc = F32(0)
    for t in range(x.shape[0]):
        acc = F32(acc + x[t, 0])
        rb[t] = acc
    return np.full(x.shape[0], NEG, F32), rb


def ctc_extend(x, state, h, cs):
    """states and prefix scores of h + c for the tokens cs (none blank or eos) -> ([(r^n, r^b)], psi [n])"""
    rn_h, rb_h = state
    T, n = x.shape[0], len(cs)
    cs = np.asarray(cs, dtype=np.int64)
    phi_all = np.logaddexp(rn_h, rb_h)
    phi = np.where((cs == (h[-1] if h else -1))[None, :], rb_h[:, None], phi_all[:, None]).astype(F32)     # [T][n]
    rn = np.empty((T, n), F32)
    rb = np.empty((T, n), F32)
    rn[0] = x[0, cs] if not h else NEG
    rb[0] = NEG
    psi = rn[0].copy()
    for t in range(1, T):
        xc = x[t, cs]
        rn[t] = np.logaddexp(rn[t - 1], phi[t - 1]) + xc
        rb[t] = np.logaddexp(rn[t - 1], rb[t - 1]) + x[t, 0]
        psi = np.logaddexp(psi, phi[t - 1] + xc)
    return [(rn[:, i].copy(), rb[:, i].copy()) for i in range(n)], psi.astype(F32)


def ctc_eos(state):
    return F32(np.logaddexp(state[0][-1], state[1][-1]))


def prefix_score(x, h):
    """psi(h) by chaining extensions from the empty hypothesis"""
    state, psi = ctc_empty(x), F32(0)
    for i, c in enumerate(h):
        sts, ps = ctc_extend(x, state, tuple(h[:i]), [c])
        state, psi = sts[0], ps[0]
    return psi, state


def joint_score(s, lp, att_w, ctc_w, psi_new, psi_old):
    return F32(F32(s + F32(att_w * lp)) + F32(ctc_w * F32(psi_new - psi_old)))


def _expand(x, h, s, state, psi, z, lp, P, eos, minlen, att_w, ctc_w, pre_gaps=None):
    """the candidates of one live hypothesis: [(joint score, logit, token, state or None, psi)] in pre-beam order"""
    C = z.shape[0]
    elig = sorted((c for c in range(1, C) if not (c == eos and len(h) < minlen)), key=lambda c: (-float(z[c]), c))
    Pk = min(P, len(elig))
    if pre_gaps is not None and len(elig) > Pk:
        pre_gaps.append(float(z[elig[Pk - 1]]) - float(z[elig[Pk]]))
    sel = elig[:Pk]
    chains = [c for c in sel if c != eos]
    sts, ps = ctc_extend(x, state, h, chains) if chains else ([], [])
    by_c = {c: (sts[i], ps[i]) for i, c in enumerate(chains)}
    out = []
    for c in sel:
        st, pn = (None, ctc_eos(state)) if c == eos else by_c[c]
        js = joint_score(s, lp[c], att_w, ctc_w, pn, psi) if pn != NEG else NEG
        out.append((js, float(z[c]), c, st, pn))
    return out


def joint_search_one(p, cfg, memory_b, mask_b, x, K, maxlen, minlen, att_w, ctc_w):
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    att_w, ctc_w = F32(att_w), F32(ctc_w)
    P = 3 * K // 2
    running = [((), F32(0), ctc_empty(x), F32(0))]           # (tokens, joint score, CTC state, psi) in rank order
    ended = []
    sel_gaps, stop_gaps, pre_gaps = [], [], []
    for t in range(1, maxlen + 1):
        z = beam_ref.last_logits(p, cfg, memory_b, mask_b, [r[0] for r in running])
        lp = beam_ref.log_softmax32(z).numpy()
        z = z.float().numpy()
        cands = []
        for k, (h, s, state, psi) in enumerate(running):
            for js, zc, c, st, pn in _expand(x, h, s, state, psi, z[k], lp[k], P, eos, minlen, att_w, ctc_w, pre_gaps):
                if js != NEG:
                    cands.append((float(js), k, zc, c, st, pn))
        cands.sort(key=lambda e: (-e[0], e[1], -e[2], e[3]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c, st, pn) in enumerate(cands[:K]):
            h = running[k][0]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), F32(sc), st, pn))
                if t == maxlen:
                    ended.append((sc, t, i, h + (c,)))
        running = nxt
        best_end = max((e[0] for e in ended), default=-math.inf)
        if running and ended and t < maxlen:
            stop_gaps.append(abs(best_end - float(running[0][1])))
        if not running or best_end >= float(running[0][1]):
            break
    ended.sort(key=lambda e: (-e[0], e[1], e[2]))
    end_gap = ended[0][0] - ended[1][0] if len(ended) > 1 else math.inf
    res = {"tokens": list(ended[0][3]) if ended else [], "score": ended[0][0] if ended else -math.inf,
           "sel_gaps": sel_gaps, "stop_gaps": stop_gaps, "end_gap": end_gap, "pre_gaps": pre_gaps}
    return res


def ctc_frames(p, cfg, xs, ilens):
    """numpy fp32 CTC log-probs of every utterance, [T_b][C] each"""
    lp, enc_lens = hybrid_ref.ctc_log_probs(p, cfg, xs, torch.as_tensor(ilens))
    lp = lp.detach().float()
    return [lp[:int(enc_lens[b]), b].numpy().astype(F32) for b in range(xs.shape[0])]


@torch.no_grad()
def joint_beam_search(p, cfg, xs, ilens, K, att_w, ctc_w, min_step_ratio=0.0, max_step_ratio=1.0):
    """one result dict per utterance (see joint_search_one); p from hybrid_ref.leafify (with the CTC head)"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    xb = ctc_frames(p, cfg, xs, ilens)
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(joint_search_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], xb[b], K, maxlen, minlen, att_w, ctc_w))
    return out


def min_gap(r):
    return min(r["sel_gaps"] + r["stop_gaps"] + r["pre_gaps"] + [r["end_gap"]], default=math.inf)


@torch.no_grad()
def joint_exhaustive(p, cfg, xs, ilens, att_w, ctc_w, min_step_ratio=0.0, max_step_ratio=1.0):
    """the best complete hypothesis of every utterance by enumeration of every token sequence without blank (tiny vocabularies only),
    scored step by step as the search does -> [(tokens, score)] (([], -inf) when none is finite)"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    xb = ctc_frames(p, cfg, xs, ilens)
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    att_w, ctc_w = F32(att_w), F32(ctc_w)
    res = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        best = (-math.inf, [])
        frontier = [((), F32(0), ctc_empty(xb[b]), F32(0))]
        for t in range(1, maxlen + 1):
            z = beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [f[0] for f in frontier])
            lp = beam_ref.log_softmax32(z).numpy()
            z = z.float().numpy()
            nxt = []
            for k, (h, s, state, psi) in enumerate(frontier):
                for js, _, c, st, pn in _expand(xb[b], h, s, state, psi, z[k], lp[k], C, eos, minlen, att_w, ctc_w):
                    if js == NEG:
                        continue
                    if c == eos:
                        if float(js) > best[0]:
                            best = (float(js), list(h))
                    elif t == maxlen:
                        if float(js) > best[0]:
                            best = (float(js), list(h) + [c])
                    else:
                        nxt.append((h + (c,), js, st, pn))
            frontier = nxt
        res.append((best[1], best[0]))
    return res
