"""CPU restatement of the joint CTC/attention beam with an n-gram LM, a length bonus and an N-best list (masr_recog_beam_ctc_lm,
include/masr.h): joint_beam_ref's search plus lm_ref's LM, the LM terms in fp32 in the written order.  A plain helper module
like joint_beam_ref.py: no fixtures, no tests.

Per step and live hypothesis h (score s, CTC state, psi):
  pre-beam   the P = floor(3K/2) best classes by g(c) = fl(lp(c) + fl(lm_w * lm(c | h))), order (g descending, class ascending); blank never,
             eos from minlen tokens on
  score      js = fl(fl(fl(fl(s + fl(att_w * lp)) + fl(ctc_w * fl(psi(h+c) - psi(h)))) + fl(lm_w * lm(c | h))) + b), b = len_bonus for a token
             and 0 for eos; a candidate with psi = -inf or js = -inf is dropped
  select     the K best by (js descending, parent rank ascending, pre-beam position ascending); eos ends the parent, at t = maxlen the running
             ones end as they are; the ended compete for the N-best list by (score descending, step ascending, rank ascending)
  stop       nothing runs, t >= maxlen, or the list holds N entries and its N-th score >= fl(run_best + fl((maxlen - t) * max(len_bonus, 0)))

`stop` selects the rule ("bound": the above; "none": run to maxlen; "old": DESIGN 9's best >= run_best with any list length; "best": the bound
rule with the best score in place of the N-th) and `bonus_on_eos` / `lm_in_prebeam` the other mutations the CPU tests must tell apart.
`drop_ctc` leaves the CTC term and the pre-beam cut out and admits class 0: lm_ref.beam_search_lm's candidates.

Decision gaps (the slack rule of joint_beam_ref.min_gap, extended): pre_gaps on g, sel_gaps, stop_gaps (|N-th - bound| wherever the comparison
was made), nb_gaps (between neighbours among the first N + 1 of the final ended list: the order inside the list and its boundary)."""
import math

import numpy as np
import torch

import beam_ref
import hybrid_ref  # noqa: F401  (callers leafify with it)
import joint_beam_ref as jr
import lm_ref

F32 = np.float32
NEG = F32(-np.inf)


def score(s, lp, att_w, ctc_w, psi_new, psi_old, lm_term, b):
    js = F32(F32(s + F32(att_w * lp)) + F32(ctc_w * F32(psi_new - psi_old)))
    return F32(F32(js + lm_term) + b)


def stop_bound(run_best, maxlen, t, len_bonus):
    return F32(F32(run_best) + F32(F32(maxlen - t) * F32(max(float(len_bonus), 0.0))))


def expand(x, h, s, state, psi, lp, P, eos, minlen, att_w, ctc_w, lm, lm_w, len_bonus, pre_gaps=None, *, bonus_on_eos=False,
           lm_in_prebeam=True, drop_ctc=False):
    """the candidates of one live hypothesis, in pre-beam order: [(js, token, state or None, psi)]"""
    C = lp.shape[0]
    lmv = lm_ref.lm_row32(lm, lm_ref.lm_context(lm, h))
    lm_term = (F32(lm_w) * lmv).astype(F32)
    g = (lp.astype(F32) + lm_term).astype(F32) if lm_in_prebeam else lp.astype(F32)
    elig = sorted((c for c in range(0 if drop_ctc else 1, C) if not (c == eos and len(h) < minlen)), key=lambda c: (-float(g[c]), c))
    Pk = len(elig) if drop_ctc else min(P, len(elig))
    if pre_gaps is not None and len(elig) > Pk:
        pre_gaps.append(float(g[elig[Pk - 1]]) - float(g[elig[Pk]]))
    sel = elig[:Pk]
    by_c = {}
    if not drop_ctc:
        chains = [c for c in sel if c != eos]
        sts, ps = jr.ctc_extend(x, state, h, chains) if chains else ([], [])
        by_c = {c: (sts[i], ps[i]) for i, c in enumerate(chains)}
    out = []
    for c in sel:
        b = F32(len_bonus) if (c != eos or bonus_on_eos) else F32(0)
        if drop_ctc:
            js = F32(F32(F32(s + F32(att_w * lp[c])) + lm_term[c]) + b)
            out.append((js, c, None, F32(0)))
            continue
        st, pn = (None, jr.ctc_eos(state)) if c == eos else by_c[c]
        js = score(s, lp[c], att_w, ctc_w, pn, psi, lm_term[c], b) if pn != NEG else NEG
        out.append((js, c, st, pn))
    return out


def search_one(p, cfg, memory_b, mask_b, x, K, N, maxlen, minlen, att_w, ctc_w, lm, lm_w, len_bonus, *, stop="bound", **mut):
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    att_w, ctc_w = F32(att_w), F32(ctc_w)
    P = 3 * K // 2
    running = [((), F32(0), None if mut.get("drop_ctc") else jr.ctc_empty(x), F32(0))]
    ended = []                                               # (score, step, rank, tokens)
    sel_gaps, stop_gaps, pre_gaps = [], [], []
    for t in range(1, maxlen + 1):
        lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory_b, mask_b, [r[0] for r in running])).numpy()
        cands = []
        for k, (h, s, state, psi) in enumerate(running):
            for pos, (js, c, st, pn) in enumerate(expand(x, h, s, state, psi, lp[k], P, eos, minlen, att_w, ctc_w, lm, lm_w, len_bonus, pre_gaps, **mut)):
                if js != NEG:
                    cands.append((float(js), k, pos, c, st, pn))
        cands.sort(key=lambda e: (-e[0], e[1], e[2]))
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
        ended.sort(key=lambda e: (-e[0], e[1], e[2]))
        if not running or t >= maxlen:
            break
        run_best = float(running[0][1])
        if stop == "none":
            continue
        if stop == "old":
            if ended and ended[0][0] >= run_best:
                break
            continue
        if len(ended) >= N:
            ref = ended[0][0] if stop == "best" else ended[N - 1][0]
            bound = float(stop_bound(run_best, maxlen, t, len_bonus))
            stop_gaps.append(abs(ref - bound))
            if ref >= bound:
                break
    top = ended[:N]
    nb_gaps = [ended[i][0] - ended[i + 1][0] for i in range(min(N, len(ended) - 1))]
    return {"nbest": [(list(e[3]), e[0]) for e in top], "tokens": list(top[0][3]) if top else [], "score": top[0][0] if top else -math.inf,
            "sel_gaps": sel_gaps, "stop_gaps": stop_gaps, "pre_gaps": pre_gaps, "nb_gaps": nb_gaps,
            "end_gap": nb_gaps[0] if nb_gaps else math.inf}


@torch.no_grad()
def search(p, cfg, xs, ilens, K, N, att_w, ctc_w, lm, lm_w, len_bonus, min_step_ratio=0.0, max_step_ratio=1.0, **kw):
    """one result dict per utterance (see search_one); p from hybrid_ref.leafify (with the CTC head)"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    xb = None if kw.get("drop_ctc") else jr.ctc_frames(p, cfg, xs, ilens)
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(search_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], None if xb is None else xb[b], K, N, maxlen, minlen, att_w, ctc_w, lm,
                              lm_w, len_bonus, **kw))
    return out


def min_gap(r):
    return min(r["sel_gaps"] + r["stop_gaps"] + r["pre_gaps"] + r["nb_gaps"], default=math.inf)


@torch.no_grad()
def exhaustive(p, cfg, xs, ilens, N, att_w, ctc_w, lm, lm_w, len_bonus, min_step_ratio=0.0, max_step_ratio=1.0):
    """the N best complete hypotheses of every utterance by enumeration of every token sequence without blank (tiny vocabularies only), scored
    step by step as the search does -> per utterance [(tokens, score)] best first (ties: the shorter, then the lexicographically smaller)"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    xb = jr.ctc_frames(p, cfg, xs, ilens)
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    att_w, ctc_w = F32(att_w), F32(ctc_w)
    res = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        done = []
        frontier = [((), F32(0), jr.ctc_empty(xb[b]), F32(0))]
        for t in range(1, maxlen + 1):
            if not frontier:
                break
            lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [f[0] for f in frontier])).numpy()
            nxt = []
            for k, (h, s, state, psi) in enumerate(frontier):
                for js, c, st, pn in expand(xb[b], h, s, state, psi, lp[k], C, eos, minlen, att_w, ctc_w, lm, lm_w, len_bonus):
                    if js == NEG:
                        continue
                    if c == eos:
                        done.append((float(js), list(h)))
                    elif t == maxlen:
                        done.append((float(js), list(h) + [c]))
                    else:
                        nxt.append((h + (c,), js, st, pn))
            frontier = nxt
        done.sort(key=lambda e: (-e[0], len(e[1]), e[1]))
        res.append([(tok, sc) for sc, tok in done[:N]])
    return res


# ---------------------------------------------------------------- the cases of tests/test_hip_joint_lm_beam.py (their qualifying share is
# asserted on this restatement alone by tests/test_joint_lm_beam_ref_cpu.py)
LM_ORDER = 3
LM_SEED = 276                                                # lm_ref.toy_lm(C_SMALL, LM_ORDER, LM_SEED): test_hip_lm_beam.py's LM
TINY_BATCHES = ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60]))      # test_hip_joint_beam.py's
TINY_KS = (4, 20)
# (att_w, ctc_w, lm_w, len_bonus, N).  The bonus of 1 nat roughly cancels what this LM charges a token the decoder likes (0.5 x ~2 nats), so
# the hypotheses keep several tokens at att_w 0.7 and the list order is not decided by length alone; 2 nats at lm_w 1; one negative bonus
SETTINGS = ((0.5, 0.5, 0.5, 1.0, 1), (0.7, 0.3, 0.3, 1.0, 2), (0.3, 0.7, 1.0, 2.0, 3), (0.5, 0.5, 0.5, -0.5, 2), (0.0, 1.0, 0.5, 1.0, 2))
# the hkust-geometry case: joint_state_dict(HKUST, 3), torch.manual_seed(3), xs = randn(4, 96, 83), K = 4
HKUST_ILENS = (96, 88, 80, 72)
HKUST_SETTINGS = ((0.5, 0.5, 0.3, 1.0, 2), (0.7, 0.3, 0.3, 1.0, 2), (0.7, 0.3, 0.3, -0.5, 2), (0.6, 0.4, 0.3, 1.0, 2))
