"""CPU restatement of the phrase-biased attention beam and joint beam (masr_recog_beam_bias, masr_recog_beam_ctc_bias; include/masr.h,
DESIGN 5.14) and the cases tests/test_bias_beam_ref_cpu.py and tests/test_hip_bias_beam.py share.  A plain helper module like
joint_lm_beam_ref.py: no fixtures, no tests.

It is lm_ref.beam_search_lm_one / joint_lm_beam_ref.search_one extended with bias_ref's automaton: every running hypothesis carries its state
(node, credited tokens), a function of its tokens alone.  `lm` may be None (f = lp; the joint score's LM term is then +0).  For a hypothesis h
of t - 1 tokens in state (u, n) and a class c at step t:
  (u', n') = bias_ref.step((u, n), c)   (classes 0 and eos have no child: (root, n - revoke(u)))
  dn = n' - n;  c != eos and t >= maxlen: dn -= revoke(u')            b(h, c) = fl(bias_w * (float)dn)
  attention   g(c) = fl(f(c) + b); the candidates by (fl(s + g) descending, parent rank ascending, g descending, class ascending); stop: nothing
              runs, t >= maxlen, or best ended >= fl(run_best + fl((float)(maxlen - t) * bias_w))
  joint       the pre-beam's P best by (g descending, class ascending), blank never, eos from minlen on; score = joint_lm_beam_ref.score's five
              roundings, then fl(. + b); stop: nothing runs, t >= maxlen, or the list holds N and its N-th >=
              fl(run_best + fl((float)(maxlen - t) * fl(max(len_bonus, 0) + bias_w)))
stop=False runs every utterance to maxlen (or until nothing runs).  `mutate` names a deliberately wrong variant:
  "no_revoke"            a match broken by a token keeps its unearned tokens
  "no_final_revoke"      neither eos nor the end at maxlen gives the unearned tokens back
  "no_retry_from_root"   the token that broke a match is not tried as the start of a new one
  "bias_not_in_prebeam"  the joint pre-beam ranks by f alone (the bias term only in the score)
  "old_stop_rule"        the stop bound without the bias_w term
A result: tokens, score, nbias (n_final of the tokens), nbest [(tokens, score, nbias)] (joint), steps (executed), revoked (unearned tokens were
taken back somewhere on the returned hypotheses' paths or at their ends), rescued (pre-beam entries of positive bias term that f alone would
have left out; joint), and joint_lm_beam_ref's decision gaps."""
import math

import numpy as np
import torch

import beam_ref
import bias_ref
import joint_beam_ref as jr
import joint_lm_beam_ref as jl
import lm_ref

F32 = np.float32
NEG = F32(-np.inf)
MUTATIONS = ("no_revoke", "no_final_revoke", "no_retry_from_root", "bias_not_in_prebeam", "old_stop_rule")


def bias_row(trie, state, C, eos, last, bias_w, mutate=None):
    """-> (b fp32 [C], dn int [C]) of a hypothesis in `state` over every class; last: t >= maxlen"""
    smut = mutate if mutate in ("no_revoke", "no_retry_from_root") else None
    dn = np.zeros(C, np.int64)
    for c in range(C):
        if c == eos:                                         # the end of the hypothesis: no child, the unearned tokens go back
            dn[c] = 0 if mutate == "no_final_revoke" else -trie["revoke"][state[0]]
            continue
        nst = bias_ref.step(trie, state, c, smut)
        dn[c] = nst[1] - state[1]
        if last and mutate != "no_final_revoke":
            dn[c] -= trie["revoke"][nst[0]]
    return (F32(bias_w) * dn.astype(F32)).astype(F32), dn


def path_revoked(trie, h, ended_by_eos):
    """unearned tokens were taken back while h was built, or at its end"""
    st = bias_ref.ROOT
    for c in h:
        if bias_ref.revoked_by(trie, st, int(c)) > 0:
            return True
        st = bias_ref.step(trie, st, int(c))
    return trie["revoke"][st[0]] > 0


def f_row(lp_row, lm, h, lm_w):
    return lm_ref.fused_row(lp_row, lm, h, lm_w) if lm is not None else lp_row.astype(F32)


def att_bound(run_best, maxlen, t, bias_w, mutate=None):
    return F32(run_best) if mutate == "old_stop_rule" else F32(F32(run_best) + F32(F32(maxlen - t) * F32(bias_w)))


def att_search_one(p, cfg, memory_b, mask_b, K, maxlen, minlen, lm, lm_w, trie, bias_w, *, stop=True, mutate=None):
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    smut = mutate if mutate in ("no_revoke", "no_retry_from_root") else None
    running = [((), F32(0.0), bias_ref.ROOT)]
    ended = []                                               # (score, step, rank, tokens)
    sel_gaps, stop_gaps = [], []
    steps = 0
    for t in range(1, maxlen + 1):
        steps = t
        lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory_b, mask_b, [r[0] for r in running])).numpy()
        cands = []
        for k, (h, ps, st) in enumerate(running):
            b, _ = bias_row(trie, st, C, eos, t >= maxlen, bias_w, mutate)
            g = (f_row(lp[k], lm, h, lm_w) + b).astype(F32)
            sc = (ps + g).astype(F32)
            for c in range(C):
                if c == eos and len(h) < minlen:
                    continue
                cands.append((float(sc[c]), k, float(g[c]), c))
        cands.sort(key=lambda x: (-x[0], x[1], -x[2], x[3]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c) in enumerate(cands[:K]):
            h, _, st = running[k]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), F32(sc), bias_ref.step(trie, st, c, smut)))
                if t == maxlen:
                    ended.append((sc, t, i, h + (c,)))
        running = nxt
        best_end = max((e[0] for e in ended), default=-math.inf)
        if not running or t >= maxlen:
            break
        bound = float(att_bound(running[0][1], maxlen, t, bias_w, mutate))
        if ended:
            stop_gaps.append(abs(best_end - bound))
        if stop and best_end >= bound:
            break
    ended.sort(key=lambda e: (-e[0], e[1], e[2]))
    end_gap = ended[0][0] - ended[1][0] if len(ended) > 1 else math.inf
    tok = list(ended[0][3])
    return {"tokens": tok, "score": ended[0][0], "nbias": bias_ref.count(trie, tok), "steps": steps, "revoked": path_revoked(trie, tok, True),
            "ended": [(list(e[3]), e[0]) for e in ended],
            "sel_gaps": sel_gaps, "stop_gaps": stop_gaps if stop else [], "end_gap": end_gap}


@torch.no_grad()
def att_search(p, cfg, xs, ilens, K, lm, lm_w, trie, bias_w, min_step_ratio=0.0, max_step_ratio=1.0, **kw):
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(att_search_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], K, maxlen, minlen, lm, lm_w, trie, bias_w, **kw))
    return out


# ---------------------------------------------------------------- the joint beam
def joint_bound(run_best, maxlen, t, len_bonus, bias_w, mutate=None):
    gain = F32(max(float(len_bonus), 0.0))
    if mutate != "old_stop_rule":
        gain = F32(gain + F32(bias_w))
    return F32(F32(run_best) + F32(F32(maxlen - t) * gain))


def joint_expand(x, h, s, state, psi, lp, P, eos, minlen, att_w, ctc_w, lm, lm_w, len_bonus, b, pre_gaps=None, rescued=None, mutate=None):
    """the candidates of one live hypothesis, in pre-beam order: [(js, token, CTC state or None, psi)]"""
    C = lp.shape[0]
    lm_term = (F32(lm_w) * lm_ref.lm_row32(lm, lm_ref.lm_context(lm, h))).astype(F32) if lm is not None else np.zeros(C, F32)
    f = (lp.astype(F32) + lm_term).astype(F32) if lm is not None else lp.astype(F32)
    g = (f + b).astype(F32)
    key = f if mutate == "bias_not_in_prebeam" else g
    allowed = [c for c in range(1, C) if not (c == eos and len(h) < minlen)]
    elig = sorted(allowed, key=lambda c: (-float(key[c]), c))
    Pk = min(P, len(elig))
    if pre_gaps is not None and len(elig) > Pk:
        pre_gaps.append(float(key[elig[Pk - 1]]) - float(key[elig[Pk]]))
    sel = elig[:Pk]
    if rescued is not None:
        by_f = set(sorted(allowed, key=lambda c: (-float(f[c]), c))[:Pk])
        rescued.extend(c for c in sel if c not in by_f and b[c] > 0)
    chains = [c for c in sel if c != eos]
    sts, ps = jr.ctc_extend(x, state, h, chains) if chains else ([], [])
    by_c = {c: (sts[i], ps[i]) for i, c in enumerate(chains)}
    out = []
    for c in sel:
        bo = F32(len_bonus) if c != eos else F32(0)
        st, pn = (None, jr.ctc_eos(state)) if c == eos else by_c[c]
        js = F32(jl.score(s, lp[c], att_w, ctc_w, pn, psi, lm_term[c], bo) + b[c]) if pn != NEG else NEG
        out.append((js, c, st, pn))
    return out


def joint_search_one(p, cfg, memory_b, mask_b, x, K, N, maxlen, minlen, att_w, ctc_w, lm, lm_w, len_bonus, trie, bias_w, *, stop=True, mutate=None):
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    att_w, ctc_w = F32(att_w), F32(ctc_w)
    P = 3 * K // 2
    smut = mutate if mutate in ("no_revoke", "no_retry_from_root") else None
    running = [((), F32(0), jr.ctc_empty(x), F32(0), bias_ref.ROOT)]
    ended = []
    sel_gaps, stop_gaps, pre_gaps, rescued = [], [], [], []
    steps = 0
    for t in range(1, maxlen + 1):
        steps = t
        lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory_b, mask_b, [r[0] for r in running])).numpy()
        cands = []
        for k, (h, s, state, psi, bst) in enumerate(running):
            b, _ = bias_row(trie, bst, C, eos, t >= maxlen, bias_w, mutate)
            for pos, (js, c, st, pn) in enumerate(joint_expand(x, h, s, state, psi, lp[k], P, eos, minlen, att_w, ctc_w, lm, lm_w, len_bonus, b,
                                                               pre_gaps, rescued, mutate)):
                if js != NEG:
                    cands.append((float(js), k, pos, c, st, pn))
        cands.sort(key=lambda e: (-e[0], e[1], e[2]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c, st, pn) in enumerate(cands[:K]):
            h, bst = running[k][0], running[k][4]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), F32(sc), st, pn, bias_ref.step(trie, bst, c, smut)))
                if t == maxlen:
                    ended.append((sc, t, i, h + (c,)))
        running = nxt
        ended.sort(key=lambda e: (-e[0], e[1], e[2]))
        if not running or t >= maxlen:
            break
        if len(ended) >= N:
            bound = float(joint_bound(running[0][1], maxlen, t, len_bonus, bias_w, mutate))
            stop_gaps.append(abs(ended[N - 1][0] - bound))
            if stop and ended[N - 1][0] >= bound:
                break
    top = ended[:N]
    nb_gaps = [ended[i][0] - ended[i + 1][0] for i in range(min(N, len(ended) - 1))]
    return {"nbest": [(list(e[3]), e[0], bias_ref.count(trie, e[3])) for e in top], "tokens": list(top[0][3]) if top else [],
            "score": top[0][0] if top else -math.inf, "nbias": bias_ref.count(trie, top[0][3]) if top else -1, "steps": steps,
            "revoked": any(path_revoked(trie, e[3], True) for e in top), "rescued": rescued,
            "sel_gaps": sel_gaps, "stop_gaps": stop_gaps if stop else [], "pre_gaps": pre_gaps, "nb_gaps": nb_gaps,
            "end_gap": nb_gaps[0] if nb_gaps else math.inf}


@torch.no_grad()
def joint_search(p, cfg, xs, ilens, K, N, att_w, ctc_w, lm, lm_w, len_bonus, trie, bias_w, min_step_ratio=0.0, max_step_ratio=1.0, **kw):
    """one result dict per utterance; p from hybrid_ref.leafify (with the CTC head)"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    xb = jr.ctc_frames(p, cfg, xs, ilens)
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(joint_search_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], xb[b], K, N, maxlen, minlen, att_w, ctc_w, lm, lm_w, len_bonus,
                                    trie, bias_w, **kw))
    return out


def att_min_gap(r):
    return min(r["sel_gaps"] + r["stop_gaps"] + [r["end_gap"]], default=math.inf)


joint_min_gap = jl.min_gap


# ---------------------------------------------------------------- the cases
# The models are decode_util.joint_state_dict(TINY, 7) (joint) and the same without its CTC head (attention: test_hip_lm_beam.py's toy model),
# the batches joint_lm_beam_ref.TINY_BATCHES, the LM lm_ref.toy_lm(C_SMALL, 3, 276).  A case's phrase list is cut on the CPU from the UNBIASED
# search's hypotheses of ranks 2 .. K, as DESIGN 5.13's: pieces of 2 - 4 tokens, a third of them with one more, random token behind (a phrase
# the hypotheses only half match, so matches break and are revoked), plus every longer piece's first pair (a phrase inside a phrase).
def cut_phrases(hyps_per_utt, C, pseed, per_utt=6):
    rng = np.random.default_rng(2000 + pseed)
    seen, out = set(), []

    def add(ph):
        ph = tuple(int(t) for t in ph)
        if ph and ph not in seen:
            seen.add(ph)
            out.append(list(ph))

    for hyps in hyps_per_utt:
        hyps = [h for h in hyps if len(h) >= 2]
        for _ in range(per_utt if hyps else 0):
            h = hyps[int(rng.integers(len(hyps)))]
            n = int(rng.integers(2, min(4, len(h)) + 1))
            at = int(rng.integers(0, len(h) - n + 1))
            piece = tuple(h[at:at + n])
            if rng.random() < 0.34:
                piece = piece + (int(rng.integers(1, C - 1)),)
            if any(t < 1 or t > C - 2 for t in piece):      # (the attention beam may emit class 0, a phrase may not hold it)
                continue
            add(piece)
            if len(piece) > 2:
                add(piece[:2])
    return out or [[1, 2]]


# name -> (K, with_lm, lm_w, bias_w, pseed, min_step_ratio) and, joint, (att_w, ctc_w, len_bonus, N) in front.  Settings and seeds were chosen
# on the CPU (tests/test_bias_beam_ref_cpu.py asserts the conditions): at least 7 of a case's 9 utterances have every decision gap above
# JOINT_DELTA; over the cases biasing changes best hypotheses (the attention model repeats one token, so only a strong LM -- lm_w = 4, which
# makes the unbiased search prefer the empty hypothesis -- leaves the phrases something to change), returned entries were revoked, and phrase
# tokens enter the pre-beam through their bias term alone.  K = 20 is left out: with 20 x 12 candidates a step some gap is below JOINT_DELTA in
# most utterances (3 of 9 qualify).
ATT_CASES = {
    "k4": (4, False, 0.0, 1.5, 1, 0.0),
    "k4_lm": (4, True, 0.5, 1.5, 0, 0.0),
    "k4_lm4": (4, True, 4.0, 3.0, 0, 0.0),
    "k6_lm4": (6, True, 4.0, 1.5, 1, 0.0),
    "k4_min": (4, False, 0.0, 2.0, 2, 0.5),
}
JOINT_CASES = {
    "k4": ((0.5, 0.5, -1.0, 1), 4, False, 0.0, 3.0, 0, 0.0),
    "k6_lm_even": ((0.5, 0.5, 1.0, 2), 6, True, 0.5, 3.0, 1, 0.0),
    "k6_lm": ((0.7, 0.3, 1.0, 2), 6, True, 0.5, 3.0, 0, 0.0),
    "k4_att": ((0.9, 0.1, 0.0, 2), 4, False, 0.0, 8.0, 0, 0.0),
}
# CPU only, for the mutations: where the pre-beam's bias term decides results the CTC weight is high and the gaps are small (2 of 9 utterances
# qualify), so the case is not compared on the GPU
JOINT_MUT_CASES = {
    "prebeam": ((0.3, 0.7, 2.0, 3), 4, False, 0.0, 3.0, 2, 0.0),
}
JOINT_CASES_ALL = dict(JOINT_CASES, **JOINT_MUT_CASES)

_made, _runs = {}, {}
_MAXR = {}                                                   # case name -> max_step_ratio where it is not 1


def _models():
    if "models" not in _made:
        import hybrid_ref
        from decode_util import C_SMALL, joint_state_dict
        from oracle import ref_cpu
        from oracle.make_goldens import TINY, synth_batch
        sd = joint_state_dict(TINY, 7)
        sd_att = {k: v for k, v in sd.items() if k not in hybrid_ref.HEAD}
        _made["models"] = dict(sd=sd, sd_att=sd_att, p=hybrid_ref.leafify(sd, TINY), p_att=ref_cpu.leafify(sd_att, TINY),
                               lm=lm_ref.toy_lm(C_SMALL, jl.LM_ORDER, jl.LM_SEED), C=C_SMALL, cfg=TINY,
                               batches=[synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in jl.TINY_BATCHES])
    return _made["models"]


def _search(kind, name, trie, bias_w, **kw):
    """all nine utterances of a case under the engine's bf16 operand rounding"""
    from oracle import ref_cpu
    m = _models()
    with ref_cpu.bf16_emulation():
        if kind == "att":
            K, with_lm, lm_w, _, _, minr = ATT_CASES[name][:6]
            return [r for xs, il in m["batches"] for r in att_search(m["p_att"], m["cfg"], xs, il, K, m["lm"] if with_lm else None, lm_w, trie, bias_w,
                                                                     min_step_ratio=minr, max_step_ratio=_MAXR.get(name, 1.0), **kw)]
        (aw, cw, bo, N), K, with_lm, lm_w, _, _, minr = JOINT_CASES_ALL[name][:7]
        N = kw.pop("N", N)
        return [r for xs, il in m["batches"] for r in joint_search(m["p"], m["cfg"], xs, il, K, N, aw, cw, m["lm"] if with_lm else None, lm_w, bo, trie,
                                                                   bias_w, min_step_ratio=minr, max_step_ratio=_MAXR.get(name, 1.0), **kw)]


def make_case(kind, name):
    """-> dict(models' fields, K, with_lm, lm_w, bias_w, minr, joint: att_w / ctc_w / len_bonus / N, phrases, trie, unbiased: the unbiased search's
    results).  Built once per process and shared: callers leave it unchanged."""
    key = (kind, name)
    if key not in _made:
        m = _models()
        spec = ATT_CASES[name] if kind == "att" else JOINT_CASES_ALL[name][1:]
        K, with_lm, lm_w, bias_w, pseed, minr = spec[:6]
        per_utt = spec[6] if len(spec) > 6 else 6
        dummy = bias_ref.build([[1, 2]])
        if kind == "att":
            plain = _search(kind, name, dummy, 0.0, stop=False)
            hyps = [[h for h, _ in r["ended"][1:K]] for r in plain]
        else:
            plain = _search(kind, name, dummy, 0.0, stop=False, N=K)
            hyps = [[h for h, _, _ in r["nbest"][1:K]] for r in plain]
        phrases = cut_phrases(hyps, m["C"], pseed, per_utt)
        cs = dict(m, K=K, with_lm=with_lm, lm_w=lm_w, bias_w=bias_w, minr=minr, phrases=phrases, trie=bias_ref.build(phrases),
                  unbiased=_search(kind, name, dummy, 0.0))
        if kind == "joint":
            aw, cw, bo, N = JOINT_CASES_ALL[name][0]
            cs.update(att_w=aw, ctc_w=cw, len_bonus=bo, N=N)
        _made[key] = cs
    return _made[key]


def case_results(kind, name, stop=True, mutate=None, bias_w=None):
    """the restatement's results of a case (all nine utterances), computed once per process and variant"""
    key = (kind, name, stop, mutate, bias_w)
    if key not in _runs:
        cs = make_case(kind, name)
        _runs[key] = _search(kind, name, cs["trie"], cs["bias_w"] if bias_w is None else bias_w, stop=stop, mutate=mutate)
    return _runs[key]
