"""CPU restatement of LSTM LM shallow fusion (include/masr.h masr_recog_beam_nlm / masr_nlm_score).  A plain helper module like
lm_ref.py: no fixtures, no tests.

The LM is a dict of fp32 numpy arrays: embed [C][E], w_ih / w_hh / b_ih / b_hh (lists, one entry per layer, torch.nn.LSTM's shapes and gate
order i, f, g, o), lo_w [C][H], lo_b [C], start_id.  One step feeds a token into the layer stack and returns the fp32 log_softmax row and the new
state [(h, c) per layer].  With emulate=True the engine's rounding points are restated: embedding rows, every weight matrix and h are bf16
values (h is rounded when it is stored, and only that form is ever read), products are accumulated in fp32, gates, c, the bias
fl(b_ih + b_hh), the output bias and the logits are fp32.  The accumulation ORDER is numpy's, not the kernel's: the comparison with the engine is
a tolerance, never bits.

The search is lm_ref.beam_search_lm_one with the fused row swapped, and it moves the LM state as the device does: per step an array of K slots,
row k reads its PARENT's slot of the step before and writes its own.  `mut` names a deliberately wrong variant (test_nlm_ref_cpu.py shows
that each changes results, so the comparison with the engine can see such a bug):
    gates     the f and g gates swapped            own_slot   the state is read from the row's own slot instead of its parent's
    no_reset  the start token continues the state that the slot held (the previous utterance's) instead of the zero state
    h_fp32    h is left unrounded
"""
import math

import numpy as np
import torch

import beam_ref

MUTATIONS = ("gates", "own_slot", "no_reset", "h_fp32")


def toy_nlm(C, E, H, L, seed, start_id=0, eos_bias=0.0):
    """uniform(-a, a) draws in a fixed order: embed (a = 1), lo_w (6.8 / sqrt(H)), lo_b (0.5; then lo_b[0] = -30: class 0 is sos, never a
    token), per layer w_ih (2 / sqrt(in)), w_hh (2 / sqrt(H)), b_ih (0.5); b_hh = 0.  eos_bias is subtracted from lo_b[C - 1] behind the
    draws: an LM that expects long sentences (every other class's log-prob moves up by the same amount per row, their order stays)"""
    rng = np.random.RandomState(seed)
    u = lambda a, *shape: rng.uniform(-a, a, size=shape).astype(np.float32)  # noqa: E731
    m = {"embed": u(1.0, C, E), "lo_w": u(6.8 / math.sqrt(H), C, H), "lo_b": u(0.5, C), "w_ih": [], "w_hh": [], "b_ih": [], "b_hh": [],
         "start_id": start_id}
    m["lo_b"][0] = -30.0
    m["lo_b"][C - 1] -= np.float32(eos_bias)
    for l in range(L):
        n_in = H if l else E
        m["w_ih"].append(u(2.0 / math.sqrt(n_in), 4 * H, n_in))
        m["w_hh"].append(u(2.0 / math.sqrt(H), 4 * H, H))
        m["b_ih"].append(u(0.5, 4 * H))
        m["b_hh"].append(np.zeros(4 * H, dtype=np.float32))
    return m


def to_state_dict(m, layout="project"):
    """the dict form -> a state dict in one of the two key layouts masr_amd.nlm accepts"""
    t = torch.from_numpy
    if layout == "project":
        sd = {"embed.weight": t(m["embed"]), "lo.weight": t(m["lo_w"]), "lo.bias": t(m["lo_b"])}
        for l in range(len(m["w_ih"])):
            sd.update({f"rnn.weight_ih_l{l}": t(m["w_ih"][l]), f"rnn.weight_hh_l{l}": t(m["w_hh"][l]), f"rnn.bias_ih_l{l}": t(m["b_ih"][l]),
                       f"rnn.bias_hh_l{l}": t(m["b_hh"][l])})
        return sd
    sd = {"predictor.embed.weight": t(m["embed"]), "predictor.lo.weight": t(m["lo_w"]), "predictor.lo.bias": t(m["lo_b"])}
    for l in range(len(m["w_ih"])):
        sd.update({f"predictor.rnn.{l}.weight_ih": t(m["w_ih"][l]), f"predictor.rnn.{l}.weight_hh": t(m["w_hh"][l]),
                   f"predictor.rnn.{l}.bias_ih": t(m["b_ih"][l]), f"predictor.rnn.{l}.bias_hh": t(m["b_hh"][l])})
    return sd


def torch_modules(m):
    """torch.nn.Embedding / LSTM / Linear holding the dict's weights"""
    C, E = m["embed"].shape
    H, L = m["w_hh"][0].shape[1], len(m["w_ih"])
    emb, rnn, lo = torch.nn.Embedding(C, E), torch.nn.LSTM(E, H, L), torch.nn.Linear(H, C)
    sd = to_state_dict(m)
    with torch.no_grad():
        emb.weight.copy_(sd["embed.weight"]); lo.weight.copy_(sd["lo.weight"]); lo.bias.copy_(sd["lo.bias"])
        for l in range(L):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(rnn, f"{n}_l{l}").copy_(sd[f"rnn.{n}_l{l}"])
    return emb, rnn, lo


def bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def _weights(m, emulate):
    key = "_bf16" if emulate else "_fp32"
    if key not in m:
        r = bf16 if emulate else (lambda x: np.asarray(x, dtype=np.float32))
        m[key] = {"embed": r(m["embed"]), "lo_w": r(m["lo_w"]), "w_ih": [r(w) for w in m["w_ih"]], "w_hh": [r(w) for w in m["w_hh"]],
                  "b": [(bi + bh).astype(np.float32) for bi, bh in zip(m["b_ih"], m["b_hh"])]}
    return m[key]


def zero_state(m):
    H = m["w_hh"][0].shape[1]
    return [(np.zeros(H, dtype=np.float32), np.zeros(H, dtype=np.float32)) for _ in m["w_ih"]]


def _sig(x):
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def log_softmax32(y):
    y = y.astype(np.float32)
    mx = y.max()
    return ((y - mx) - np.log(np.exp(y - mx, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)).astype(np.float32)


def step(m, tok, state, emulate=True, mut=None):
    """feed `tok` from `state` -> (fp32 log_softmax row [C], new state)"""
    w = _weights(m, emulate)
    H = m["w_hh"][0].shape[1]
    x = w["embed"][tok]
    new = []
    for l, (h_prev, c_prev) in enumerate(state):
        z = (w["w_ih"][l] @ x + w["w_hh"][l] @ h_prev).astype(np.float32) + w["b"][l]
        zi, zf, zg, zo = (z[g * H:(g + 1) * H] for g in range(4))
        if mut == "gates":
            zf, zg = zg, zf
        c = (_sig(zf) * c_prev + _sig(zi) * np.tanh(zg, dtype=np.float32)).astype(np.float32)
        h = (_sig(zo) * np.tanh(c, dtype=np.float32)).astype(np.float32)
        if emulate and mut != "h_fp32":
            h = bf16(h)
        new.append((h, c))
        x = h
    y = (w["lo_w"] @ x).astype(np.float32) + m["lo_b"]
    return log_softmax32(y), new


def _after(m, h, emulate, cache):
    """(row, state) after feeding [start] + h from the zero state, cached per prefix"""
    h = tuple(h)
    if h not in cache:
        state = zero_state(m) if not h else _after(m, h[:-1], emulate, cache)[1]
        cache[h] = step(m, h[-1] if h else m["start_id"], state, emulate)
    return cache[h]


def lm_row(m, h, emulate=True):
    """lm(. | h) for every class: the fp32 log_softmax row after feeding [start] + h from the zero state"""
    return _after(m, h, emulate, m.setdefault("_rows_bf16" if emulate else "_rows_fp32", {}))[0]


def score(m, tokens, emulate=True):
    """the teacher-forced log-probability of tokens + [eos], fp32 additions in position order"""
    eos = m["embed"].shape[0] - 1
    acc = np.float32(0.0)
    for i, t in enumerate(list(tokens) + [eos]):
        acc = np.float32(acc + lm_row(m, tokens[:i], emulate)[t])
    return float(acc)


# ---------------------------------------------------------------- the search
def fuse(lp_row, lm_rowv, lm_w):
    """f(c) = fl(lp(c) + fl(lm_w * lm(c))) for every class, fp32, two roundings"""
    return (lp_row.astype(np.float32) + (np.float32(lm_w) * lm_rowv).astype(np.float32)).astype(np.float32)


def beam_search_nlm_one(p, cfg, memory_b, mask_b, K, maxlen, minlen, m, lm_w, emulate=True, mut=None, slots=None):
    """lm_ref.beam_search_lm_one with the LSTM LM's fused row; slots: the K state slots as the previous decode left them (no_reset reads them)"""
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    running = [((), np.float32(0.0), 0)]                    # (tokens, score, parent slot)
    prev = slots if slots is not None else [zero_state(m) for _ in range(K)]
    ended = []
    sel_gaps, stop_gaps = [], []
    for t in range(1, maxlen + 1):
        z = beam_ref.last_logits(p, cfg, memory_b, mask_b, [h for h, _, _ in running])
        lp = beam_ref.log_softmax32(z).numpy()
        cur = list(prev)                                    # (slots of rows that do not run keep what they held)
        cands = []
        for k, (h, ps, par) in enumerate(running):
            src = prev[k if mut == "own_slot" else par]
            if t == 1 and mut != "no_reset":
                src = zero_state(m)
            row, cur[k] = step(m, h[-1] if h else m["start_id"], src, emulate, mut)
            f = fuse(lp[k], row, lm_w)
            sc = (ps + f).astype(np.float32)
            for c in range(C):
                if c == eos and len(h) < minlen:
                    continue
                cands.append((float(sc[c]), k, float(f[c]), c))
        prev = cur
        cands.sort(key=lambda x: (-x[0], x[1], -x[2], x[3]))
        if len(cands) > K:
            sel_gaps.append(cands[K - 1][0] - cands[K][0])
        nxt = []
        for i, (sc, k, _, c) in enumerate(cands[:K]):
            h = running[k][0]
            if c == eos:
                ended.append((sc, t, i, h))
            else:
                nxt.append((h + (c,), np.float32(sc), k))
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
    if slots is not None:
        slots[:] = prev
    return {"tokens": list(ended[0][3]), "score": ended[0][0], "sel_gaps": sel_gaps, "stop_gaps": stop_gaps, "end_gap": end_gap}


@torch.no_grad()
def beam_search_nlm(p, cfg, xs, ilens, K, m, lm_w, min_step_ratio=0.0, max_step_ratio=1.0, emulate=True, mut=None, slots=None):
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    if slots is None and mut == "no_reset":
        slots = [zero_state(m) for _ in range(K)]
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        out.append(beam_search_nlm_one(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], K, maxlen, minlen, m, lm_w, emulate, mut, slots))
    return out


@torch.no_grad()
def greedy_nlm(p, cfg, xs, ilens, m, lm_w, min_step_ratio=0.0, max_step_ratio=1.0, emulate=True):
    """step-by-step arg-max of the fused increment (first maximal class; eos excluded below minlen), stopped at eos or maxlen ->
    [(tokens, score)]"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    out = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        C = p["char_trans.weight"].shape[0]
        h, s = (), np.float32(0.0)
        for t in range(1, maxlen + 1):
            z = beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [h])
            f = fuse(beam_ref.log_softmax32(z).numpy()[0], lm_row(m, h, emulate), lm_w)
            if len(h) < minlen:
                f = f.copy(); f[C - 1] = -np.inf
            c = int(np.argmax(f))
            s = np.float32(s + f[c])
            if c == C - 1:
                break
            h = h + (c,)
        out.append((list(h), float(s)))
    return out


@torch.no_grad()
def exhaustive_nlm(p, cfg, xs, ilens, m, lm_w, min_step_ratio=0.0, max_step_ratio=1.0, emulate=True):
    """beam_ref.exhaustive with the fused increment (tiny vocabularies only) -> [(tokens, score)]"""
    memory, pad_mask, enc_lens = beam_ref.encode(p, cfg, xs, torch.as_tensor(ilens))
    C = p["char_trans.weight"].shape[0]
    eos = C - 1
    res = []
    for b in range(xs.shape[0]):
        maxlen, minlen = beam_ref.beam_lengths(int(enc_lens[b]), min_step_ratio, max_step_ratio)
        best = (-math.inf, None)
        frontier = [((), np.float32(0.0))]
        for t in range(1, maxlen + 1):
            lp = beam_ref.log_softmax32(beam_ref.last_logits(p, cfg, memory[:, b:b + 1], pad_mask[b:b + 1], [h for h, _ in frontier])).numpy()
            nxt = []
            for k, (h, ps) in enumerate(frontier):
                sc = (ps + fuse(lp[k], lm_row(m, h, emulate), lm_w)).astype(np.float32)
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
