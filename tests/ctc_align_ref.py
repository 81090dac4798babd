"""CPU restatements of masr_ctc_align (include/masr.h): a plain helper module like ctc_beam_ref.py, no fixtures, no tests.

Semantics, restated.  n = enc_len, L = tgt_len, S = 2L + 1, label(s) = blank for even s, y[(s - 1) / 2] for odd s.
  emissions   u_t(c) = fl(z_t(c) - max_t), max_t the row maximum over the C classes: one fp32 subtraction
  start       v_0(0) = u_0(blank), v_0(1) = u_0(y[0]) if L > 0, every other state -inf
  recursion   v_t(s) = fl(m + u_t(label(s))), m the largest of v_{t-1}(s) [back-pointer 0], v_{t-1}(s - 1) [1, s >= 1] and v_{t-1}(s - 2)
              [2, s odd, s >= 3, label(s) != label(s - 2)]; a tie goes to the smaller back-pointer; m = -inf: state -inf, back-pointer 0
  end         the final state is S - 1, or S - 2 if L > 0 and v_{n-1}(S - 2) > v_{n-1}(S - 1) (a tie: S - 1); the back-pointers are walked from there
  score       acc = 0.f; for t = 0 .. n - 1 in order: acc = fl(acc + lsum_t), lsum_t = fp32 log sum_c exp(u_t(c)); score = fl(v_{n-1}(final) - acc)
  frames      [Tp]: at t < n the target index i of state 2i + 1, -1 in a blank state; -2 at t >= n
  start, end  [maxL]: first frame of token i and one past its last; -1 for i >= L
  L = 0: the all-blank path (n = 0 too: score 0).  Infeasible (both final states -inf; n = 0 with L > 0): score -inf, frames -2, start / end -1.
  Refused (tgt_len < 0 or > maxL, a token outside [0, C) or equal to blank): score NaN, the rest as for infeasible.

align_f32 is the restatement: fp32 additions and comparisons in that order, so its path equals the kernels' bit for bit on the same logits.
Its lsum is numpy's fp32 log / exp, not the device's, so its score is the kernels' only up to the log-sum's error (lse_err_bound).
viterbi_f64 is the fp64 optimum on log_softmax; path_logprob_f64 the fp64 log-probability of a given path; brute_force enumerates."""
import itertools

import numpy as np

F = np.float32
NEG = F(-np.inf)


def emissions(z):
    """z fp32 [n, C] -> u fp32 [n, C]"""
    z = np.asarray(z, F)
    return (z - z.max(axis=1, keepdims=True)).astype(F) if len(z) else z


def refused(y, L, maxL, C, blank):
    return L < 0 or L > maxL or any(t < 0 or t >= C or t == blank for t in y[:max(L, 0)])


def outputs(Tp, maxL, n, L, states):
    """frames [Tp], start [maxL], end [maxL] of the state sequence `states` (None: infeasible or refused)"""
    frames, start, end = np.full(Tp, -2, np.int32), np.full(maxL, -1, np.int32), np.full(maxL, -1, np.int32)
    if states is None:
        return frames, start, end
    for t, s in enumerate(states):
        frames[t] = s >> 1 if s & 1 else -1
    for t in range(n):
        i = frames[t]
        if i >= 0 and (t == 0 or frames[t - 1] != i):
            start[i] = t
        if i >= 0 and (t == n - 1 or frames[t + 1] != i):
            end[i] = t + 1
    return frames, start, end


def align_f32(z, n, y, blank, Tp=None, maxL=None):
    """z fp32 [>= n, C] (rows past n are not read), y the target list -> dict(score, v, frames, start, end, states)"""
    C = z.shape[1]
    L = len(y)
    Tp = len(z) if Tp is None else Tp
    maxL = L if maxL is None else maxL
    n = min(max(int(n), 0), Tp)
    if refused(list(y), L, maxL, C, blank):
        return dict(score=F(np.nan), v=F(np.nan), states=None, **dict(zip(("frames", "start", "end"), outputs(Tp, maxL, n, 0, None))))
    S = 2 * L + 1
    lab = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    u = emissions(z[:n, :C])
    states, vfin = None, NEG
    if n == 0:
        if L == 0:
            states, vfin = [], F(0.0)
    else:
        lab_a = np.asarray(lab)
        skip = np.zeros(S, bool)
        skip[3::2] = lab_a[3::2] != lab_a[1:-2:2]
        v = np.full(S, NEG, F)
        v[0] = u[0, blank]
        if L > 0:
            v[1] = u[0, lab[1]]
        bp = np.zeros((n, S), np.int8)
        for t in range(1, n):                                   # all states of a frame at once; per state the scalar rule above
            m, d = v.copy(), bp[t]
            c1 = np.concatenate(([NEG], v[:-1]))
            k = c1 > m
            m[k], d[k] = c1[k], 1
            c2 = np.concatenate(([NEG, NEG], v[:-2]))[:S]
            k = skip & (c2 > m)
            m[k], d[k] = c2[k], 2
            dead = m == NEG
            d[dead] = 0
            with np.errstate(invalid="ignore"):
                v = (m + u[t, lab_a]).astype(F)
            v[dead] = NEG
        fin = S - 1
        if L > 0 and v[S - 2] > v[S - 1]:
            fin = S - 2
        vfin = v[fin]
        if vfin != NEG:
            states = [fin]
            for t in range(n - 1, 0, -1):
                states.append(states[-1] - int(bp[t, states[-1]]))
            states.reverse()
    if states is None:
        score = NEG
    else:
        acc = F(0.0)
        with np.errstate(over="ignore"):
            for t in range(n):
                acc = F(acc + np.log(np.exp(u[t]).sum(dtype=F), dtype=F))
        score = F(vfin - acc)
    frames, start, end = outputs(Tp, maxL, n, L, states)
    return dict(score=score, v=vfin, states=states, frames=frames, start=start, end=end)


def collapse(frames, y):
    """the token sequence a frames row spells: the targets of its runs of equal indices >= 0"""
    idx = [int(i) for i in frames if i != -2]
    return [int(y[i]) for k, i in enumerate(idx) if i >= 0 and (k == 0 or idx[k - 1] != i)]


def log_softmax_f64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def path_logprob_f64(z, n, y, blank, frames):
    """fp64 log-probability of the path `frames` describes -> (log-prob, M = the largest partial sum in magnitude on the way: of the
    max-shifted emissions, of the normalisers, and the result)"""
    zz = np.asarray(z[:n], np.float64)
    u = zz - zz.max(axis=1, keepdims=True) if n else zz
    ls = np.log(np.exp(u).sum(axis=1)) if n else np.zeros(0)
    a = b = M = 0.0
    for t in range(n):
        i = int(frames[t])
        a += u[t, blank if i < 0 else int(y[i])]
        b += ls[t]
        M = max(M, abs(a), abs(b))
    return a - b, max(M, abs(a - b))


def viterbi_f64(z, n, y, blank):
    """the fp64 optimum over all alignments on log_softmax(z) -> (best log-prob or -inf, M)"""
    L, S = len(y), 2 * len(y) + 1
    if n == 0:
        return (0.0 if L == 0 else -np.inf), 0.0
    lp = log_softmax_f64(z[:n])
    lab = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    v = np.full(S, -np.inf)
    v[0] = lp[0, blank]
    if L:
        v[1] = lp[0, lab[1]]
    M = float(np.abs(v[np.isfinite(v)]).max())
    lab_a = np.asarray(lab)
    skip = np.zeros(S, bool)
    skip[3::2] = lab_a[3::2] != lab_a[1:-2:2]
    for t in range(1, n):
        m = np.maximum(v, np.concatenate(([-np.inf], v[:-1])))
        m = np.where(skip, np.maximum(m, np.concatenate(([-np.inf, -np.inf], v[:-2]))[:S]), m)
        v = m + lp[t, lab_a]
        fin = v[np.isfinite(v)]
        if len(fin):
            M = max(M, float(np.abs(fin).max()))
    return float(max(v[S - 1], v[S - 2] if L else -np.inf)), M


def lse_err_bound(z, n):
    """Bound on sum over t < n of |device lsum_t - log sum_c exp(u_t(c))|, from the formats (u exact in fp64 here).
    exp(u) is exp2(fl(u * log2 e)): the product's rounding moves the result by a relative |u| 2^-24, the hardware exp2 by 2 ulp = 2^-22; the
    sum of C such terms in a strided-then-tree order carries a relative (C / 64 + 7) 2^-24 of s; a relative error of s is an absolute one
    of log s; the hardware log2 (1 ulp) times ln 2 (rounded) moves log s by a relative 2^-22, taken of max(log s, 1)."""
    zz = np.asarray(z[:n], np.float64)
    if not n:
        return 0.0
    u = zz - zz.max(axis=1, keepdims=True)
    e = np.exp(u)
    s = e.sum(axis=1)
    C = zz.shape[1]
    rel = (e * (np.abs(u) * 2.0 ** -24 + 2.0 ** -22)).sum(axis=1) / s + (C / 64 + 7) * 2.0 ** -24
    return float((rel + 2.0 ** -22 * np.maximum(np.log(s), 1.0)).sum())


def score_bound(z, n, M, on_grid=True):
    """|fp32 score - fp64 log-prob of the same path|: the n additions of acc, the final subtraction and one more in hand, each half an ulp of
    a partial sum of at most M: 2^-24 (n + 2) M, plus the log-sums' own error.  That is the whole of it where the logits lie on a grid that
    makes the emissions and the n - 1 additions of v exact, as the kernel tests' do (on_grid).  On other logits (the models') those additions
    round too, n 2^-24 M more, and so does each emission's one subtraction, n 2^-24 max|u| more: 2^-24 ((2 n + 2) M + n max|u|) in all."""
    b = 2.0 ** -24 * (n + 2) * M + lse_err_bound(z, n)
    if not on_grid and n:
        zz = np.asarray(z[:n], np.float64)
        b += 2.0 ** -24 * n * (M + float(np.abs(zz - zz.max(axis=1, keepdims=True)).max()))
    return b


def brute_force(z, n, y, blank):
    """Every class sequence of n frames that collapses to y, scored in fp32 in frame order on the emissions; the winner under the tie rule
    (among the best, the state sequence that is largest read from the last frame backwards: the end prefers S - 1, every step the smaller
    back-pointer) -> (v, states) or (-inf, None)"""
    C, L = z.shape[1], len(y)
    u = emissions(z[:n, :C])
    best, best_states = NEG, None
    for path in itertools.product(range(C), repeat=n):
        i, prev, states = -1, blank, []
        for c in path:
            if c != blank and c != prev:
                i += 1
            if i >= L or (c != blank and y[i] != c):
                states = None
                break
            states.append(2 * i + 1 if c != blank else 2 * (i + 1))
            prev = c
        if states is None or i != L - 1:
            continue
        v = F(0.0)
        for t, c in enumerate(path):
            v = F(u[t, c]) if t == 0 else F(v + u[t, c])
        if best_states is None or v > best or (v == best and states[::-1] > best_states[::-1]):
            best, best_states = v, states
    return best, best_states
