"""float64 restatement of the CTC loss of csrc/ctc.hip (include/masr.h masr_ctc_loss; mk_ctc_loss_joint): a plain helper module like
ctc_align_ref.py, no fixtures, no tests.  It also holds the cases that tests/test_hip_ctc_loss_kernels.py runs on the device, so that
tests/test_ctc_loss_ref_cpu.py can pin this module on exactly those inputs.

Semantics, restated: nn.CTCLoss(blank, reduction='mean', zero_infinity=True) on log_softmax(logits).  Per utterance b with n = in_len[b],
L = tgt_len[b], y = targets[tgt_off[b] .. + L), S = 2L + 1, label(s) = blank for even s, y[(s - 1) / 2] for odd s, lp_t = log_softmax(z_t):
  start       alpha_0(0) = lp_0(blank), alpha_0(1) = lp_0(y[0]) if L > 0, every other state -inf
  recursion   alpha_t(s) = lp_t(label(s)) + log(exp alpha_{t-1}(s) + exp alpha_{t-1}(s - 1) [s >= 1] + exp alpha_{t-1}(s - 2) [s odd, s >= 3,
              label(s) != label(s - 2)]); beta is its mirror image from frame n - 1 and the states S - 1, S - 2
  nll         -log(exp alpha_{n-1}(S - 1) + exp alpha_{n-1}(S - 2) [L > 0]); n = 0: 0 if L = 0 too, else +inf
  zero_infinity: an infinite nll (no path) counts 0 and has a zero gradient
  loss        mean_b(nll_b / max(L_b, 1))
  gradient    d loss / d z_t(c) = (softmax(z_t)(c) - sum_{s: label(s) = c} exp(alpha_t(s) + beta_t(s) - lp_t(c) - ll)) / (max(L, 1) B) for t < n,
              zero for t >= n: the derivative with respect to the LOGITS (folded through the softmax)
The lattice axis is vectorised; the frames are a Python loop."""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "nll nll_raw loss grad")
Case = namedtuple("Case", "name logits targets tgt_off in_len tgt_len blank feasible")


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


def _lattice(lp, ext):
    """lp float64 [n, C] log-probs, ext [S] -> (ll, alpha [n, S], beta [n, S]); n >= 1"""
    n, S = lp.shape[0], ext.size
    em = lp[:, ext]                                             # [n, S]
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]                       # into odd s >= 3 from s - 2
    ninf = -np.inf
    al, be = np.full((n, S), ninf), np.full((n, S), ninf)
    al[0, :2] = em[0, :2]
    with np.errstate(invalid="ignore"):
        for t in range(1, n):
            p = al[t - 1]
            a = p.copy()
            a[1:] = np.logaddexp(a[1:], p[:-1])
            a[skip] = np.logaddexp(a[skip], p[:-2][skip[2:]])
            al[t] = a + em[t]
        ll = np.logaddexp.reduce(al[n - 1, max(S - 2, 0):])
        be[n - 1, max(S - 2, 0):] = em[n - 1, max(S - 2, 0):]
        for t in range(n - 2, -1, -1):
            p = be[t + 1]
            a = p.copy()
            a[:-1] = np.logaddexp(a[:-1], p[1:])
            a[:-2][skip[2:]] = np.logaddexp(a[:-2][skip[2:]], p[skip])
            be[t] = a + em[t]
    return ll, al, be


def ctc_loss(logits, targets, tgt_off, in_len, tgt_len, blank=0):
    """logits [T][B][C]; targets int, utterance b's labels at targets[tgt_off[b] .. + tgt_len[b]) (any order, gaps allowed).
    -> Result(nll [B] with zero_infinity applied, nll_raw [B] with +inf where no path exists, loss, grad float64 [T][B][C])"""
    z = np.asarray(logits, np.float64)
    T, B, C = z.shape
    targets = np.asarray(targets, np.int64)
    lp = log_softmax(z)
    grad = np.zeros_like(z)
    raw = np.zeros(B)
    for b in range(B):
        n, L = int(in_len[b]), int(tgt_len[b])
        assert 0 <= n <= T and L >= 0
        y = targets[int(tgt_off[b]):int(tgt_off[b]) + L]
        assert y.size == L and np.all((y >= 0) & (y < C) & (y != blank))
        if n == 0:
            raw[b] = 0.0 if L == 0 else np.inf
            continue
        ext = np.full(2 * L + 1, blank, np.int64)
        ext[1::2] = y
        ll, al, be = _lattice(lp[:n, b], ext)
        raw[b] = -ll
        if not np.isfinite(ll):
            continue
        occ = np.exp(al + be - lp[:n, b][:, ext] - ll)             # [n, S]; a state no path crosses: exp(-inf) = 0
        post = np.zeros((C, n))
        np.add.at(post, ext, occ.T)
        grad[:n, b] = (np.exp(lp[:n, b]) - post.T) / (max(L, 1) * B)
    nll = np.where(np.isfinite(raw), raw, 0.0)
    loss = float(np.mean(nll / np.maximum(np.asarray(tgt_len, np.float64)[:B], 1.0)))
    return Result(nll, raw, loss, grad)


def concatenated(case):
    """the case's targets as torch's CTCLoss takes them: utterance after utterance, in order"""
    parts = [case.targets[int(o):int(o) + int(l)] for o, l in zip(case.tgt_off, case.tgt_len)]
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)


def padded(case):
    """-> (targets [B][Lmax] int32 flat, tgt_off = b * Lmax, Lmax): the layout of the transformer engine's gold array"""
    B, Lmax = len(case.tgt_len), max(1, int(max(case.tgt_len)))
    out = np.zeros((B, Lmax), np.int32)
    for b, (o, l) in enumerate(zip(case.tgt_off, case.tgt_len)):
        out[b, :int(l)] = case.targets[int(o):int(o) + int(l)]
    return out.reshape(-1), (np.arange(B) * Lmax).astype(np.int32), Lmax


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_hip_ctc_loss_kernels.py (seeded, built on the CPU)
def _labels(rng, n, C, blank):
    y = rng.integers(0, C - 1, n)                               # the C - 1 classes that are not the blank
    return (y + (y >= blank)).astype(np.int32)


def _scatter(rng, per_utt):
    """the utterances' label arrays laid out in a shuffled order with gaps (filled with an id no class has) -> (targets, tgt_off)"""
    order = rng.permutation(len(per_utt))
    off, chunks, pos = np.zeros(len(per_utt), np.int32), [], 0
    for b in order:
        gap = int(rng.integers(0, 3))
        chunks.append(np.full(gap, -7, np.int32))
        pos += gap
        off[b] = pos
        chunks.append(np.asarray(per_utt[b], np.int32))
        pos += len(per_utt[b])
    return np.concatenate(chunks + [np.full(1, -7, np.int32)]), off


def _make(name, seed, T, C, tgt_len, in_len, blank, scale, feasible, fixed=None):
    rng = np.random.default_rng(seed)
    B = len(tgt_len)
    logits = (rng.standard_normal((T, B, C)) * scale).astype(np.float32)
    per = [_labels(rng, int(l), C, blank) for l in tgt_len]
    for b, y in (fixed or {}).items():
        per[b] = np.asarray(y, np.int32)
        assert len(y) == tgt_len[b]
    targets, off = _scatter(rng, per)
    return Case(name, logits, targets, off, np.asarray(in_len, np.int32), np.asarray(tgt_len, np.int32), blank, tuple(feasible))


def case_wide(scale):
    """S = 257 (the first wide width), 601 (a ragged third stride), 255 (the last narrow width), 513 (two strides plus one), and an
    infeasible wide one (299 frames for 300 labels); 39 labels over hundreds of positions repeat, so both skip decisions occur"""
    return _make(f"wide-x{scale}", 101, 640, 40, [128, 300, 127, 256, 300], [640, 601, 400, 560, 299], 0, float(scale),
                 [True, True, True, True, False])


def case_limit():
    """the widest lattice the launcher accepts: S = 2047"""
    return _make("limit", 102, 1100, 40, [1023], [1100], 0, 1.0, [True])


VOCAB_CS = (2, 63, 64, 65, 512, 513, 577, 4096)


def case_vocab(C):
    """the wave's eight register slots (C <= 512) and the re-read tail (C > 512); class C - 1 is a target of two utterances"""
    if C == 2:
        return _make("vocab-2", 103, 8, 2, [1, 0, 1], [8, 5, 3], 0, 3.0, [True, True, True], {0: [1], 2: [1]})
    rng = np.random.default_rng(1000 + C)
    a, b2, c = (1 + rng.choice(C - 2, 3, replace=False)).tolist()  # three distinct labels below C - 1
    return _make(f"vocab-{C}", 103, 8, C, [2, 0, 3], [8, 5, 3], 0, 3.0, [True, True, True], {0: [C - 1, a], 2: [b2, C - 1, c]})


def case_short(blank=0):
    """in_len 1, 2, 5, 6, 7, 8, 12, 13 around the PF = 6 prefetch ring of the narrow sweep, the empty target, and in_len == tgt_len = 3 with
    distinct labels (feasible) and with a repeat (infeasible)"""
    lab = [c for c in range(9) if c != blank]
    return _make(f"short-blank{blank}", 104, 13, 9, [0, 1, 2, 3, 3, 1, 2, 3, 3, 3], [1, 2, 5, 6, 7, 8, 12, 13, 3, 3], blank, 1.0,
                 [True] * 9 + [False], {8: [lab[2], lab[0], lab[5]], 9: [lab[3], lab[3], lab[6]]})


def all_cases():
    return ([case_wide(1), case_wide(8), case_limit()] + [case_vocab(C) for C in VOCAB_CS] + [case_short(0), case_short(8), case_short(4)])
