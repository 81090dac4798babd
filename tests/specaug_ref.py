"""SpecAugment as include/masr.h masr_specaug defines it, restated in numpy for the tests: every draw is an integer computed
with Python ints (the hash of csrc/common.h, the multiply-shift `uni`), every value is fp64.  No GPU, no libmasr."""
import numpy as np

M32 = 0xFFFFFFFF
SITE = 0x53504147
KEYS = ("time_warp", "freq_masks", "freq_width", "freq_bins", "time_masks", "time_width", "time_ratio")


def mix32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def dropout_key(seed, site):
    return mix32((seed * 0x9E3779B1 + site * 0x85EBCA77 + 0x632BE5AB) & M32)


def dropout_word(key, idx):
    return mix32((idx ^ key) & M32)


def step_seed(seed, step):
    """the 32-bit seed of one step, from the position masr_dropout_state reports"""
    return ((((seed * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 32) + (step & M32) * 7919) & M32


def uni(w, r):
    return (w * r) >> 32


def full_policy(policy, D):
    p = {k: 0 for k in KEYS}
    p["freq_bins"] = D
    p.update(policy or {})
    return p


def draws(policy, D, n, b, seed, step):
    """the draws of utterance b (length n): {'warp': (c, c') or None, 'freq': [(f0, f)], 'time': [(t0, tau)]}"""
    p = full_policy(policy, D)
    key = dropout_key(step_seed(seed, step), SITE)
    word = lambda j: dropout_word(key, (b * 64 + j) & M32)
    W, Df = p["time_warp"], p["freq_bins"]
    warp = None
    if W > 0 and n > 2 * W:
        c = W + uni(word(0), n - 2 * W)
        warp = (c, c + uni(word(1), 2 * W - 1) - (W - 1))
    freq = []
    for i in range(p["freq_masks"]):
        f = uni(word(2 + 2 * i), min(p["freq_width"], Df) + 1)
        freq.append((uni(word(3 + 2 * i), Df - f + 1), f))
    cap = min(p["time_width"], int(np.floor(np.float32(p["time_ratio"]) * np.float32(n))))      # one fp32 product
    time = []
    for i in range(p["time_masks"]):
        tau = uni(word(18 + 2 * i), cap + 1)
        time.append((uni(word(19 + 2 * i), n - tau + 1), tau))
    return {"warp": warp, "freq": freq, "time": time}


def source_rows(n, warp):
    """per output row t < n: (i, r, den) -- the row reads source position i + r / den"""
    i, r, den = np.arange(n), np.zeros(n, np.int64), np.ones(n, np.int64)
    if warp is None:
        return i, r, den
    c, cw = warp
    for t in range(n):
        num, d, base = (t * c, cw, 0) if t < cw else ((t - cw) * (n - 1 - c), n - 1 - cw, c)
        i[t], r[t], den[t] = base + num // d, num % d, d
    return i, r, den


def specaug(xs, ilens, policy, seed, step):
    """xs [B, T, D] (any float dtype; rows >= ilens[b] are never read), ilens [B] -> (out fp64 [B, T, D], a, b, kind):
    a / b fp64 [B, T, D] = the two source values a cell was interpolated from (a alone where it was copied), kind int8 [B, T, D] =
    0 zero (padding or mask), 1 copied bit for bit, 2 interpolated."""
    xs = np.asarray(xs)
    B, T, D = xs.shape
    out = np.zeros((B, T, D), np.float64)
    a, bb, kind = np.zeros_like(out), np.zeros_like(out), np.zeros((B, T, D), np.int8)
    for b in range(B):
        n = int(ilens[b])
        dr = draws(policy, D, n, b, seed, step)
        i, r, den = source_rows(n, dr["warp"])
        x = xs[b, :n].astype(np.float64)
        lo = x[i]
        hi = x[np.minimum(i + 1, n - 1)]
        assert np.all((r == 0) | (i + 1 <= n - 1))
        phi = (r / den)[:, None]
        val = np.where(r[:, None] == 0, lo, lo + phi * (hi - lo))
        k = np.where(r[:, None] == 0, 1, 2) * np.ones((1, D), np.int8)
        for f0, f in dr["freq"]:
            val[:, f0:f0 + f] = 0.0; k[:, f0:f0 + f] = 0
        for t0, tau in dr["time"]:
            val[t0:t0 + tau] = 0.0; k[t0:t0 + tau] = 0
        out[b, :n], a[b, :n], bb[b, :n], kind[b, :n] = val, lo, hi, k
    return out, a, bb, kind
