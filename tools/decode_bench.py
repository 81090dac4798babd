"""What the decoder benchmark scripts share (bench_beam, bench_joint_beam, bench_ctc_beam, bench_lm_beam, bench_ctc_lm_beam,
bench_joint_lm_beam, bench_nlm_joint_beam, bench_rescore): the hkust geometry, an engine on it, the synthetic n-gram LM and the timing loop.  Importing it
runs nothing; the scripts put the repository root on sys.path first."""
import time

import numpy as np
import torch

C_ = 367                                                        # hkust output classes
HKUST = {"idim": 80, "nheads": 8, "d_model": 512, "d_inner": 2048, "dropout": 0.1, "pos_dropout": 0.1, "tgt_share_weight": 1,
         "encoder": {"nlayers": 2}, "decoder": {"nlayers": 4}}
HKUST_CTC = dict(HKUST, ctc_weight=0.3)                         # with a CTC head


def hkust_engine(ctc: bool, seed=531):
    """a MasrEngine on the hkust geometry (ctc: with a CTC head) holding the reference-replay init; seeds torch first (seed None: not)"""
    from masr_amd.engine import MasrEngine
    from masr_amd.model import reference_init_state_dict
    cfg = HKUST_CTC if ctc else HKUST
    if seed is not None:
        torch.manual_seed(seed)
    eng = MasrEngine(cfg, C_)
    eng.load_state_dict(reference_init_state_dict(cfg, C_))
    return eng


def synthetic_lm(n_total, seed=7):
    """order 3 over C_ classes, n_total n-grams in all: dense unigrams, distinct random bigrams (at most half of n_total; there are only
    365^2 of them) and distinct random trigrams of the units 1 .. C_ - 2, random values"""
    from masr_amd.lm import NGramLM
    rng = np.random.RandomState(seed)
    U = C_ - 2
    grams = [np.arange(C_, dtype=np.int32).reshape(-1, 1)]
    want = {2: min(U * U, n_total // 2)}
    want[3] = n_total - C_ - want[2]
    for n in (2, 3):
        total = U ** n
        idx = np.unique(rng.randint(total, size=int(want[n] * 1.2) + 16)) if want[n] < total else np.arange(total)
        idx = rng.permutation(idx)[:want[n]]
        grams.append(np.stack([(idx // U ** (n - 1 - j)) % U + 1 for j in range(n)], axis=1).astype(np.int32))
    logp = [(-8.0 * rng.rand(len(g))).astype(np.float32) for g in grams]
    bo = [(-2.0 * rng.rand(len(g))).astype(np.float32) for g in grams]
    return NGramLM(3, C_, grams, logp, bo)


def timed(fn, n, stream=None):
    """ms per call over n calls of fn behind one warm-up call, all on `stream` (None: the current one) -> (ms, what the warm-up call returned)"""
    with torch.cuda.stream(stream):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for _ in range(n):
            fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, out
