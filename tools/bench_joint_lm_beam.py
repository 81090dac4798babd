"""What the n-gram LM, the length bonus and the N-best list cost over the joint CTC/attention beam: masr_recog_beam_ctc and
masr_recog_beam_ctc_lm side by side in one process on the hkust geometry with a CTC head, B = 16, T = 1000 (as tools/bench_joint_beam.py),
random-init weights, K = 1 / 4 / 10 / 20, N = 1 and N = K, with tools/bench_lm_beam.py's synthetic 3-gram LM of about 10^6 n-grams.  Every
decode replays its step graph Lmax = T / 4 times whatever the stop rule decides, so ms per step = ms per decode / steps includes the
encoder's share in all columns alike; the difference of two columns is the fused pre-beam, the LM prefix kernel and the N-best select
against the joint beam's three step kernels.  For per-launch times run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_joint_lm_beam.py` and read beam_ctc_lm_prebeam_kernel, beam_ctc_prefix_kernel and
beam_select_nbest_kernel in the stats.
usage: python tools/bench_joint_lm_beam.py [B] [T] [n-grams in all]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd.engine import MasrEngine
from masr_amd.lm import NGramLM
from masr_amd.model import reference_init_state_dict

HKUST = {"idim": 80, "nheads": 8, "d_model": 512, "d_inner": 2048, "dropout": 0.1, "pos_dropout": 0.1, "tgt_share_weight": 1,
         "encoder": {"nlayers": 2}, "decoder": {"nlayers": 4}, "ctc_weight": 0.3}
C_ = 367
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
N_TOTAL = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
ATT_W, CTC_W, LM_W, BONUS = 0.7, 0.3, 0.3, 0.5


def synthetic_lm(n_total, seed=7):
    """tools/bench_lm_beam.py's: order 3 over C_ classes, n_total n-grams in all -- dense unigrams, distinct random bigrams (at most half of
    n_total) and distinct random trigrams of the units 1 .. C_ - 2, random values"""
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


torch.manual_seed(531)
eng = MasrEngine(HKUST, C_)
eng.load_state_dict(reference_init_state_dict(HKUST, C_))
lm = synthetic_lm(N_TOTAL)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "lm_ngrams": lm.counts, "weights": [ATT_W, CTC_W, LM_W, BONUS], "decode_ms": {}}


def timed(fn, n=3):
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, out


for K in (1, 4, 10, 20):
    joint, _ = timed(lambda: eng.recog_beam(xs, il, K, att_weight=ATT_W, ctc_weight=CTC_W))
    row = {"joint": round(joint, 2), "joint_step": round(joint / steps, 4)}
    line = f"K = {K:2d}: joint {joint:8.2f} ms ({joint / steps:.4f} per step)"
    for N in sorted({1, K}):
        ms, lists = timed(lambda: eng.recog_beam_ctc_lm(xs, il, K, lm, LM_W, BONUS, N, att_weight=ATT_W, ctc_weight=CTC_W))
        row[f"joint_lm_N{N}"] = round(ms, 2)
        row[f"joint_lm_N{N}_step"] = round(ms / steps, 4)
        row[f"extra_us_per_step_N{N}"] = round((ms - joint) / steps * 1e3, 1)
        row[f"mean_entries_N{N}"] = sum(len(u) for u in lists) / B
        line += f"  + LM, N = {N:2d}: {ms:8.2f} ms ({ms / steps:.4f} per step, {(ms - joint) / steps * 1e3:+6.1f} us)"
    res["decode_ms"][f"K{K}"] = row
    print(line, flush=True)
print(json.dumps(res))
