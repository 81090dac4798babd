"""What n-gram LM shallow fusion costs over the plain attention beam: masr_recog_beam and masr_recog_beam_lm side by side in one process on
the hkust geometry, B = 16, T = 1000 (as tools/bench_beam.py), random-init weights, K = 1 / 4 / 10 / 20, with a synthetic 3-gram LM of about
10^6 n-grams over the 367 classes (random n-grams with random log-probabilities: the kernel's work -- up to two table probes and the dense
unigram per class -- does not depend on the values).  Both decodes replay all T / 4 steps (random weights never end a hypothesis early at
lm_w = 0.3 with min_step_ratio = 1), so ms per step = ms per decode / steps includes the encoder's share in both columns alike; the
difference of the two columns is the row stage (beam_rows_kernel) with the n-gram LM against the one without.
usage: python tools/bench_lm_beam.py [B] [T] [n-grams in all]"""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from decode_bench import hkust_engine, synthetic_lm, timed as timed_on

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
N_TOTAL = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000


eng = hkust_engine(ctc=False)
t0 = time.perf_counter()
lm = synthetic_lm(N_TOTAL)
build_s = time.perf_counter() - t0
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "lm_ngrams": lm.counts, "lm_device_mb": round(lm.device_bytes / 2 ** 20, 1), "lm_build_s": round(build_s, 2),
       "decode_ms": {}}


def timed(fn, n=4):
    return timed_on(fn, n, side)


for K in (1, 4, 10, 20):
    plain, (tp, _) = timed(lambda: eng.recog_beam(xs, il, K, min_step_ratio=1.0))
    fused, (tf, _) = timed(lambda: eng.recog_beam_lm(xs, il, K, lm, 0.3, min_step_ratio=1.0))
    assert all(len(t) == steps for t in tp + tf), "a decode ended before the last step"
    res["decode_ms"][f"K{K}"] = {"beam": round(plain, 2), "beam_lm": round(fused, 2), "beam_step": round(plain / steps, 4),
                                 "beam_lm_step": round(fused / steps, 4), "lm_extra_us_per_step": round((fused - plain) / steps * 1e3, 1)}
    print(f"K = {K:2d}: beam {plain:7.2f} ms ({plain / steps:.4f} per step)  beam + LM {fused:7.2f} ms ({fused / steps:.4f} per step)  "
          f"LM extra {(fused - plain) / steps * 1e3:6.1f} us per step", flush=True)
print(json.dumps(res))
