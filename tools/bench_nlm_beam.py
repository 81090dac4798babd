"""What LSTM LM shallow fusion costs over the plain attention beam: masr_recog_beam and masr_recog_beam_nlm side by side in one process on the
hkust geometry, B = 16, T = 1000 (as tools/bench_beam.py), random-init weights, K = 1 / 4 / 10 / 20, with a random 2 x 650 LSTM LM on
650-dim embeddings over the 367 classes (the kernels' work does not depend on the values).  Both decodes replay all T / 4 steps (random
weights never end a hypothesis early at lm_w = 0.3 with min_step_ratio = 1), so ms per step = ms per decode / steps includes the encoder's
share in both columns alike; the difference of the two columns is the LM's L layer launches, its output projection and the row stage (beam_rows_kernel)
with the LM logits against the one without.
usage: python tools/bench_nlm_beam.py [B] [T] [H] [L]"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd.nlm import LstmLM
from decode_bench import C_, hkust_engine, timed as timed_on

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
H = int(sys.argv[3]) if len(sys.argv) > 3 else 650
L = int(sys.argv[4]) if len(sys.argv) > 4 else 2


def random_lm(seed=7):
    rng = np.random.RandomState(seed)
    u = lambda a, *shape: rng.uniform(-a, a, size=shape).astype(np.float32)  # noqa: E731
    return LstmLM(u(1.0, C_, H), [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H) for _ in range(L)],
                  [u(0.1, 4 * H) for _ in range(L)], u(0.1, C_, H), u(0.1, C_))


eng = hkust_engine(ctc=False)
lm = random_lm()
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "lm": f"{L} x {H}", "lm_device_mb": round(lm.device_bytes / 2 ** 20, 1), "decode_ms": {}}


def timed(fn, n=4):
    return timed_on(fn, n, side)


for K in (1, 4, 10, 20):
    plain, (tp, _) = timed(lambda: eng.recog_beam(xs, il, K, min_step_ratio=1.0))
    fused, (tf, _) = timed(lambda: eng.recog_beam_nlm(xs, il, K, lm, 0.3, min_step_ratio=1.0))
    assert all(len(t) == steps for t in tp + tf), "a decode ended before the last step"
    res["decode_ms"][f"K{K}"] = {"beam": round(plain, 2), "beam_nlm": round(fused, 2), "beam_step": round(plain / steps, 4),
                                 "beam_nlm_step": round(fused / steps, 4), "lm_extra_us_per_step": round((fused - plain) / steps * 1e3, 1)}
    print(f"K = {K:2d}: beam {plain:7.2f} ms ({plain / steps:.4f} per step)  beam + LSTM LM {fused:7.2f} ms ({fused / steps:.4f} per step)  "
          f"LM extra {(fused - plain) / steps * 1e3:6.1f} us per step", flush=True)
print(json.dumps(res))
