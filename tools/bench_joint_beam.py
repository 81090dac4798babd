"""Joint CTC/attention beam (masr_recog_beam_ctc) beside the attention-only beam (masr_recog_beam) on the hkust model with a CTC head
(asr_model.ctc_weight > 0), B = 16, T = 1000.  Every decode replays its step graph Lmax = T/4 times (a random-init model hardly ever
ends a hypothesis), so ms per step = decode time / Lmax.  For the per-launch time of the prefix kernel run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_joint_beam.py` and read beam_ctc_prefix_kernel in the stats.
usage: python tools/bench_joint_beam.py [B] [T]"""
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from decode_bench import hkust_engine, timed

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
eng = hkust_engine(ctc=True)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
L = T // 4
res = {"B": B, "T": T, "steps": L, "decode": {}}

for K in (1, 4, 10, 20):
    for cw in (0.0, 0.5):
        ms, (toks, _) = timed(lambda: eng.recog_beam(xs, il, K, att_weight=1.0 - cw, ctc_weight=cw), 2, side)
        tag = f"K{K}_ctc{cw}"
        res["decode"][tag] = {"ms": round(ms, 2), "ms_per_step": round(ms / L, 3), "mean_len": sum(map(len, toks)) / B}
        print(f"K={K:2d} ctc_w={cw}: {ms:8.1f} ms  {ms / L:6.3f} ms/step  (mean hypothesis length {sum(map(len, toks)) / B:.1f})",
              flush=True)
print(json.dumps(res))
