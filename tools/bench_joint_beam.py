"""Joint CTC/attention beam (masr_recog_beam_ctc) beside the attention-only beam (masr_recog_beam) on the hkust model with a CTC head
(asr_model.ctc_weight > 0), B = 16, T = 1000.  Every decode replays its step graph Lmax = T/4 times (a random-init model hardly ever
ends a hypothesis), so ms per step = decode time / Lmax.  For the per-launch time of the prefix kernel run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_joint_beam.py` and read beam_ctc_prefix_kernel in the stats.
usage: python tools/bench_joint_beam.py [B] [T]"""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd.engine import MasrEngine
from masr_amd.model import reference_init_state_dict

HKUST = {"idim": 80, "nheads": 8, "d_model": 512, "d_inner": 2048, "dropout": 0.1, "pos_dropout": 0.1, "tgt_share_weight": 1,
         "encoder": {"nlayers": 2}, "decoder": {"nlayers": 4}, "ctc_weight": 0.3}
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
torch.manual_seed(531)
eng = MasrEngine(HKUST, 367)
eng.load_state_dict(reference_init_state_dict(HKUST, 367))
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
L = T // 4
res = {"B": B, "T": T, "steps": L, "decode": {}}


def timed(fn, n):
    with torch.cuda.stream(side):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for _ in range(n):
            r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, r


for K in (1, 4, 10, 20):
    for cw in (0.0, 0.5):
        ms, (toks, _) = timed(lambda: eng.recog_beam(xs, il, K, att_weight=1.0 - cw, ctc_weight=cw), 2)
        tag = f"K{K}_ctc{cw}"
        res["decode"][tag] = {"ms": round(ms, 2), "ms_per_step": round(ms / L, 3), "mean_len": sum(map(len, toks)) / B}
        print(f"K={K:2d} ctc_w={cw}: {ms:8.1f} ms  {ms / L:6.3f} ms/step  (mean hypothesis length {sum(map(len, toks)) / B:.1f})",
              flush=True)
print(json.dumps(res))
