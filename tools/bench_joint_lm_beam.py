"""What the n-gram LM, the length bonus and the N-best list cost over the joint CTC/attention beam: masr_recog_beam_ctc and
masr_recog_beam_ctc_lm side by side in one process on the hkust geometry with a CTC head, B = 16, T = 1000 (as tools/bench_joint_beam.py),
random-init weights, K = 1 / 4 / 10 / 20, N = 1 and N = K, with tools/bench_lm_beam.py's synthetic 3-gram LM of about 10^6 n-grams.  Every
decode replays its step graph Lmax = T / 4 times whatever the stop rule decides, so ms per step = ms per decode / steps includes the
encoder's share in all columns alike; the difference of two columns is the fused pre-beam, the LM prefix kernel and the N-best select
against the joint beam's three step kernels.  For per-launch times run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_joint_lm_beam.py` and read beam_rows_kernel, beam_ctc_prefix_kernel and
beam_select_nbest_kernel in the stats.
usage: python tools/bench_joint_lm_beam.py [B] [T] [n-grams in all]"""
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from decode_bench import hkust_engine, synthetic_lm, timed as timed_on

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
N_TOTAL = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
ATT_W, CTC_W, LM_W, BONUS = 0.7, 0.3, 0.3, 0.5


eng = hkust_engine(ctc=True)
lm = synthetic_lm(N_TOTAL)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "lm_ngrams": lm.counts, "weights": [ATT_W, CTC_W, LM_W, BONUS], "decode_ms": {}}


def timed(fn, n=3):
    return timed_on(fn, n, side)


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
