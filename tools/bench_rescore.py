"""The four decoders of a hybrid model side by side on the hkust model with a CTC head, B = 16, T = 1000 (as tools/bench_beam.py): ms per decode of
the CTC prefix beam (masr_recog_ctc_beam), attention rescoring of its N-best (masr_recog_rescore, N = K: one teacher-forced decoder pass over
B * N hypotheses), the attention beam (masr_recog_beam) and the joint CTC/attention beam (masr_recog_beam_ctc) at K = N = 4 / 10 / 20.  The
results stay on the device in all four; the
rescoring time includes its one host synchronisation between the passes; `L` is the number of decoder positions its second pass ran.
usage: python tools/bench_rescore.py [B] [T]"""
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from decode_bench import hkust_engine, timed as timed_on

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
eng = hkust_engine(ctc=True)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
res = {"B": B, "T": T, "decode_ms": {}}


def timed(fn, n=40):
    return timed_on(fn, n, side)[0]


for K in (4, 10, 20):
    row = {
        "ctc_beam": timed(lambda: eng.recog_ctc_beam(xs, il, K, K, raw=True)),
        "rescore": timed(lambda: eng.recog_rescore(xs, il, K, K, 0.5, 0.5, raw=True)),
        "beam": timed(lambda: eng.recog_beam(xs, il, K), 4),
        "joint_beam": timed(lambda: eng.recog_beam(xs, il, K, att_weight=0.5, ctc_weight=0.5), 4),
    }
    with torch.cuda.stream(side):
        eng.recog_rescore(xs, il, K, K, 0.5, 0.5, raw=True)
        row["L"] = int(eng.last_rescore_logits()[1].shape[1])
    torch.cuda.synchronize()
    res["decode_ms"][f"K{K}"] = {k: round(v, 2) for k, v in row.items()}
    print(f"K = N = {K:2d}: ctc_beam {row['ctc_beam']:7.2f}  rescore {row['rescore']:7.2f} (L = {row['L']})  beam {row['beam']:7.2f}  "
          f"joint beam {row['joint_beam']:7.2f}  ms per decode", flush=True)
print(json.dumps(res))
