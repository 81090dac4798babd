"""What the LSTM LM costs in the joint CTC/attention beam: the joint beam in three forms side by side in one process on the hkust geometry with a
CTC head, B = 16, T = 1000 (as tools/bench_joint_lm_beam.py), random-init weights, K = 1 / 4 / 10 / 20, N-best 1:
  joint        masr_recog_beam_ctc, no LM
  joint_lm     masr_recog_beam_ctc_lm with tools/decode_bench.py's synthetic 3-gram LM of about 10^6 n-grams
  joint_nlm    masr_recog_beam_ctc_nlm with tools/bench_nlm_beam.py's random 2 x 650 LSTM LM on 650-dim embeddings
Every decode replays its step graph Lmax = T / 4 times whatever the stop rule decides, so ms per step = ms per decode / steps includes the
encoder's share in all columns alike.  joint_nlm - joint_lm per step is the LSTM LM's added cost over the n-gram form: its L layer launches and
its output projection, and the row stage reading a row of LM logits against probing the n-gram tables; the prefix kernel, the N-best select and
the weights' launch are the same in both.  tools/bench_nlm_beam.py gives the same difference for the attention beam.
usage: python tools/bench_nlm_joint_beam.py [B] [T] [H] [L]"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd.nlm import LstmLM
from decode_bench import C_, hkust_engine, synthetic_lm, timed as timed_on

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
H = int(sys.argv[3]) if len(sys.argv) > 3 else 650
L = int(sys.argv[4]) if len(sys.argv) > 4 else 2
ATT_W, CTC_W, LM_W, BONUS = 0.7, 0.3, 0.3, 0.5


def random_lm(seed=7):
    """bench_nlm_beam.py's LM"""
    rng = np.random.RandomState(seed)
    u = lambda a, *shape: rng.uniform(-a, a, size=shape).astype(np.float32)  # noqa: E731
    return LstmLM(u(1.0, C_, H), [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H) for _ in range(L)],
                  [u(0.1, 4 * H) for _ in range(L)], u(0.1, C_, H), u(0.1, C_))


eng = hkust_engine(ctc=True)
ngram = synthetic_lm(1_000_000)
nlm = random_lm()
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "nlm": f"{L} x {H}", "lm_ngrams": ngram.counts, "weights": [ATT_W, CTC_W, LM_W, BONUS], "decode_ms": {}}


def timed(fn, n=3):
    return timed_on(fn, n, side)[0]


for K in (1, 4, 10, 20):
    joint = timed(lambda: eng.recog_beam(xs, il, K, att_weight=ATT_W, ctc_weight=CTC_W))
    with_ngram = timed(lambda: eng.recog_beam_ctc_lm(xs, il, K, ngram, LM_W, BONUS, 1, att_weight=ATT_W, ctc_weight=CTC_W))
    with_nlm = timed(lambda: eng.recog_beam_ctc_nlm(xs, il, K, nlm, LM_W, BONUS, 1, att_weight=ATT_W, ctc_weight=CTC_W))
    extra = (with_nlm - with_ngram) / steps * 1e3
    res["decode_ms"][f"K{K}"] = {"joint": round(joint, 2), "joint_lm": round(with_ngram, 2), "joint_nlm": round(with_nlm, 2),
                                 "joint_step": round(joint / steps, 4), "joint_lm_step": round(with_ngram / steps, 4),
                                 "joint_nlm_step": round(with_nlm / steps, 4), "nlm_extra_us_per_step_over_ngram": round(extra, 1),
                                 "nlm_extra_us_per_step_over_joint": round((with_nlm - joint) / steps * 1e3, 1)}
    print(f"K = {K:2d}: joint {joint:8.2f} ms ({joint / steps:.4f} per step)  + n-gram {with_ngram:8.2f} ms ({with_ngram / steps:.4f})  "
          f"+ LSTM LM {with_nlm:8.2f} ms ({with_nlm / steps:.4f})  LSTM over n-gram {extra:+6.1f} us per step", flush=True)
print(json.dumps(res))
