"""What contextual phrase biasing costs in the attention beam and the joint beam: on the hkust geometry with a CTC head
(tools/decode_bench.py), B = 16, T = 1000, random-init weights, K = 1 / 4 / 10 / 20, the synthetic 3-gram LM of about 10^6 n-grams and 1 000
random phrases of 2 - 6 units.  First the searches that exist without this feature -- `beam`, `lm_beam`, `lm_joint_beam` -- then
`bias_beam` and `bias_joint_beam`, each without and with the LM.  Every decode replays its step graph Lmax = T / 4 times whatever the stop
rule decides (a finished utterance's rows idle through the rest), so the looser stop bound of the biased searches adds no launches: ms per
decode is Lmax steps in every column, and the difference of two columns is the row stage's table probes (and, joint, the sixth add and the
state's two loads and one store per row).  `mean_len` is the mean length of the returned hypotheses.
--no-bias runs the three existing searches alone, through entry points that exist without this feature: the rows to compare a build
against (run the two builds alternately, one process each, and take the median of three processes per build).
usage: python tools/bench_bias_beam.py [--no-bias] [B] [T] [n-grams in all]"""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from decode_bench import C_, hkust_engine, synthetic_lm, timed as timed_on

args = [a for a in sys.argv[1:] if a != "--no-bias"]
NO_BIAS = "--no-bias" in sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 16
T = int(args[1]) if len(args) > 1 else 1000
N_TOTAL = int(args[2]) if len(args) > 2 else 1_000_000
ATT_W, CTC_W, LM_W, BONUS, BIAS_W = 0.7, 0.3, 0.3, 0.5, 3.0
N_PHRASES = 1000


def random_phrases(n, seed=11):
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    while len(out) < n:
        ph = tuple(int(t) for t in rng.randint(1, C_ - 1, size=rng.randint(2, 7)))
        if ph not in seen:
            seen.add(ph)
            out.append(list(ph))
    return out


eng = hkust_engine(ctc=True)
lm = synthetic_lm(N_TOTAL)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
steps = T // 4
res = {"B": B, "T": T, "steps": steps, "lm_ngrams": lm.counts, "weights": [ATT_W, CTC_W, LM_W, BONUS, BIAS_W], "decode_ms": {}}
bias = None
if not NO_BIAS:
    from masr_amd.bias import ContextBias
    bias = ContextBias(C_, random_phrases(N_PHRASES))
    res.update(phrases=bias.phrases, trie_nodes=bias.nodes, bias_device_kb=round(bias.bytes / 1024, 1))


def timed(fn, n=3):
    return timed_on(fn, n, side)


def mean_len(toks):
    return round(sum(len(t) for t in toks) / len(toks), 1)


for K in (1, 4, 10, 20):
    modes = {
        "beam": lambda: eng.recog_beam(xs, il, K)[0],
        "lm_beam": lambda: eng.recog_beam_lm(xs, il, K, lm, LM_W)[0],
        "lm_joint_beam": lambda: [u[0][0] if u else [] for u in eng.recog_beam_ctc_lm(xs, il, K, lm, LM_W, BONUS, 1, att_weight=ATT_W, ctc_weight=CTC_W)],
    }
    if bias is not None:
        modes.update({
            "bias_beam": lambda: eng.recog_beam_bias(xs, il, K, bias, BIAS_W)[0],
            "bias_beam_lm": lambda: eng.recog_beam_bias(xs, il, K, bias, BIAS_W, lm, LM_W)[0],
            "bias_joint_beam": lambda: [u[0][0] if u else [] for u in eng.recog_beam_ctc_bias(xs, il, K, bias, BIAS_W, None, 0.0, BONUS, 1,
                                                                                              att_weight=ATT_W, ctc_weight=CTC_W)],
            "bias_joint_beam_lm": lambda: [u[0][0] if u else [] for u in eng.recog_beam_ctc_bias(xs, il, K, bias, BIAS_W, lm, LM_W, BONUS, 1,
                                                                                                 att_weight=ATT_W, ctc_weight=CTC_W)],
        })
    row, line = {}, f"K = {K:2d}:"
    for name, fn in modes.items():
        ms, toks = timed(fn)
        row[name] = round(ms, 2)
        row[name + "_mean_len"] = mean_len(toks)
        line += f"  {name} {ms:8.2f} ms"
    res["decode_ms"][f"K{K}"] = row
    print(line, flush=True)
print(json.dumps(res))
