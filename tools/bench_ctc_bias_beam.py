"""What contextual phrase biasing costs in the CTC prefix beam: the model-free prefix beam in four configurations side by side
in one process -- plain (masr_ctc_beam_search), with the n-gram LM (masr_ctc_beam_search_lm), and with 1 000 random phrases of 2 - 6 units
without and with that LM (masr_ctc_beam_search_bias) -- on random logits of DESIGN 5.3's two shapes (B 8 x T' 100 and B 16 x T' 250, C 367),
K = 1 / 4 / 10 / 20, with the synthetic 3-gram LM of tools/bench_ctc_lm_beam.py.  The kernel's extra work -- at most two table probes per
(entry, class) pair that is still a candidate, and per kept extension -- does not depend on which phrases the list holds.  Reports ms per
call.  Every utterance has all T' frames; the logits are randn * scale (1: flat, the most extensions; 12: peaked).
--no-bias runs the plain and LM rows alone, through entry points that exist without this feature: the rows to compare a build against.
usage: python tools/bench_ctc_bias_beam.py [--no-bias] [--repeats N] [n-grams in all]"""
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd._cabi import lib
from decode_bench import C_, synthetic_lm, timed as timed_on

KS = (1, 4, 10, 20)
SHAPES = ((8, 100), (16, 250))
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


def main():
    args = sys.argv[1:]
    no_bias = "--no-bias" in args
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 1
    rest = [a for i, a in enumerate(args) if a not in ("--no-bias", "--repeats") and (i == 0 or args[i - 1] != "--repeats")]
    n_total = int(rest[0]) if rest else 1_000_000
    torch.manual_seed(531)
    l = lib()
    lm = synthetic_lm(n_total)
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    res = {"lm_ngrams": lm.counts, "rows": []}
    bias = None
    if not no_bias:
        from masr_amd.bias import ContextBias
        bias = ContextBias(C_, random_phrases(N_PHRASES))
        res.update(phrases=bias.phrases, trie_nodes=bias.nodes, bias_device_kb=round(bias.bytes / 1024, 1))
    for rep in range(repeats):
        for B, Tp in SHAPES:
            for scale in (1.0, 12.0):
                z = torch.randn(B, Tp, C_, device="cuda") * scale
                lens = torch.full((B,), Tp, dtype=torch.int32, device="cuda")
                for K in KS:
                    nb = int(l.masr_ctc_beam_lm_work_bytes(B, Tp, C_, K))
                    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
                    tok = torch.empty(B, 1, Tp, dtype=torch.int32, device="cuda")
                    ln, nbias = torch.empty(B, 1, dtype=torch.int32, device="cuda"), torch.empty(B, 1, dtype=torch.int32, device="cuda")
                    sc, am = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
                    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                    def plain():
                        assert l.masr_ctc_beam_search(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, p(work), nb, p(tok), p(ln), p(sc), st) == 0

                    def fused():
                        assert l.masr_ctc_beam_search_lm(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, lm.h, 0.3, 0.0, p(work), nb, p(tok), p(ln),
                                                         p(sc), p(am), st) == 0

                    def biased(with_lm):
                        def run():
                            assert l.masr_ctc_beam_search_bias(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, lm.h if with_lm else None, 0.3, 0.0,
                                                               bias.h, 3.0, p(work), nb, p(tok), p(ln), p(sc), p(am), p(nbias), st) == 0
                        return run

                    row = {"rep": rep, "B": B, "Tp": Tp, "scale": scale, "K": K, "ctc_beam_ms": round(timed_on(plain, 10)[0], 3),
                           "ctc_beam_lm_ms": round(timed_on(fused, 10)[0], 3)}
                    if bias is not None:
                        row["bias_ms"] = round(timed_on(biased(False), 10)[0], 3)
                        row["bias_lm_ms"] = round(timed_on(biased(True), 10)[0], 3)
                    res["rows"].append(row)
                    print(" ".join(f"{k} {v}" for k, v in row.items()), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
