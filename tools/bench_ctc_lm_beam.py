"""What the n-gram LM costs in the CTC prefix beam: masr_ctc_beam_search and masr_ctc_beam_search_lm side by side in one
process, model-free, on random logits of DESIGN 5.3's two shapes (B 8 x T' 100 and B 16 x T' 250, C 367), K = 1 / 4 / 10 / 20, with the
synthetic 3-gram LM of about 10^6 n-grams that tools/bench_lm_beam.py uses (random n-grams with random log-probabilities: the kernel's
work -- up to two table probes and the dense unigram per (entry, class) pair -- does not depend on the values).  Reports ms per call and
the difference per frame in microseconds.  Every utterance has all T' frames.  The logits are randn * scale: scale 1 is a flat
distribution (every frame refills the beam with new prefixes: the most extensions, hence the most lookups), scale 12 a peaked one.
usage: python tools/bench_ctc_lm_beam.py [n-grams in all]"""
import ctypes as C
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd._cabi import lib
from decode_bench import C_, synthetic_lm, timed as timed_on

KS = (1, 4, 10, 20)
SHAPES = ((8, 100), (16, 250))
N_TOTAL = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000


def timed(fn, n=10):
    return timed_on(fn, n)[0]


def main():
    torch.manual_seed(531)
    l = lib()
    lm = synthetic_lm(N_TOTAL)
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    res = {"lm_ngrams": lm.counts, "lm_device_mb": round(lm.device_bytes / 2 ** 20, 1), "rows": []}
    for B, Tp in SHAPES:
        for scale in (1.0, 12.0):
            z = torch.randn(B, Tp, C_, device="cuda") * scale
            lens = torch.full((B,), Tp, dtype=torch.int32, device="cuda")
            for K in KS:
                nb = int(l.masr_ctc_beam_lm_work_bytes(B, Tp, C_, K))
                work = torch.empty(nb, dtype=torch.uint8, device="cuda")
                tok = torch.empty(B, 1, Tp, dtype=torch.int32, device="cuda")
                ln = torch.empty(B, 1, dtype=torch.int32, device="cuda")
                sc, am = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def plain():
                    assert l.masr_ctc_beam_search(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, p(work), nb, p(tok), p(ln), p(sc), st) == 0

                def fused():
                    assert l.masr_ctc_beam_search_lm(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, lm.h, 0.3, 0.0, p(work), nb, p(tok), p(ln),
                                                     p(sc), p(am), st) == 0

                tp, tf = timed(plain), timed(fused)
                row = {"B": B, "Tp": Tp, "scale": scale, "K": K, "ctc_beam_ms": round(tp, 3), "ctc_beam_lm_ms": round(tf, 3),
                       "plain_us_per_frame": round(tp / Tp * 1e3, 2), "lm_extra_us_per_frame": round((tf - tp) / Tp * 1e3, 2)}
                res["rows"].append(row)
                print(f"B {B:2d} x T' {Tp:3d} scale {scale:4.1f} K = {K:2d}: ctc_beam {tp:7.3f} ms  with LM {tf:7.3f} ms  "
                      f"plain {tp / Tp * 1e3:6.2f} us per frame  LM extra {(tf - tp) / Tp * 1e3:6.2f} us per frame", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
