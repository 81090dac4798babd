"""What the LSTM LM costs in the CTC prefix beam: masr_ctc_beam_search, masr_ctc_beam_search_lm and masr_ctc_beam_search_nlm side
by side in one process, model-free, on random logits of DESIGN 5.3's two shapes (B 8 x T' 100 and B 16 x T' 250, C 367), K = 1 / 4 / 10 / 20,
with the synthetic 3-gram LM of tools/bench_ctc_lm_beam.py and the random 2 x 650 LSTM LM of tools/bench_nlm_beam.py (the kernels' work does
not depend on the values, except through how often a beam row takes a token: the logits are randn * scale, scale 1 a flat distribution where
every frame refills the beam with new prefixes -- every row steps the LM -- and scale 12 a peaked one where most rows stay and only copy).
The operator launches every frame's kernels directly.  Behind that table the model path on the hkust geometry with a CTC head:
masr_recog_ctc_beam against masr_recog_ctc_beam_nlm with the frame replayed as a hipGraph (a side stream) and launched directly
(MASR_RECOG_NO_GRAPH); the encoder pass is in both columns alike, the difference is the search.
usage: python tools/bench_ctc_nlm_beam.py [n-grams in all] [H] [L]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd._cabi import lib
from masr_amd.nlm import LstmLM
from decode_bench import C_, hkust_engine, synthetic_lm, timed as timed_on

KS = (1, 4, 10, 20)
SHAPES = ((8, 100), (16, 250))
N_TOTAL = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
H = int(sys.argv[2]) if len(sys.argv) > 2 else 650
L = int(sys.argv[3]) if len(sys.argv) > 3 else 2


def random_nlm(seed=7):
    rng = np.random.RandomState(seed)
    u = lambda a, *shape: rng.uniform(-a, a, size=shape).astype(np.float32)  # noqa: E731
    return LstmLM(u(1.0, C_, H), [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H, H) for _ in range(L)], [u(0.1, 4 * H) for _ in range(L)],
                  [u(0.1, 4 * H) for _ in range(L)], u(0.1, C_, H), u(0.1, C_))


def timed(fn, n=10, stream=None):
    return timed_on(fn, n, stream)[0]


def main():
    torch.manual_seed(531)
    l = lib()
    lm, nlm = synthetic_lm(N_TOTAL), random_nlm()
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    res = {"lm_ngrams": lm.counts, "nlm": f"{L} x {H}", "nlm_device_mb": round(nlm.device_bytes / 2 ** 20, 1), "rows": [], "model_rows": []}
    for B, Tp in SHAPES:
        for scale in (1.0, 12.0):
            z = torch.randn(B, Tp, C_, device="cuda") * scale
            lens = torch.full((B,), Tp, dtype=torch.int32, device="cuda")
            for K in KS:
                nb = int(l.masr_ctc_beam_nlm_work_bytes(nlm.h, B, Tp, C_, K))
                work = torch.empty(nb, dtype=torch.uint8, device="cuda")
                tok = torch.empty(B, 1, Tp, dtype=torch.int32, device="cuda")
                ln = torch.empty(B, 1, dtype=torch.int32, device="cuda")
                sc, am = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

                def plain():
                    assert l.masr_ctc_beam_search(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, p(work), nb, p(tok), p(ln), p(sc), st) == 0

                def ngram():
                    assert l.masr_ctc_beam_search_lm(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, lm.h, 0.3, 0.0, p(work), nb, p(tok), p(ln),
                                                     p(sc), p(am), st) == 0

                def neural():
                    assert l.masr_ctc_beam_search_nlm(p(z), C_, p(lens), B, Tp, C_, K, 1, 0, C_ - 1, nlm.h, 0.3, 0.0, p(work), nb, p(tok), p(ln),
                                                      p(sc), p(am), st) == 0

                tp, tf, tn = timed(plain), timed(ngram), timed(neural, 4)
                res["rows"].append({"B": B, "Tp": Tp, "scale": scale, "K": K, "ctc_beam_ms": round(tp, 3), "ctc_beam_lm_ms": round(tf, 3),
                                    "ctc_beam_nlm_ms": round(tn, 3), "nlm_us_per_frame": round(tn / Tp * 1e3, 2)})
                print(f"B {B:2d} x T' {Tp:3d} scale {scale:4.1f} K = {K:2d}: ctc_beam {tp:7.3f} ms  n-gram {tf:7.3f} ms  LSTM LM {tn:8.3f} ms  "
                      f"({tn / Tp * 1e3:6.2f} us per frame)", flush=True)
    eng = hkust_engine(ctc=True)
    side = torch.cuda.Stream()
    for B, Tp in SHAPES:
        T = 4 * Tp
        xs = torch.randn(B, T, 80, device="cuda")
        il = torch.full((B,), T, dtype=torch.int64)
        for K in KS:
            tp = timed(lambda: eng.recog_ctc_beam(xs, il, K, raw=True), 4, side)
            tg = timed(lambda: eng.recog_ctc_beam_nlm(xs, il, K, nlm, 0.3, raw=True), 4, side)
            os.environ["MASR_RECOG_NO_GRAPH"] = "1"
            td = timed(lambda: eng.recog_ctc_beam_nlm(xs, il, K, nlm, 0.3, raw=True), 4, side)
            del os.environ["MASR_RECOG_NO_GRAPH"]
            res["model_rows"].append({"B": B, "T": T, "K": K, "recog_ctc_beam_ms": round(tp, 3), "recog_ctc_beam_nlm_graph_ms": round(tg, 3),
                                      "recog_ctc_beam_nlm_direct_ms": round(td, 3)})
            print(f"model B {B:2d} x T {T:4d} K = {K:2d}: recog_ctc_beam {tp:7.3f} ms  with LSTM LM, graph {tg:8.3f} ms  direct {td:8.3f} ms", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
