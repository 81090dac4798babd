"""Beam search (masr_recog_beam) beside the greedy decode (masr_recog) on the hkust model, and the decode's few-row GEMM against the
NT GEMM at B*K rows.  Both decodes run their whole Lmax = T/4 steps here (a random-init model hardly ever ends a hypothesis), so
ms per step = decode time / Lmax.  usage: python tools/bench_beam.py [B] [T]"""
import ctypes as C
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd import _cabi
from decode_bench import hkust_engine, timed

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
eng = hkust_engine(ctc=False)
xs = torch.randn(B, T, 80, device="cuda")
il = torch.full((B,), T, dtype=torch.int64)
side = torch.cuda.Stream()
L = T // 4
res = {"B": B, "T": T, "steps": L, "decode": {}, "gemm_us": []}

ms, _ = timed(lambda: eng.recog(xs, il), 3, side)
res["decode"]["greedy"] = {"ms": round(ms, 2), "ms_per_step": round(ms / L, 3), "utt_per_s": round(B / ms * 1e3, 1)}
print(f"greedy        : {ms:8.1f} ms  {ms / L:6.3f} ms/step  {B / ms * 1e3:7.1f} utt/s", flush=True)
for K in (1, 4, 10, 20):
    ms, (toks, sc) = timed(lambda: eng.recog_beam(xs, il, K), 2, side)
    steps = L   # the graph is replayed Lmax times whatever ends earlier
    res["decode"][f"beam{K}"] = {"ms": round(ms, 2), "ms_per_step": round(ms / steps, 3), "utt_per_s": round(B / ms * 1e3, 1),
                                 "mean_len": sum(map(len, toks)) / B}
    print(f"beam K={K:2d}     : {ms:8.1f} ms  {ms / steps:6.3f} ms/step  {B / ms * 1e3:7.1f} utt/s  (mean hypothesis length "
          f"{sum(map(len, toks)) / B:.1f})", flush=True)

# decoder Linears at B*K rows: skinny (what the decode launches) vs the NT GEMM of gemm.hip, same epilogues
lib = _cabi.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
E, F = 512, 2048
for M in (16, 64, 160, 320):
    for (N, K, relu, resid, out16) in ((3 * E, E, 0, False, True), (E, E, 0, True, False), (F, E, 1, False, True), (E, F, 0, True, False)):
        a = torch.randn(M, K, device="cuda").bfloat16(); w = torch.randn(N, K, device="cuda").bfloat16()
        bias = torch.randn(N, device="cuda"); r = torch.randn(M, N, device="cuda") if resid else None
        c32 = None if out16 else torch.empty(M, N, device="cuda"); c16 = torch.empty(M, N, device="cuda").bfloat16() if out16 else None
        st = C.c_void_p(side.cuda_stream)
        sk = lambda: _cabi.check(lib.masr_test_skinny_gemm(P(a), K, P(w), K, M, N, K, P(bias), relu, P(r), P(c32), P(c16), st))
        nt = lambda: _cabi.check(lib.masr_test_gemm_epi(P(a), K, P(w), K, M, N, K, P(bias), relu, C.c_float(0.0), P(r), None, P(c32), P(c16), st))
        us = {}
        for tag, fn in (("skinny", sk), ("nt", nt)):
            with torch.cuda.stream(side):
                for _ in range(20): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200): fn()
                e1.record()
            torch.cuda.synchronize()
            us[tag] = e0.elapsed_time(e1) / 200 * 1e3
        o1 = (c32 if c32 is not None else c16.float()).clone()
        res["gemm_us"].append({"M": M, "N": N, "K": K, "skinny": round(us["skinny"], 2), "nt": round(us["nt"], 2)})
        print(f"GEMM M={M:4d} N={N:5d} K={K:5d}{' relu' if relu else ''}{' +res' if resid else ''}: skinny {us['skinny']:7.2f} us, "
              f"NT {us['nt']:7.2f} us", flush=True)
print(json.dumps(res))
