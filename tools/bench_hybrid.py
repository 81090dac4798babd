"""Cost of the joint CTC/attention objective (asr_model.ctc_weight) on the hkust geometry (E 512, 2e/4d, B 16, T 1000, labels ~31):
one task's inner step (run_batch + clip + SGD) and four concurrent task slots (the FOMAML --tasks_per_gpu 4 shape), at w = 0 and w = 0.3,
for idim 80 and 83; and the head's forward / dgrad GEMM shapes timed alone.  The CTC launches' own durations come from a kernel trace:
run `--trace` under `rocprofv3 --kernel-trace --stats` (a few w = 0.3 steps) and read the ctc_* rows of its stats.
usage: python tools/bench_hybrid.py [--steps N] [--trace]"""
import argparse
import ctypes as C
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd import _cabi
from masr_amd.engine import MasrEngine
from masr_amd.model import reference_init_state_dict

HKUST = {"nheads": 8, "d_model": 512, "d_inner": 2048, "dropout": 0.1, "pos_dropout": 0.1, "tgt_share_weight": 1,
         "encoder": {"nlayers": 2}, "decoder": {"nlayers": 4}}
ODIM, B, T, L = 367, 16, 1000, 31


def batch(idim, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(B, T, idim, generator=g).cuda()
    il = torch.full((B,), T, dtype=torch.int64) - torch.randint(0, 120, (B,), generator=g)
    ol = torch.randint(L - 6, L + 6, (B,), generator=g)
    ys = [torch.randint(1, ODIM - 1, (int(n),), generator=g) for n in ol]
    return xs, il, ys, ol


def make(idim, w, slots):
    cfg = dict(HKUST, idim=idim, ctc_weight=w)
    torch.manual_seed(531)
    sd = reference_init_state_dict(cfg, ODIM)
    engs = []
    for i in range(slots):
        e = MasrEngine(cfg, ODIM, label_smoothing=0.1)
        e.load_state_dict(sd); e.set_seed(7 + i); e.set_concurrency(slots)
        engs.append(e)
    return engs


def run(engs, streams, batches, steps, warmup):
    moms = [torch.zeros_like(e.params) for e in engs]

    def step(i):
        for e, s, m in zip(engs, streams, moms):
            with torch.cuda.stream(s):
                e.run_batch(*batches[i % len(batches)], train=True)
                e.clip_sgd_step(m, 5.0, 1e-4, 0.9, True, i == 0)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return ms, len(engs) * B / ms * 1e3


def gemm_us(M, N, K, bias, side, n=200):
    lib = _cabi.lib()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    a = torch.randn(M, K, device="cuda").bfloat16(); w = torch.randn(N, K, device="cuda").bfloat16()
    b = torch.randn(N, device="cuda") if bias else None
    c = torch.empty(M, N, device="cuda")
    st = C.c_void_p(side.cuda_stream)
    fn = lambda: _cabi.check(lib.masr_test_gemm_epi(P(a), K, P(w), K, M, N, K, P(b), 0, C.c_float(0.0), None, None, P(c), None, st))
    with torch.cuda.stream(side):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="a few w = 0.3 single-task steps only (for a kernel trace)")
    a = ap.parse_args()
    if a.trace:
        engs = make(83, 0.3, 1)
        run(engs, [torch.cuda.Stream()], [batch(83, 1)], 3, 2)
        return
    res = {"B": B, "T": T, "L": L, "odim": ODIM, "single": {}, "four_slots": {}}
    for idim in (80, 83):
        bs = [batch(idim, s) for s in range(4)]
        for w in (0.0, 0.3):
            engs = make(idim, w, 1)
            ms, ups = run(engs, [torch.cuda.Stream()], bs, a.steps, a.warmup)
            res["single"][f"idim{idim}_w{w}"] = {"ms": round(ms, 3), "utt_per_s": round(ups, 1)}
            print(f"idim {idim} w {w}: one task {ms:7.3f} ms/step {ups:8.1f} utt/s", flush=True)
            del engs
            engs = make(idim, w, 4)
            ms, ups = run(engs, [torch.cuda.Stream() for _ in engs], bs, a.steps, a.warmup)
            res["four_slots"][f"idim{idim}_w{w}"] = {"ms": round(ms, 3), "utt_per_s": round(ups, 1)}
            print(f"idim {idim} w {w}: four slots {ms:7.3f} ms/meta-round {ups:8.1f} utt/s", flush=True)
            del engs
            torch.cuda.empty_cache()
    side = torch.cuda.Stream()
    rows = B * (T // 4)
    res["head_gemm_us"] = {"fwd_4000x367x512": round(gemm_us(rows, ODIM, 512, True, side), 2),
                           "dgrad_4000x512x384": round(gemm_us(rows, 512, 384, False, side), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
