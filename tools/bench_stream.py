#!/usr/bin/env python3
"""What the streaming first pass costs at the hkust geometry, chunk c = 16 (640 ms of audio), left in {-1, 2}:
  1. attn_stream_kernel (masr_test_attention_stream: the attention AND the cache append) against the composition it replaces at left = -1,
     two row copies into a cache of exactly pos + R rows + masr_test_attention (Tq = R, Tk = pos + R), at pos in {0, 240, 984}, R = 16,
     8 heads of 64, B = 1 and 16.  Device events around WINDOW back-to-back calls, the legs alternating, REPS windows behind a warm-up round;
  2. the chunk step: a T = 1000 stream fed in pieces of 4 c frames, B = 1 and 16 -- GPU ms per chunk step (device events around the whole
     stream / its 16 chunks), the host's enqueue time for the same calls, the real-time factor at 640 ms per chunk, the step's launches;
  3. the whole stream + the final K = 1 beam against masr_recog_ctc_beam (K = 1) = one full chunk-masked encoder pass + head + the same sweep;
  4. the resumable prefix beam, left = -1: the chunk step with the beam open at K in {1, 4, 10, 20} beside the step without it
     (the legs alternating), and on the logits the stream left behind the sum of the resumed calls over the utterance (masr_ctc_beam_run_*:
     one advance per 16 frames, then the result) beside the one-shot masr_ctc_beam_search.
python tools/bench_stream.py      prints one JSON line at the end (run it in three processes and take the medians)"""
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch
import masr_amd  # noqa: F401
from masr_amd._cabi import check, lib
from masr_amd.engine import MasrEngine
from masr_amd.model import reference_init_state_dict

HK = dict(idim=83, nheads=8, d_model=512, d_inner=2048, dropout=0.1, pos_dropout=0.1, tgt_share_weight=1, encoder=dict(nlayers=2),
          decoder=dict(nlayers=4), ctc_weight=0.3, meta={"optimizer_opt": {"k": 1.0, "warmup_steps": 25000}})
H, HD, R, T, D, CH = 8, 64, 16, 1000, 83, 16
WINDOW, REPS = 200, 5
assert torch.cuda.is_available(), "needs the MI355X"
L = lib()
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / n


# ---- 1. the attention kernel against append + the forward kernel
attn = {}
g = torch.Generator(device="cuda").manual_seed(0)
for B in (1, 16):
    for pos in (0, 240, 984):
        Tk = pos + R
        q, kn, vn = (torch.randn(B, R, H, HD, device="cuda", generator=g).bfloat16() for _ in range(3))
        kc, vc = (torch.randn(B, Tk, H, HD, device="cuda", generator=g).bfloat16() for _ in range(2))
        o = torch.zeros_like(q); lse = torch.zeros(B, H, R, device="cuda")
        klens = torch.full((B,), Tk, dtype=torch.int32, device="cuda")

        def new():
            check(L.masr_test_attention_stream(vp(q), vp(kn), vp(vn), vp(kc), vp(vc), vp(o), vp(klens), B, H, HD, R, pos, 0, Tk, stream()))

        def old():
            kc[:, pos:].copy_(kn); vc[:, pos:].copy_(vn)
            check(L.masr_test_attention(vp(q), vp(kc), vp(vc), None, vp(o), None, None, None, vp(lse), None, vp(klens), B, H, R, Tk, HD, 0, stream()))

        us = {"stream_kernel": [], "append_plus_fwd": []}
        for rep in range(REPS + 1):                              # (the first round warms up and is dropped)
            for name, fn in (("stream_kernel", new), ("append_plus_fwd", old)):
                t = timed(fn, WINDOW) * 1e3
                if rep:
                    us[name].append(t)
        attn[f"B{B}_pos{pos}"] = {n: statistics.median(x) for n, x in us.items()}
        print(f"attention, B {B:2d} pos {pos:3d}: " + ", ".join(f"{n} {statistics.median(x):6.2f} us" for n, x in us.items()))

# ---- 2. + 3. the chunk step and the whole stream
torch.manual_seed(531)
sd = reference_init_state_dict(HK, 367)
res = {"attention_us": attn, "step": {}}
NE = HK["encoder"]["nlayers"]
res["launches_per_step"] = 1 + 4 + 1 + 1 + 7 * NE + 1 + 1 + 1 + 1      # window, convs, vgg2enc, centre + PE, the layers, final LN, head, greedy, the row copy
for B in (1, 16):
    gc = torch.Generator().manual_seed(B)
    lens = torch.randint(600, T + 1, (B,), generator=gc)
    lens[0] = T
    xs = torch.zeros(B, T, D)
    for b in range(B):
        xs[b, :int(lens[b])] = torch.randn(int(lens[b]), D, generator=gc)
    xs = xs.cuda()
    for left in (-1, 2):
        eng = MasrEngine(dict(HK, chunk=dict(size=CH, left=left)), 367)
        eng.load_state_dict(sd)
        pieces = [(xs[:, t0:t0 + 4 * CH].contiguous(), [max(0, min(int(l), t0 + 4 * CH) - t0) for l in lens.tolist()], t0 + 4 * CH >= T)
                  for t0 in range(0, T, 4 * CH)]

        def run_stream(beam):
            eng.stream_begin(B, T)
            for x, v, last in pieces:
                eng.stream_feed(x, v, last)
            if beam:
                eng.stream_ctc_beam(1, raw=True)

        gpu, host, with_beam, full = [], [], [], []
        for rep in range(4):                                     # (the first round warms up and is dropped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run_stream(False); b.record()
            t1 = time.perf_counter()
            b.synchronize()
            wb = timed(lambda: run_stream(True), 1)
            fp = timed(lambda: eng.recog_ctc_beam(xs, lens, 1, raw=True), 1)
            if rep:
                gpu.append(a.elapsed_time(b)); host.append((t1 - t0) * 1e3); with_beam.append(wb); full.append(fp)
        chunks = (T // 4 + CH - 1) // CH
        r = {"gpu_ms_per_chunk": statistics.median(gpu) / chunks, "host_enqueue_ms_per_chunk": statistics.median(host) / chunks,
             "rtf": statistics.median(gpu) / chunks / 640.0, "stream_plus_beam_ms": statistics.median(with_beam), "full_pass_plus_beam_ms": statistics.median(full)}
        res["step"][f"B{B}_left{left}"] = r
        print(f"B {B:2d} left {left:2d}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()))

# ---- 4. the resumable beam inside the stream and alone
KS = (1, 4, 10, 20)
res["beam"] = {}
for B in (1, 16):
    gc = torch.Generator().manual_seed(B)
    lens = torch.randint(600, T + 1, (B,), generator=gc)
    lens[0] = T
    xs = torch.zeros(B, T, D)
    for b in range(B):
        xs[b, :int(lens[b])] = torch.randn(int(lens[b]), D, generator=gc)
    xs = xs.cuda()
    eng = MasrEngine(dict(HK, chunk=dict(size=CH, left=-1)), 367)
    eng.load_state_dict(sd)
    pieces = [(xs[:, t0:t0 + 4 * CH].contiguous(), [max(0, min(int(l), t0 + 4 * CH) - t0) for l in lens.tolist()], t0 + 4 * CH >= T)
              for t0 in range(0, T, 4 * CH)]
    chunks = (T // 4 + CH - 1) // CH

    def run_stream(K):
        eng.stream_begin(B, T)
        if K:
            eng.stream_beam_open(K)
        for x, v, last in pieces:
            eng.stream_feed(x, v, last)

    step = {K: [] for K in (0,) + KS}
    for rep_ in range(4):                                        # (the first round warms up and is dropped)
        for K in step:
            t = timed(lambda: run_stream(K), 1) / chunks
            if rep_:
                step[K].append(t)
    # the search alone, on the logits of the last stream
    z, klen, _ = eng.stream_logits()
    z, klen = z.clone(), klen.clone()
    cap, ld = z.shape[1], z.shape[2]
    alone = {}
    for K in KS:
        nb = int(L.masr_ctc_beam_run_work_bytes(B, cap, 367, K))
        work = torch.empty(nb, dtype=torch.uint8, device="cuda")
        tok = torch.empty(B, 1, cap, dtype=torch.int32, device="cuda")
        ln, sc = torch.empty(B, 1, dtype=torch.int32, device="cuda"), torch.empty(B, 1, device="cuda")

        def one_shot():
            check(L.masr_ctc_beam_search(vp(z), ld, vp(klen), B, cap, 367, K, 1, 0, 366, vp(work), nb, vp(tok), vp(ln), vp(sc), stream()))

        def resumed():
            run = L.masr_ctc_beam_run_open(vp(z), ld, vp(klen), B, cap, 367, K, 0, 366, None, 0.0, 0.0, None, 0.0, vp(work), nb, stream())
            assert run, L.masr_last_error()
            for t in list(range(CH, cap, CH)) + [cap]:
                check(L.masr_ctc_beam_run_advance(run, t, stream()))
            check(L.masr_ctc_beam_run_result(run, 1, vp(tok), vp(ln), vp(sc), None, None, stream()))
            L.masr_ctc_beam_run_close(run)                       # (host memory only: the launches hold their own arguments)

        ms = {"one_shot": [], "resumed": []}
        for rep_ in range(REPS + 1):
            for name, fn in (("one_shot", one_shot), ("resumed", resumed)):
                t = timed(fn, 1)
                if rep_:
                    ms[name].append(t)
        alone[K] = {n: statistics.median(x) for n, x in ms.items()}
    r = {"gpu_ms_per_chunk": {f"K{K}" if K else "no_beam": statistics.median(x) for K, x in step.items()},
         "search_ms": {f"K{K}": v for K, v in alone.items()}}
    res["beam"][f"B{B}"] = r
    print(f"B {B:2d} chunk step, GPU ms: " + ", ".join(f"{k} {v:.4f}" for k, v in r["gpu_ms_per_chunk"].items()))
    print(f"B {B:2d} search over {cap} frames, ms: " + ", ".join(f"{k} one-shot {v['one_shot']:.3f} resumed {v['resumed']:.3f}" for k, v in r["search_ms"].items()))
print(json.dumps(res))
