"""CTC forced alignment (masr_ctc_align): what the operator and the model calls cost.
  1. the operator alone on random logits at the hkust hybrid shape (B 16, T' 250, C 367, transcripts of 25 .. 37 tokens, S ~ 63) and at a
     wide lattice (L 150, S 301, back-pointers in the work buffer): us per call (ctc_align_frames + ctc_align_sweep) from device events
     around WINDOW back-to-back calls, beside masr_ctc_loss on the same logits and targets (ctc_lse + both sweeps + ctc_grad + the mean: the
     training lattice, the yardstick of DESIGN 5.1) and beside the alignment whose sweep ends behind the score (include/masr_test.h
     masr_test_ctc_align_no_trace: the difference is the back-trace and the start / end pass), the legs alternating, REPS windows each;
  2. the model calls, ms per call with the copy of the results to the host: MasrEngine.ctc_align on the hkust geometry (B 16, T 1000) beside
     recog_ctc_beam at K = 1 (the same encoder pass and head GEMM), and BlstmEngine.ctc_align at B 8 x 400 frames beside the forward alone.
For the two kernels' own times run `rocprofv3 --kernel-trace --stats -- python tools/bench_ctc_align.py` and read them in the stats.
usage: python tools/bench_ctc_align.py      prints one JSON line at the end"""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd._cabi import align_outputs, align_targets, check, lib
from masr_amd.blstm_engine import BlstmEngine
from masr_amd.blstm_engine import reference_init_state_dict as blstm_init
from decode_bench import hkust_engine, timed

WINDOW, REPS = 200, 5
DEV = "cuda"
p = lambda t: C.c_void_p(t.data_ptr())                          # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731


def operator_legs(B, Tp, Cn, lo, hi, g):
    """the alignment and the training lattice on the same random logits and targets -> {leg: us per call, best of REPS windows}"""
    l = lib()
    z = torch.randn(B, Tp, Cn, generator=g).to(DEV)
    zt = z.transpose(0, 1).contiguous()                         # masr_ctc_loss reads [T][B][C]
    ol = torch.randint(lo, hi + 1, (B,), generator=g).tolist()
    ys = [torch.randint(1, Cn - 1, (n,), generator=g).tolist() for n in ol]
    tgt, off, tl, maxL = align_targets(ys, ol, DEV)
    lens = torch.full((B,), Tp, dtype=torch.int32, device=DEV)
    nb = int(l.masr_ctc_align_work_bytes(B, Tp, maxL))
    work = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out, ptrs = align_outputs(B, Tp, maxL, DEV)
    maxS = 2 * maxL + 1
    lwork = torch.zeros(int(l.masr_ctc_work_floats(Tp, B, maxS)), device=DEV)
    nll, loss, grad = torch.zeros(B, device=DEV), torch.zeros(1, device=DEV), torch.zeros_like(zt)
    legs = {
        "ctc_align": lambda: l.masr_ctc_align(p(z), Cn, p(lens), p(tgt), p(off), p(tl), B, Tp, Cn, 0, maxL, p(work), nb, *ptrs, stream()),
        "ctc_align_no_trace": lambda: l.masr_test_ctc_align_no_trace(p(z), Cn, p(lens), p(tgt), p(off), p(tl), B, Tp, Cn, 0, maxL, p(work), nb, *ptrs,
                                                                     stream()),
        "ctc_loss": lambda: l.masr_ctc_loss(p(zt), p(tgt), p(off), p(lens), p(tl), Tp, B, Cn, 0, p(nll), p(loss), p(grad), p(lwork), maxS, stream()),
    }
    us = {k: [] for k in legs}
    for rep in range(REPS + 1):                                 # (the first round warms up and is dropped)
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(WINDOW):
                check(fn(), name)
            b.record(); b.synchronize()
            if rep:
                us[name].append(a.elapsed_time(b) * 1e3 / WINDOW)
    assert torch.isfinite(out[3]).all()
    return {f"{k}_us": round(min(v), 2) for k, v in us.items()} | {f"{k}_us_median": round(statistics.median(v), 2) for k, v in us.items()} | \
        {"B": B, "Tp": Tp, "C": Cn, "maxL": maxL, "work_bytes": nb}


def main():
    g = torch.Generator().manual_seed(531)
    torch.manual_seed(531)
    res = {"operator_hkust": operator_legs(16, 250, 367, 25, 37, g), "operator_wide": operator_legs(16, 330, 367, 150, 150, g)}
    print(json.dumps(res), flush=True)
    ms = lambda fn, n=5: round(timed(fn, n)[0], 3)              # noqa: E731
    cfg = {"encoder": {"idim": 83, "enc_dim": 360, "proj_dim": 360, "odim": 360, "sample_rate": "1_1_1", "dropout": "0_0_0"}}
    eng = BlstmEngine(cfg, 367)
    eng.load_state_dict(blstm_init(cfg, 367))
    B, T = 8, 400
    xs = torch.randn(B, T, 83, device=DEV)
    il = torch.full((B,), T, dtype=torch.int64)
    ol = torch.randint(10, 26, (B,), generator=g).tolist()
    ys = [torch.randint(1, 366, (n,), generator=g).tolist() for n in ol]
    res["blstm"] = {"B": B, "T": T, "forward_ms": ms(lambda: eng.forward(xs, il)), "ctc_align_ms": ms(lambda: eng.ctc_align(xs, il, ys, ol)),
                    "per_utterance_ms": ms(lambda: [eng.ctc_align(xs[b:b + 1], il[b:b + 1], [ys[b]], [ol[b]]) for b in range(B)])}
    del eng
    eng = hkust_engine(ctc=True, seed=None)
    B, T = 16, 1000
    xs = torch.randn(B, T, 80, device=DEV)
    il = torch.full((B,), T, dtype=torch.int64)
    ol = torch.randint(25, 38, (B,), generator=g).tolist()
    ys = [torch.randint(1, 366, (n,), generator=g).tolist() for n in ol]
    res["hybrid"] = {"B": B, "T": T, "ctc_align_ms": ms(lambda: eng.ctc_align(xs, il, ys, ol)), "ctc_beam_K1_ms": ms(lambda: eng.recog_ctc_beam(xs, il, 1))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
