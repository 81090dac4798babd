#!/usr/bin/env python3
"""What the chunk mask of the encoder's self-attention costs or saves at the hkust shape:
  1. the encoder attention alone, forward + backward (masr_test_attention_chunk), 16 x 8 heads x 250 x 250, head dim 64, dropout 0.1: unmasked,
     chunk 16 with every earlier chunk visible (left -1), chunk 16 with two earlier chunks (left 2: key blocks are skipped from both ends).
     Device events around WINDOW back-to-back launches, the three settings alternating, REPS windows each behind a warm-up round;
  2. the single-task training step (run_batch + clip + SGD, k-split on as train.py runs it; B = 16, T = 1000) with the policy off,
     {size 16, left -1} and the dynamic policy {size 0, left -1, dynamic 1}, in one process, the legs alternating; device events around
     each leg's steps.
python tools/bench_chunk.py [steps per leg = 100]      prints one JSON line at the end (run it in three processes and take the medians)"""
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch
import masr_amd  # noqa: F401
from masr_amd._cabi import check, lib
from masr_amd.engine import MasrEngine
from masr_amd.model import reference_init_state_dict

HK = dict(idim=83, nheads=8, d_model=512, d_inner=2048, dropout=0.1, pos_dropout=0.1, tgt_share_weight=1, encoder=dict(nlayers=2),
          decoder=dict(nlayers=4), meta={"optimizer_opt": {"k": 1.0, "warmup_steps": 25000}})
B, H, TP, HD, T, D = 16, 8, 250, 64, 1000, 83
WINDOW, REPS = 200, 7
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
assert torch.cuda.is_available(), "needs the MI355X"
L = lib()
vp = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

# ---- 1. the attention alone
g = torch.Generator(device="cuda").manual_seed(0)
q, k, v, dout = (torch.randn(B, TP, H, HD, device="cuda", generator=g).bfloat16() for _ in range(4))
o, dq, dk, dv = (torch.zeros_like(q) for _ in range(4))
lse = torch.zeros(B, H, TP, device="cuda")
klens = torch.randint(150, TP + 1, (B,), device="cuda", generator=g).int()
klens[0] = TP
ATTN = {"unmasked": (0, -1), "chunk16_left_all": (16, -1), "chunk16_left2": (16, 2)}
us = {name: [] for name in ATTN}
for rep in range(REPS + 1):                                     # (the first round warms up and is dropped)
    for name, (c, left) in ATTN.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(WINDOW):
            check(L.masr_test_attention_chunk(vp(q), vp(k), vp(v), vp(dout), vp(o), vp(dq), vp(dk), vp(dv), vp(lse), vp(klens), B, H, TP, TP, HD, 0, 0.1,
                                              531 + i, 7, c, left, None, stream()), name)
        b.record(); b.synchronize()
        if rep:
            us[name].append(a.elapsed_time(b) * 1e3 / WINDOW)
for name, x in us.items():
    print(f"attention fwd + bwd, {name:18s} {min(x):7.2f} us best, {statistics.median(x):7.2f} us median of {REPS} x {WINDOW} launches")

# ---- 2. the training step under three policies
gc = torch.Generator().manual_seed(0)
lens = torch.randint(600, T + 1, (B,), generator=gc)
lens[0] = T
xs = torch.zeros(B, T, D)
for b in range(B):
    xs[b, :int(lens[b])] = torch.randn(int(lens[b]), D, generator=gc)
xs = xs.cuda()
torch.manual_seed(531)
sd = reference_init_state_dict(HK, 367)
ol = torch.randint(10, 41, (B,), generator=gc)
ys = [torch.randint(1, 366, (int(n),), generator=gc) for n in ol]
eng = MasrEngine(HK, 367, label_smoothing=0.2)
eng.load_state_dict(sd)
eng.set_ksplit(True)
mom = torch.zeros_like(eng.params)
lr = 512 ** -0.5 * 25000 ** -0.5
POLICIES = {"off": None, "size16": dict(size=16, left=-1, dynamic=0), "dynamic": dict(size=0, left=-1, dynamic=1)}


def run(n):
    drawn = []
    for _ in range(n):
        eng.run_batch(xs, lens, ys, ol.clone(), train=True)
        eng.clip_sgd_step(mom, 5.0, lr, 0.9, True, False)
        drawn.append(eng.chunk_last())
    return drawn


ms = {name: [] for name in POLICIES}
for rep in range(4):                                            # (the first round warms up and is dropped)
    for name, pol in POLICIES.items():
        eng.set_chunk(pol)
        run(20)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        drawn = run(steps)
        b.record(); b.synchronize()
        if rep:
            ms[name].append(a.elapsed_time(b) / steps)
        assert set(drawn) == ({0} if pol is None else {16}) or pol["dynamic"], (name, set(drawn))
for name, x in ms.items():
    print(f"training step, policy {name:8s}: " + " / ".join(f"{t:.4f}" for t in x) + " ms")
res = {"attention_us": {name: statistics.median(x) for name, x in us.items()}, "step_ms": {name: statistics.median(x) for name, x in ms.items()},
       "dynamic_full_context_share": sum(c == 0 for c in drawn) / len(drawn)}
print(json.dumps(res))
