#!/usr/bin/env python3
"""What SpecAugment inside the training step costs at the hkust shape (B = 16, T = 1000, D = 83):
  1. the pass itself (masr_specaug) beside masr_gather_pad on the same shape -- the same bytes written, the natural yardstick: device
     events around WINDOW back-to-back launches, the two alternating, REPS windows each;
  2. the single-task training step (run_batch + clip + SGD, k-split on as train.py runs it) with the policy off and on, in one process,
     the legs alternating.
python tools/bench_specaug.py [seconds per step leg = 1.0]      prints one JSON line at the end"""
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
from masr_amd._cabi import MasrSpecaugPolicy, check, lib
from masr_amd.engine import SPECAUG_KEYS, MasrEngine
from masr_amd.model import reference_init_state_dict

HK = dict(idim=83, nheads=8, d_model=512, d_inner=2048, dropout=0.1, pos_dropout=0.1, tgt_share_weight=1, encoder=dict(nlayers=2),
          decoder=dict(nlayers=4), meta={"optimizer_opt": {"k": 1.0, "warmup_steps": 25000}})
POLICY = dict(time_warp=5, freq_masks=2, freq_width=30, freq_bins=80, time_masks=2, time_width=40, time_ratio=0.2)
B, T, D = 16, 1000, 83
WINDOW, REPS = 500, 7
secs = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
assert torch.cuda.is_available(), "needs the MI355X"
g = torch.Generator().manual_seed(0)
lens = torch.randint(600, T + 1, (B,), generator=g)
lens[0] = T
xs = torch.zeros(B, T, D)
for b in range(B):
    xs[b, :int(lens[b])] = torch.randn(int(lens[b]), D, generator=g)
xs = xs.cuda()
L = lib()
vp = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

# ---- 1. the pass beside gather_pad
lens32 = lens.to(torch.int32).cuda()
feat = torch.randn(int(lens.sum()), D, device="cuda")           # the shard rows gather_pad reads: the same bytes SpecAugment reads from xs
row_start = (torch.cumsum(lens, 0) - lens).cuda()
out = torch.empty_like(xs)
pol = MasrSpecaugPolicy(*[POLICY[k] for k in SPECAUG_KEYS])
off = MasrSpecaugPolicy(0, 0, 0, D, 0, 0, 0.0)
legs = {
    "gather_pad": lambda i: L.masr_gather_pad(vp(feat), vp(row_start), vp(lens32), vp(out), B, T, D, stream()),
    "specaug": lambda i: L.masr_specaug(vp(xs), vp(lens32), vp(out), B, T, D, C.byref(pol), 531, i, stream()),
    "specaug_off_policy": lambda i: L.masr_specaug(vp(xs), vp(lens32), vp(out), B, T, D, C.byref(off), 531, i, stream()),
}
us = {k: [] for k in legs}
for rep in range(REPS + 1):                                     # (the first round warms up and is dropped)
    for name, fn in legs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(WINDOW):
            check(fn(i), name)
        b.record(); b.synchronize()
        if rep:
            us[name].append(a.elapsed_time(b) * 1e3 / WINDOW)
mb = (int(lens.sum()) + B * T) * D * 4 / 1e6                    # valid rows read + the whole batch written
for name, v in us.items():
    print(f"{name:20s} {min(v):6.2f} us best, {statistics.median(v):6.2f} us median of {REPS} x {WINDOW} launches  ({mb / min(v):.2f} TB/s at best; the 5 MB buffers repeat, so the caches serve part of it)")

# ---- 2. the training step, policy off / on
torch.manual_seed(531)
sd = reference_init_state_dict(HK, 367)
ol = torch.randint(10, 41, (B,), generator=g)
ys = [torch.randint(1, 366, (int(n),), generator=g) for n in ol]
eng = MasrEngine(HK, 367, label_smoothing=0.2)
eng.load_state_dict(sd)
eng.set_ksplit(True)
mom = torch.zeros_like(eng.params)
lr = 512 ** -0.5 * 25000 ** -0.5


def run(n):
    for _ in range(n):
        eng.run_batch(xs, lens, ys, ol.clone(), train=True)
        eng.clip_sgd_step(mom, 5.0, lr, 0.9, True, False)
    torch.cuda.synchronize()


ms = {False: [], True: []}
for rep in range(4):
    for on in (False, True):
        eng.set_specaug(POLICY if on else None)
        run(30)
        t0 = time.perf_counter(); run(50); dt = (time.perf_counter() - t0) / 50
        n = max(50, int(secs / dt))
        t0 = time.perf_counter(); run(n); dt = (time.perf_counter() - t0) / n
        if rep:
            ms[on].append(dt * 1e3)
        if on:
            eng.specaug_last()                                  # (raises unless the last step augmented)
for on, v in ms.items():
    print(f"training step, policy {'on ' if on else 'off'}: " + " / ".join(f"{x:.4f}" for x in v) + " ms")
res = {"shape": [B, T, D], "gather_pad_us": min(us["gather_pad"]), "specaug_us": min(us["specaug"]), "specaug_off_policy_us": min(us["specaug_off_policy"]),
       "step_ms_policy_off": statistics.median(ms[False]), "step_ms_policy_on": statistics.median(ms[True])}
res["step_cost_pct"] = 100.0 * (res["step_ms_policy_on"] / res["step_ms_policy_off"] - 1.0)
print(json.dumps(res))
