"""bench.py's plain run (set-up, warm-up, the timed region, the headline line) and --dump-outputs: the same arguments give the same
outputs from run to run -- also for slot 0, on which the one-task leg that sizes the stagger runs a timing-dependent number of steps
first -- and the dump stays inside its budget."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench(cwd, *extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "2", "--tasks-per-gpu", "2", "--single-seconds", "0.2",
                        *extra], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_dumped_outputs_repeat(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench(tmp_path, "--dump-outputs", str(a))
    assert d["full"] is False and d["steps"] == 3 and d["unit"] == "utt/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 16 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    for k in ("long_run", "single_task_fomaml", "single_task_train", "mixed_lengths", "matrix"):
        assert d[k] is None, k
    for k in ("roofline", "meta_step", "e2e_pretrain", "e2e_train", "cpu_baseline"):
        assert k not in d, k
    _bench(tmp_path, "--dump-outputs", str(b))
    names = sorted(p.name for p in a.glob("*.npy"))
    assert names == sorted(p.name for p in b.glob("*.npy"))
    assert names == sorted(f"slot{k}_{n}.npy" for k in range(2) for n in ("stats", "logits", "params", "momentum", "grads"))
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 * 2 ** 20
    loss, n_correct, n_total, grad_norm = np.load(a / "slot0_stats.npy")
    assert loss > 0 and 0 <= n_correct <= n_total and n_total > 0 and grad_norm > 0
    assert np.abs(np.load(a / "slot0_momentum.npy")).max() > 0
