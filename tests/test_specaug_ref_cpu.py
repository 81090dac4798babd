"""SpecAugment without a GPU: properties of the numpy restatement (tests/specaug_ref.py) that the GPU tests compare the kernel with,
the asr_model.specaug validator, and the BLSTM trainer's refusal."""
import numpy as np
import pytest

import masr_amd  # noqa: F401
import specaug_ref as R
from masr_amd.blstm_trainer import get_trainer
from masr_amd.engine import specaug_of

# the case tests/test_hip_specaug.py runs on the GPU
GPU_POLICY = dict(time_warp=5, freq_masks=2, freq_width=30, freq_bins=80, time_masks=2, time_width=40, time_ratio=0.2)
GPU_LENS, GPU_SEED, GPU_STEP, D = [300, 257, 64, 11, 10, 4], 531, 0, 83


def batch(lens, d=D, seed=3):
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((len(lens), max(lens), d)).astype(np.float32)
    for b, n in enumerate(lens):
        xs[b, n:] = np.nan                                      # the padding of the input is never read
    return xs


def test_off_policy_is_a_copy_with_zeroed_padding():
    lens = [37, 36, 12]
    xs = batch(lens, 80)
    for policy in (None, {}, dict(freq_width=30, time_width=40, time_ratio=1.0)):      # no warp, no masks: widths alone do nothing
        out, a, b, kind = R.specaug(xs, lens, policy, 531, 7)
        for i, n in enumerate(lens):
            np.testing.assert_array_equal(out[i, :n], xs[i, :n].astype(np.float64))
            assert np.all(out[i, n:] == 0.0) and np.all(kind[i, :n] == 1) and np.all(kind[i, n:] == 0)
        assert not np.isnan(out).any()


def test_draws_stay_inside_their_bounds():
    """widths and starts over 200 (seed, step) pairs, several lengths and policies, the edge values included"""
    policies = [GPU_POLICY, dict(time_warp=40, freq_masks=8, freq_width=200, freq_bins=83, time_masks=8, time_width=1000, time_ratio=1.0),
                dict(time_warp=1, freq_masks=1, freq_width=0, freq_bins=1, time_masks=1, time_width=3, time_ratio=0.0)]
    rng = np.random.default_rng(0)
    for k in range(200):
        seed, step = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
        p = policies[k % 3]
        for b, n in enumerate([4, 11, 81, 82, 300, 1000]):
            dr = R.draws(p, D, n, b, seed, step)
            W, Df = p["time_warp"], p["freq_bins"]
            if n <= 2 * W:
                assert dr["warp"] is None
            else:
                c, cw = dr["warp"]
                assert W <= c <= n - W - 1 and abs(cw - c) <= W - 1 and 1 <= cw <= n - 2
            assert len(dr["freq"]) == p["freq_masks"] and len(dr["time"]) == p["time_masks"]
            for f0, f in dr["freq"]:
                assert 0 <= f <= min(p["freq_width"], Df) and 0 <= f0 and f0 + f <= Df
            cap = min(p["time_width"], int(np.floor(np.float32(p["time_ratio"]) * np.float32(n))))
            for t0, tau in dr["time"]:
                assert 0 <= tau <= cap and 0 <= t0 and t0 + tau <= n


def test_warp_keeps_the_end_rows_and_is_monotone():
    rng = np.random.default_rng(1)
    moved = 0
    for k in range(200):
        n, W = int(rng.integers(3, 400)), int(rng.integers(1, 50))
        dr = R.draws(dict(time_warp=W), D, n, k % 7, int(rng.integers(0, 2 ** 63)), k)
        if n <= 2 * W:
            assert dr["warp"] is None                           # too short for the window: never warped
            continue
        i, r, den = R.source_rows(n, dr["warp"])
        assert (i[0], r[0]) == (0, 0) and (i[n - 1], r[n - 1]) == (n - 1, 0)      # row 0 and row n - 1 survive
        c, cw = dr["warp"]
        assert (i[cw], r[cw]) == (c, 0)                         # the centre lands on a source row exactly
        pos = i + r / den
        assert np.all(np.diff(pos) > 0) and np.all((r == 0) | (i + 1 <= n - 1)) and np.all(r < den)
        if c == cw:
            assert np.all(r == 0) and np.all(i == np.arange(n))
        moved += c != cw
    assert moved > 50


def test_short_utterances_are_never_warped():
    xs = batch([10, 4, 2])
    out, _, _, kind = R.specaug(xs, [10, 4, 2], dict(time_warp=5), 531, 0)
    for b, n in enumerate([10, 4, 2]):
        np.testing.assert_array_equal(out[b, :n], xs[b, :n].astype(np.float64))
        assert np.all(kind[b, :n] == 1)


def test_gpu_case_is_not_vacuous():
    """the case the kernel is compared on shows every branch: a moved warp centre, a frequency mask and a time mask of positive width,
    interpolated cells, and utterances too short to warp"""
    ds = [R.draws(GPU_POLICY, D, n, b, GPU_SEED, GPU_STEP) for b, n in enumerate(GPU_LENS)]
    assert [d["warp"] is not None for d in ds] == [True, True, True, True, False, False]
    assert any(d["warp"] and d["warp"][0] != d["warp"][1] for d in ds)
    assert ds[3]["warp"] == (5, 3)
    assert any(f > 0 for d in ds for _, f in d["freq"]) and any(tau > 0 for d in ds for _, tau in d["time"])
    _, _, _, kind = R.specaug(batch(GPU_LENS), GPU_LENS, GPU_POLICY, GPU_SEED, GPU_STEP)
    assert all((kind == k).any() for k in (0, 1, 2))
    assert (kind[:, :, 80:][:, :4] != 0).any()                  # freq_bins = 80 spares the pitch dims
    for b, n in enumerate(GPU_LENS):
        tmask = np.zeros(n, bool)
        for t0, tau in ds[b]["time"]:
            tmask[t0:t0 + tau] = True
        assert np.all(kind[b, :n, 80:][~tmask] != 0)


HK = dict(idim=83, d_model=64)


def test_specaug_of_accepts():
    assert specaug_of(HK) is None and specaug_of(dict(HK, specaug=None)) is None
    assert specaug_of(dict(HK, specaug={})) is None             # nothing to do = off
    assert specaug_of(dict(HK, specaug=dict(freq_width=30, time_width=40))) is None
    p = specaug_of(dict(HK, specaug=GPU_POLICY))
    assert p == GPU_POLICY and tuple(p) == R.KEYS
    p = specaug_of(dict(HK, specaug=dict(freq_masks=2, freq_width=27)))
    assert p == dict(time_warp=0, freq_masks=2, freq_width=27, freq_bins=83, time_masks=0, time_width=0, time_ratio=0.0)
    assert specaug_of(dict(HK, specaug=dict(time_masks=8, time_width=0, time_ratio=1, freq_bins=1)))["time_ratio"] == 1.0


@pytest.mark.parametrize("key,val", [("time_warp", -1), ("time_warp", 2.5), ("freq_masks", 9), ("freq_masks", -1), ("freq_width", -3),
                                     ("freq_bins", 0), ("freq_bins", 84), ("time_masks", 9), ("time_masks", True), ("time_width", -1),
                                     ("time_ratio", 1.5), ("time_ratio", -0.1), ("time_ratio", float("nan")), ("time_ratio", "0.2"),
                                     ("fill", 0)])
def test_specaug_of_rejects(key, val):
    with pytest.raises(ValueError, match=key):
        specaug_of(dict(HK, specaug=dict(GPU_POLICY, **{key: val})))


def test_specaug_of_rejects_a_non_mapping():
    with pytest.raises(ValueError, match="asr_model.specaug"):
        specaug_of(dict(HK, specaug=[5, 2, 30]))


def test_blstm_trainer_refuses_the_key():
    with pytest.raises(ValueError, match="asr_model.specaug: transformer only"):
        get_trainer(object, {"asr_model": {"specaug": GPU_POLICY}}, None, None)
