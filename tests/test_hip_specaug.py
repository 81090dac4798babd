"""SpecAugment on the GPU: the kernel behind masr_specaug against the numpy restatement (tests/specaug_ref.py), and the training step
that runs it -- what the engine feeds its encoder, that conv1's forward and weight gradient both read it, graph replay, resume."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import specaug_ref as R  # noqa: E402
from masr_amd._cabi import MasrError, MasrSpecaugPolicy, lib  # noqa: E402
from masr_amd.engine import MasrEngine, specaug  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from test_specaug_ref_cpu import GPU_LENS, GPU_POLICY, GPU_SEED, GPU_STEP  # noqa: E402

GUARD = 1024                                                    # floats on either side of the output
ILENS, OLENS = [64, 52, 40, 33], [9, 7, 5, 3]                   # the tiny engine batch of tests/test_hip_engine.py ("ragged")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def loss_stats(e):
    st = e.read_stats()                                         # (the gradient norm is only formed by the optimiser passes)
    return st["loss"], st["n_correct"], st["n_total"]


def nan_padded(lens, D, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.full((len(lens), max(lens), D), float("nan"))
    for b, n in enumerate(lens):
        xs[b, :n] = torch.randn(n, D, generator=g)
    return xs


def run_guarded(xs_dev, lens, policy, seed, step):
    """masr_specaug into the middle of a sentinel-filled buffer -> (out [B, T, D], the whole buffer)"""
    B, T, D = xs_dev.shape
    n = B * T * D
    buf = torch.full((n + 2 * GUARD,), -7.25, device="cuda")
    pol = MasrSpecaugPolicy(*[R.full_policy(policy, D)[k] for k in R.KEYS])
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rc = lib().masr_specaug(C.c_void_p(xs_dev.data_ptr()), C.c_void_p(lens_dev.data_ptr()), C.c_void_p(buf.data_ptr() + 4 * GUARD), B, T, D,
                            C.byref(pol), C.c_uint64(seed), C.c_uint64(step), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib().masr_last_error()
    torch.cuda.synchronize()
    return buf[GUARD:GUARD + n].view(B, T, D), buf


def check_against_reference(xs, lens, policy, seed, step):
    out, buf = run_guarded(xs.cuda(), lens, policy, seed, step)
    got = out.cpu().numpy()
    ref, a, b, kind = R.specaug(xs.numpy(), lens, policy, seed, step)
    assert not np.isnan(got).any()
    g32 = got.view(np.int32)
    assert np.all(g32[kind == 0] == 0)                          # masks and padding: +0.0f
    x32 = ref.astype(np.float32).view(np.int32)                 # (a copied cell's fp64 value IS the fp32 input)
    assert np.array_equal(g32[kind == 1], x32[kind == 1])       # copied cells, bit for bit
    # Interpolated cells: the exact value is v = a + phi (b - a), phi = r / den in (0, 1).  The kernel rounds three times with unit roundoff
    # u = 2^-24: phi^ = phi (1 + d1), (b - a)^ = (b - a)(1 + d2), and the fused multiply-add (1 + d3).  To first order the error is
    # u (2 phi |b - a| + |v|) <= u (2 (|a| + |b|) + max(|a|, |b|)) <= 3 u (|a| + |b|) < 2^-22 (|a| + |b|); with the product rounded on its own (no
    # fused multiply-add) a fourth rounding gives 4 u (|a| + |b|) = 2^-22 (|a| + |b|).  The factor 2 covers the second-order terms and the
    # equivalent (1 - phi) a + phi b form.
    m = kind == 2
    err, bound = np.abs(got.astype(np.float64) - ref)[m], 2.0 ** -21 * (np.abs(a) + np.abs(b))[m]
    print(f"interpolated cells {int(m.sum())}, worst error / bound {float((err / np.maximum(bound, 1e-300)).max()) if m.any() else 0.0:.3f}")
    assert np.all(err <= bound)
    assert torch.all(buf[:GUARD] == -7.25) and torch.all(buf[-GUARD:] == -7.25)      # nothing written outside the output
    return kind


def test_stateless_call_matches_the_reference():
    xs = nan_padded(GPU_LENS, 83, 5)                            # B = 6, T = 300: 25 workgroups per utterance
    kind = check_against_reference(xs, GPU_LENS, GPU_POLICY, GPU_SEED, GPU_STEP)
    assert all((kind == k).any() for k in (0, 1, 2))
    seen = set()
    xs = nan_padded([37, 36, 12], 80, 6)
    for step in range(3):
        seen |= set(np.unique(check_against_reference(xs, [37, 36, 12], GPU_POLICY, GPU_SEED, step)).tolist())
    assert seen == {0, 1, 2}


def test_off_policy_is_a_bit_exact_copy():
    for lens, D in ((GPU_LENS, 83), ([37, 36, 12], 80)):
        xs = nan_padded(lens, D, 7)
        out, buf = run_guarded(xs.cuda(), lens, None, GPU_SEED, 3)
        want = torch.nan_to_num(xs, nan=0.0)                    # (the data holds no NaN: only the padding did)
        assert same_bits(out.cpu(), want)
        assert torch.all(buf[:GUARD] == -7.25) and torch.all(buf[-GUARD:] == -7.25)
        assert same_bits(specaug(xs.cuda(), lens, None, GPU_SEED, 3).cpu(), want)


def test_stateless_call_vets_its_arguments():
    xs = torch.zeros(2, 16, 83, device="cuda")
    for bad in (dict(freq_masks=9), dict(time_masks=1, time_ratio=1.5), dict(freq_masks=1, freq_bins=84), dict(time_warp=-1)):
        with pytest.raises(ValueError):
            specaug(xs, [16, 16], bad, 1, 0)
    pol = MasrSpecaugPolicy(0, 9, 0, 83, 0, 0, 0.0)
    lens = torch.tensor([16, 16], dtype=torch.int32, device="cuda")
    out = torch.empty_like(xs)
    args = lambda o, p: (C.c_void_p(xs.data_ptr()), C.c_void_p(lens.data_ptr()), C.c_void_p(o.data_ptr()), 2, 16, 83, C.byref(p), 1, 0, None)
    assert lib().masr_specaug(*args(out, pol)) == -1 and b"freq_masks" in lib().masr_last_error()
    assert lib().masr_specaug(*args(xs, MasrSpecaugPolicy(0, 0, 0, 83, 0, 0, 0.0))) == -1 and b"another buffer" in lib().masr_last_error()


@pytest.fixture(scope="module")
def sd():
    return ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)


def engine(sd, policy, dropout=0.0, seed=77):
    cfg = dict(TINY, dropout=dropout, pos_dropout=dropout)
    if policy is not None:
        cfg["specaug"] = policy
    e = MasrEngine(cfg, ODIM, label_smoothing=0.2)
    e.load_state_dict(sd); e.set_seed(seed)
    return e


def test_engine_feeds_its_encoder_what_the_stateless_call_gives(sd):
    xs, il, ys, ol = synth_batch(11, ILENS, OLENS)
    xs_nan = xs.clone()
    for b, n in enumerate(ILENS):
        xs_nan[b, n:] = float("nan")                             # under a policy the step never reads the padding of its input
    e = engine(sd, GPU_POLICY)
    assert e.specaug == GPU_POLICY
    with pytest.raises(MasrError, match="did not augment"):
        e.specaug_last()
    xd = xs_nan.cuda()
    for _ in range(2):
        state = e.dropout_state()
        e.run_batch(xd, il, ys, ol, train=True)
        xa = e.specaug_last()
        assert xa.shape == xs.shape and same_bits(xa, specaug(xd, il, GPU_POLICY, *state))
        assert np.isfinite(e.read_stats()["loss"]) and bool(torch.isfinite(e.grads).all())
    assert not same_bits(xa, torch.nan_to_num(xd, nan=0.0))      # (it did augment)
    # evaluation never augments: the loss of a policy-free engine on the raw batch
    plain = engine(sd, None)
    e.run_batch(xs.cuda(), il, ys, ol, train=False)
    plain.run_batch(xs.cuda(), il, ys, ol, train=False)
    assert loss_stats(e) == loss_stats(plain)
    with pytest.raises(MasrError, match="did not augment"):
        e.specaug_last()
    # ... and set_specaug(None) is the policy-free training step, bit for bit
    e.set_specaug(None); e.set_dropout_state(plain.dropout_state())
    e.run_batch(xs.cuda(), il, ys, ol, train=True)
    plain.run_batch(xs.cuda(), il, ys, ol, train=True)
    assert loss_stats(e) == loss_stats(plain) and same_bits(e.grads, plain.grads)


def test_conv1_forward_and_weight_gradient_both_read_the_augmented_batch(sd):
    """engine A augments xs itself, engine B (no policy) gets the pre-augmented batch: same loss, same gradient, bit for bit -- the loss
    differs if conv1's forward keeps reading xs, feat_extractor.0.weight's gradient if conv1's weight gradient does"""
    xs, il, ys, ol = synth_batch(11, ILENS, OLENS)
    xd = xs.cuda()
    A, Bm = engine(sd, GPU_POLICY, dropout=0.1), engine(sd, None, dropout=0.1)
    state = (1234, 5)
    A.set_dropout_state(state); Bm.set_dropout_state(state)
    xa = specaug(xd, il, GPU_POLICY, *state)
    A.run_batch(xd, il, ys, ol, train=True)
    Bm.run_batch(xa, il, ys, ol, train=True)
    assert loss_stats(A) == loss_stats(Bm)
    assert same_bits(A.grads, Bm.grads)
    assert same_bits(A.view("feat_extractor.0.weight", A.grads), Bm.view("feat_extractor.0.weight", Bm.grads))
    Bm.run_batch(xd, il, ys, ol, train=True)                     # (the raw batch gives another gradient: the comparison above can fail)
    assert not same_bits(A.view("feat_extractor.0.weight", A.grads), Bm.view("feat_extractor.0.weight", Bm.grads))


def test_replayed_graphs_see_the_steps_seed_and_lengths(sd):
    xs, il, ys, ol = synth_batch(11, ILENS, OLENS)
    xd = xs.cuda()
    e = engine(sd, GPU_POLICY, dropout=0.1)
    e.set_step_graphs(True)
    outs = []
    with torch.cuda.stream(torch.cuda.Stream()):                 # (steps on the legacy NULL stream are never captured)
        for k in range(4):
            lens = il.clone()
            if k == 3:
                lens[1] -= 5                                     # another raw length at the same shape (olens unchanged)
            state = e.dropout_state()
            e.run_batch(xd, lens, ys, ol, train=True)
            xa = e.specaug_last().clone()
            assert same_bits(xa, specaug(xd, lens, GPU_POLICY, *state)), k
            outs.append(xa)
        torch.cuda.current_stream().synchronize()
    c = e.step_counters()
    assert c["captured"] == 1 and c["replayed"] >= 2, c
    assert all(not same_bits(outs[k], outs[k + 1]) for k in range(3))
    assert bool((outs[3][1, int(il[1]) - 5:] == 0).all())


def test_resumed_position_repeats_the_augmentation(sd):
    xs, il, ys, ol = synth_batch(11, ILENS, OLENS)
    xd = xs.cuda()
    e = engine(sd, GPU_POLICY)
    e.run_batch(xd, il, ys, ol, train=True)
    saved = e.dropout_state()
    first = e.specaug_last().clone()
    e.run_batch(xd, il, ys, ol, train=True)
    second = e.specaug_last().clone()
    assert not same_bits(first, second)
    e.set_dropout_state(saved)
    e.run_batch(xd, il, ys, ol, train=True)
    assert same_bits(e.specaug_last(), second)
