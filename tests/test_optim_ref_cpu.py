"""tests/optim_ref.py pinned without a GPU: the restatements the GPU tests compare the optimiser and shadow kernels with are themselves compared,
in float64 and over several steps, with torch.optim.SGD / Adam / AdamW and torch.nn.utils.clip_grad_norm_, and the conv / vgg2enc layouts with
what the tested kernels consume (F.conv2d and its input gradient; the inverse of the gradient un-permutation)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_ref as O
import train_rowops_ref as R

F64 = np.float64
N = 257
RTOL = 1e-12           # float64 on both sides, a handful of operations per element and step, six steps


def rnd(seed, n=N, scale=1.0):
    return np.random.default_rng(seed).standard_normal(n) * scale


def close(a, b, what):
    assert np.allclose(a, b, rtol=RTOL, atol=1e-14), (what, float(np.abs(a - b).max()))


# ---------------------------------------------------------------- SGD
@pytest.mark.parametrize("momentum,nesterov", ((0.9, 0), (0.9, 1), (0.0, 0)))
def test_sgd_is_torch_sgd(momentum, nesterov):
    p0 = rnd(1)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([pt], lr=0.05, momentum=momentum, nesterov=bool(nesterov))
    p, mom = p0.copy(), np.full(N, np.nan)                     # (the first step must not read the buffer: NaN would show)
    steps = 6
    for k in range(steps):
        g = rnd(10 + k)
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        flags = (1 if k == 0 else 0) | (2 if k == steps - 1 else 0)
        r = O.sgd(p, g, mom, 1.0, 0.05, momentum, nesterov, flags)
        if momentum == 0.0 or k == steps - 1:
            assert r["mom"] is None                            # nothing to write: no buffer, or the optimiser is dropped
            full = O.sgd(p, g, mom, 1.0, 0.05, momentum, nesterov, flags & 1)
            assert np.array_equal(full["p"], r["p"]), "the last-step bit changes only what is written"
        else:
            mom = r["mom"]
            close(mom, opt.state[pt]["momentum_buffer"].numpy(), ("momentum buffer", k))
        p = r["p"]
        close(p, pt.detach().numpy(), ("p", k))
        assert (r["p_bound"] > 0).all()


def test_sgd_first_and_last_in_one_step():
    """flags 3 (a one-step optimiser): buf = g, nothing read, nothing written"""
    p, g = rnd(2), rnd(3)
    r = O.sgd(p, g, None, 0.5, 0.1, 0.9, 1, 3)
    assert r["mom"] is None
    close(r["p"], p - 0.1 * (0.5 * g + 0.9 * 0.5 * g), "nesterov on the first step")


# ---------------------------------------------------------------- the norm and the clip coefficient
@pytest.mark.parametrize("max_norm", (0.0, 0.5, 5.0, 1e6))
def test_clip_is_clip_grad_norm(max_norm):
    g = rnd(4, scale=0.3).astype(np.float32)
    pt = torch.zeros(N, requires_grad=True)
    pt.grad = torch.tensor(g)
    total = torch.nn.utils.clip_grad_norm_([pt], max_norm)
    assert abs(float(total) - O.norm(g)) <= 4 * N * 2.0 ** -24 * O.norm(g)          # (torch sums in fp32)
    coef = O.clip_coef(np.float32(total), max_norm)
    assert coef.dtype == np.float32 and coef <= 1
    assert np.array_equal(O.scale_bits(g, coef).view(np.int32), pt.grad.numpy().view(np.int32))


def test_clip_coef_edges():
    assert O.clip_coef(np.float32(0.0), 5.0) == 1.0            # 5 / 1e-6 clamped
    assert O.clip_coef(np.float32(0.0), 0.0) == 0.0
    assert O.clip_coef(np.float32(np.inf), 5.0) == 0.0
    assert np.isnan(O.clip_coef(np.float32(np.nan), 5.0))
    assert np.isnan(O.clip_coef(np.float32(np.nan), 0.0))
    c = O.clip_coef(np.float32(10.0), 5.0)
    assert c == np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6)) and c < 0.5
    x = np.full(5, 1e30, np.float32)
    assert np.isfinite(O.norm(x)) and O.norm_f32(x) == np.float32(np.sqrt(5.0) * 1e30)
    assert O.norm_f32(np.full(4, 3e38, np.float32)) == np.inf
    assert np.isnan(O.norm(np.array([1.0, np.nan], np.float32))) and O.norm(np.array([1.0, np.inf], np.float32)) == np.inf


def test_axpy_and_sum_list():
    a, g = rnd(5), rnd(6)
    v, b = O.axpy(a, g, 0.25)
    close(v, a + 0.25 * g, "axpy")
    gs = [rnd(20 + k) for k in range(8)]
    v, b = O.sum_list(gs, 1.0 / 3.0)
    close(v, sum(gs) / 3.0, "sum_list")
    assert (b > 0).all()
    v, b = O.sum_list(gs[:1], 1.0)
    assert np.array_equal(v, gs[0]) and (b <= 2.0 ** -24 * np.abs(v) * O.SLACK).all()


# ---------------------------------------------------------------- Adam / AdamW / Adam with L2
@pytest.mark.parametrize("kind,wd", (("adam", 0.0), ("adam", 0.05), ("adamw", 0.05)))
def test_adam_is_torch_adam(kind, wd):
    lr, b1, b2, eps = 3e-3, 0.9, 0.98, 1e-9
    p0 = rnd(7)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    for t in range(1, 7):
        g = rnd(30 + t)
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        sc = O.adam_scalars(lr, b1, b2, t, wd, int(kind == "adamw"), dtype=F64)
        r = O.adam(p, g, m, v, sc, eps)
        p, m, v = r["p"], r["m"], r["v"]
        close(p, pt.detach().numpy(), (kind, "p", t))
        close(m, opt.state[pt]["exp_avg"].numpy(), (kind, "m", t))
        close(v, opt.state[pt]["exp_avg_sq"].numpy(), (kind, "v", t))
        assert all((r[k] >= 0).all() and np.isfinite(r[k]).all() for k in ("p_bound", "m_bound", "v_bound"))


def test_adam_scalars_fp32_are_single_roundings():
    sc = O.adam_scalars(1e-3, 0.9, 0.98, 3, 0.125, 1)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.98))
    assert sc["step_size"] == float(np.float32(float(np.float32(1e-3)) / (1 - b1 ** 3)))
    assert sc["inv_sqrt_bc2"] == float(np.float32(1 / np.sqrt(1 - b2 ** 3)))
    assert sc["omb1"] == float(np.float32(1) - np.float32(0.9)) and sc["l2"] == 0.0
    assert sc["decay_mul"] == float(np.float32(1) - np.float32(1e-3) * np.float32(0.125))
    assert O.adam_scalars(1e-3, 0.9, 0.98, 3, 0.125, 0)["l2"] == 0.125


def test_adam_sum_is_adam_on_the_scaled_sum():
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p0 = rnd(8)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    for t in range(1, 4):
        gs = [rnd(100 * t + k) for k in range(3)]
        pt.grad = torch.tensor(((gs[0] + gs[1]) + gs[2]) * (1.0 / 3.0), dtype=torch.float64)
        opt.step()
        r = O.adam_sum(p, gs, 1.0 / 3.0, m, v, O.adam_scalars(lr, b1, b2, t, dtype=F64), eps)
        p, m, v = r["p"], r["m"], r["v"]
        close(p, pt.detach().numpy(), ("p", t))
        plain = O.adam(p0, gs[0], np.zeros(N), np.zeros(N), O.adam_scalars(lr, b1, b2, 1, dtype=F64), eps)
        one = O.adam_sum(p0, gs[:1], 1.0, np.zeros(N), np.zeros(N), O.adam_scalars(lr, b1, b2, 1, dtype=F64), eps)
        assert (one["p_bound"] >= plain["p_bound"]).all()      # the summed form carries the rounding of the scale on top


def test_guarded_state_machine_is_skip_on_nan():
    """the training loops' `if isnan(norm): warn else: step()` with a host that runs one launch ahead: launch i is queued knowing the verdicts up to
    launch i - 2, with A = the step number if launch i - 1 was applied and B = if it was skipped"""
    lr, b1, b2, eps, wd = 2e-3, 0.9, 0.98, 1e-9, 0.05
    norms = [1.0, np.nan, 1.0, 1.0, np.nan, np.nan, 1.0, 1.0]
    p0 = rnd(9)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    flags, applied = [0, 0], []
    for i, nv in enumerate(norms):
        g = rnd(200 + i)
        if not np.isnan(nv):
            pt.grad = torch.tensor(g, dtype=torch.float64)
            opt.step()
        known = sum(applied[:max(i - 1, 0)])                   # steps applied among the launches the host has seen finished
        t_a, t_b = (known + 2, known + 1) if i > 0 else (1, 1)
        slot = i & 1
        skip, cand, after = O.guarded(flags, slot, nv)
        assert skip == bool(np.isnan(nv)) and after[slot ^ 1] == flags[slot ^ 1] and after[slot] == int(skip)
        flags = after
        applied.append(0 if skip else 1)
        if not skip:
            t = t_b if cand == "B" else t_a
            assert t == sum(applied)                           # the candidate the flags select IS the optimiser's step number
            r = O.adam(p, g, m, v, O.adam_scalars(lr, b1, b2, t, wd, 1, dtype=F64), eps)
            p, m, v = r["p"], r["m"], r["v"]
        close(p, pt.detach().numpy(), ("p after launch", i))


# ---------------------------------------------------------------- the shadow layouts
@pytest.mark.parametrize("CO,CI", ((4, 3), (2, 5)))
def test_conv_layouts_feed_conv2d_and_its_input_gradient(CO, CI):
    rng = np.random.default_rng(11)
    w = rng.standard_normal((CO, CI, 3, 3))
    x = rng.standard_normal((CI, 5, 6))
    dy = rng.standard_normal((CO, 5, 6))
    wk, wd = O.conv_layouts(w)
    assert wk.shape == (CO, 9 * CI) and wd.shape == (CI, 9 * CO)
    xt = torch.tensor(x[None], requires_grad=True)
    yt = F.conv2d(xt, torch.tensor(w), padding=1)
    close(O.conv_with_operand(x, wk, CO), yt[0].detach().numpy(), "forward from wk")
    yt.backward(torch.tensor(dy[None]))
    close(O.conv_with_operand(dy, wd, CI), xt.grad[0].numpy(), "input gradient from wd")


def test_conv_layouts_elementwise():
    CO, CI = 3, 2
    w = np.arange(CO * CI * 9, dtype=np.float32).reshape(CO, CI, 3, 3)
    wk, wd = O.conv_layouts(w)
    for co in range(CO):
        for ci in range(CI):
            for tap in range(9):
                assert wk[co, tap * CI + ci] == w[co, ci, tap // 3, tap % 3]
                assert wd[ci, tap * CO + co] == w[co, ci, (8 - tap) // 3, (8 - tap) % 3]


@pytest.mark.parametrize("E,C,Dp", ((8, 128, 20), (70, 6, 11), (3, 4, 5)))
def test_vgg2enc_layout_is_the_inverse_of_the_gradient_unpermute(E, C, Dp):
    n = E * C * Dp
    g = torch.arange(n, dtype=torch.float32)                   # a gradient in the engine's order [E][Dp][C]
    dw = R.vgg2enc_unpermute(g, E, C, Dp).numpy()              # ... in the reference's order [E][C][Dp], as the pinned kernel test checks it
    wk, wt = O.vgg2enc_layouts(dw, E, C, Dp)
    assert np.array_equal(wk.reshape(-1), g.numpy())
    assert np.array_equal(wt, wk.T) and wt.shape == (Dp * C, E)
    w = np.arange(n, dtype=np.float32).reshape(E, C * Dp)
    wk, _ = O.vgg2enc_layouts(w, E, C, Dp)
    assert wk[E - 1, (Dp - 1) * C + 1] == w[E - 1, 1 * Dp + Dp - 1]


def test_linear_layouts_and_bf16_cast():
    w = np.arange(12, dtype=np.float32).reshape(3, 4)
    k, t = O.linear_layouts(w)
    assert np.array_equal(k, w) and np.array_equal(t, w.T)
    # round to nearest even at the bf16 grid: 1 + 2^-8 is a tie -> 1 (even); 1 + 3 2^-8 is a tie -> 1 + 2^-6 (even); just above a tie goes up
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8], np.float32)
    assert O.bf16(x).float().tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]
