"""The CPU restatement of the BLSTM path's LSTM kernels (tests/lstm_ref.py) against independent facts, and its checkers against an honest fp32
emulation of the kernels and against mutated ones.  The free-running fp64 form must be torch.nn.LSTM(bidirectional, batch_first) on a packed
batch -- outputs and, through autograd, the gradient wrt the gate pre-activations; the permutation helpers must round-trip against torch's
g * H + u layout; the checkers must pass the emulation at every shape of the GPU test (the worst err / bound per tolerance class is printed:
the evidence that a correct fp32 / bf16 evaluation stays inside the bounds on the chosen inputs) and must fail every mutation.  CPU only."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_ref as L

F64 = torch.float64


def _torch_lstm(H, B, T, lens, seed):
    """nn.LSTM whose input IS the gate pre-activation contribution: input size 4H, W_ih = identity, no biases -- so x.grad = dL/dz"""
    torch.manual_seed(seed)
    m = torch.nn.LSTM(4 * H, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for sfx in ("", "_reverse"):
            getattr(m, "weight_ih_l0" + sfx).copy_(torch.eye(4 * H))
            getattr(m, "bias_ih_l0" + sfx).zero_()
            getattr(m, "bias_hh_l0" + sfx).zero_()
            getattr(m, "weight_hh_l0" + sfx).mul_(3.0)          # (so that the recurrent term matters)
    return m


@pytest.mark.parametrize("H,B,T,lens", [(8, 4, 6, [4, 6, 1, 3]), (5, 3, 7, [7, 1, 2]), (40, 2, 3, [3, 2]), (3, 1, 1, [1])])
def test_free_running_form_is_torch_lstm_forward_and_gate_gradient(H, B, T, lens):
    g = torch.Generator().manual_seed(H + T)
    m = _torch_lstm(H, B, T, lens, seed=H)
    lens_t = torch.tensor(lens)
    r = L.unit_major_rows(H)
    # the two directions get different inputs (torch feeds one x to both: a second LSTM run carries the reverse direction's)
    xs = [(torch.randn(B, T, 4 * H, generator=g, dtype=F64) * 2.0).requires_grad_(True) for _ in range(2)]
    dy = torch.randn(B, T, 2 * H, generator=g, dtype=F64)
    outs = []
    for x in xs:
        packed = pack_padded_sequence(x, lens_t, batch_first=True, enforce_sorted=False)
        o, _ = pad_packed_sequence(m(packed)[0], batch_first=True, total_length=T)
        outs.append(o)
    want_y = torch.cat((outs[0][..., :H], outs[1][..., H:]), dim=-1)
    (outs[0][..., :H] * dy[..., :H]).sum().backward()
    (outs[1][..., H:] * dy[..., H:]).sum().backward()
    # torch's column g * H + u -> the kernels' u * 4 + g
    gx = [xs[0].detach()[..., r], xs[1].detach()[..., r]]
    w = [m.weight_hh_l0.detach()[r], m.weight_hh_l0_reverse.detach()[r]]
    y, act, c = L.blstm_free(gx, w, lens_t)
    assert (y - want_y).abs().max() <= 1e-12, float((y - want_y).abs().max())
    for b, n in enumerate(lens):
        assert (y[b, n:] == 0).all() and (act[0][b, n:] == 0).all() and (c[1][b, n:] == 0).all()
    dz = L.blstm_free_bwd(dy, act, c, w, lens_t)
    for d in range(2):
        want = xs[d].grad[..., r]
        assert (dz[d] - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max())), (d, float((dz[d] - want).abs().max()))
        for b, n in enumerate(lens):
            assert (dz[d][b, n:] == 0).all()


def test_permutation_helpers_round_trip_against_torch_layout():
    H, pc, pd = 6, 4, 5
    K = pc * pd
    g = torch.Generator().manual_seed(3)
    wih, whh = torch.randn(4 * H, K, generator=g), torch.randn(4 * H, H, generator=g)
    bih, bhh = torch.randn(4 * H, generator=g), torch.randn(4 * H, generator=g)
    for p in ((0, 0), (pc, pd)):
        wih16, wihT16, whh16, whhT16, bias = L.shadows(wih, whh, bih, bhh, H, K, *p)
        for u in range(H):
            for gate in range(4):
                assert bias[u * 4 + gate] == bih[gate * H + u] + bhh[gate * H + u]
                assert torch.equal(whh16[u * 4 + gate, :H], whh[gate * H + u].bfloat16()) and (whh16[u * 4 + gate, H:] == 0).all()
                for k in (0, 1, pc, K - 1):
                    tk = (k % pc) * pd + k // pc if p[0] else k              # NHWC position d * pc + c <- torch's c * pd + d
                    assert wih16[u * 4 + gate, k] == wih[gate * H + u, tk].bfloat16()
        assert torch.equal(wihT16, wih16.t()) and torch.equal(whhT16, whh16[:, :H].t()) and whh16.shape[1] == 32
        # the un-permutation is the inverse of the shadow's permutation
        perm = wih[L.unit_major_rows(H)][:, L.src_col(K, *p)]
        assert torch.equal(L.unperm(perm, H, K, *p), wih)
    # an nn.LSTM cell agrees with fwd_step on unit-major columns
    cell = torch.nn.LSTMCell(3, H).double()
    x, h0, c0 = torch.randn(2, 3, dtype=F64), torch.randn(2, H, dtype=F64), torch.randn(2, H, dtype=F64)
    z = x @ cell.weight_ih.t() + cell.bias_ih + h0 @ cell.weight_hh.t() + cell.bias_hh
    _, c1, h1 = L.fwd_step(z[:, L.unit_major_rows(H)].view(2, H, 4), c0)
    hw, cw = cell(x, (h0, c0))
    assert (h1 - hw).abs().max() < 1e-14 and (c1 - cw).abs().max() < 1e-14


def test_bf16_half_ulp():
    v = torch.tensor([1.0, 1.99, 2.0, 0.75, 3e-5], dtype=F64)
    assert L.bf16_half_ulp(v).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -24]
    # a correctly rounded value is within it, and the bound is attained to within a fraction: 2^-9 |v| would refuse correct roundings
    x = torch.linspace(1.0, 2.0, 4097, dtype=F64)
    err = (x.float().bfloat16().double() - x).abs()
    assert (err <= L.bf16_half_ulp(x)).all() and float(err.max()) == 2.0 ** -8


_RESULTS = {}


def _emulated(H, B, T, resident):
    key = (H, B, T, resident)
    if key not in _RESULTS:
        case = L.make_case(H, B, T)
        y16, act, c = L.emulate_fwd(case, resident)
        act_s, c_s = (act, c) if not resident else _emulated(H, B, T, 0)[2:4]      # the backward is fed the per-step forward's act / c
        _RESULTS[key] = (case, y16, act, c, L.emulate_bwd(case, act_s, c_s, resident))
    return _RESULTS[key]


@pytest.fixture(scope="module")
def worst():
    w = L.Worst()
    yield w
    print("\nfp32 emulation, worst err / bound per tolerance class:", {k: round(v, 4) for k, v in sorted(w.items())})


@pytest.mark.parametrize("resident", (0, 1))
@pytest.mark.parametrize("H,B,T", L.COMBOS)
def test_checkers_pass_the_honest_emulation(worst, H, B, T, resident):
    case, y16, act, c, dz16 = _emulated(H, B, T, resident)
    L.check_fwd(case["lens"], case["gx"], case["whh16"], y16, act, c, worst, (H, B, T, resident))
    act_s, c_s = _emulated(H, B, T, 0)[2:4]
    L.check_bwd(case["lens"], case["dy"], act_s, c_s, case["whhT16"], dz16, worst, (H, B, T, resident))


def test_inputs_reach_their_cases():
    for H, B, T in L.COMBOS:
        case = L.make_case(H, B, T)
        lens = case["lens"].tolist()
        assert len(lens) == B and all(1 <= n <= T for n in lens)
        if B >= 3:
            assert lens[1] == T and lens[2] == 1 and lens[0] == max(1, (T + 1) // 2) and (T < 3 or lens != sorted(lens))
    _, _, act, _, _ = _emulated(40, 32, 12, 0)
    a = act[0][torch.isfinite(act[0])].view(-1, 4)
    sat = ((a[:, 0] < 0.01) | (a[:, 0] > 0.99)).float().mean()
    lin = ((a[:, 0] > 0.25) & (a[:, 0] < 0.75)).float().mean()
    assert sat > 0.1 and lin > 0.2, (float(sat), float(lin))


MUT_SHAPES = ((40, 3, 5), (8, 17, 5))


@pytest.mark.parametrize("resident", (0, 1))
@pytest.mark.parametrize("mut", L.FWD_MUTATIONS)
def test_forward_checker_fails_the_mutation(mut, resident):
    for H, B, T in MUT_SHAPES:
        case = L.make_case(H, B, T)
        y16, act, c = L.emulate_fwd(case, resident, mut)
        with pytest.raises(AssertionError):
            L.check_fwd(case["lens"], case["gx"], case["whh16"], y16, act, c, L.Worst(), mut)


@pytest.mark.parametrize("resident", (0, 1))
@pytest.mark.parametrize("mut", L.BWD_MUTATIONS)
def test_backward_checker_fails_the_mutation(mut, resident):
    for H, B, T in MUT_SHAPES:
        case = L.make_case(H, B, T)
        _, act, c = L.emulate_fwd(case, 0)
        dz16 = L.emulate_bwd(case, act, c, resident, mut)
        with pytest.raises(AssertionError):
            L.check_bwd(case["lens"], case["dy"], act, c, case["whhT16"], dz16, L.Worst(), mut)
