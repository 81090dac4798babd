"""The chunk mask inside the attention kernels (csrc/attention.hip, template parameter CH), through masr_test_attention_chunk: every
kernel body -- head dim 64: the 4-wave and the 8-wave ring forward, the one- and two-tile ring backward; head dim 16 / 32: the
register-staged bodies -- against the fp64 restatement of tests/chunk_ref.py, and the exact properties the mask promises.

Tolerances are test_attention's (tests/test_hip_kernels.py): o 2e-2; gradients rtol 3e-2, atol 4e-2.  lse is compared at 1e-3: the scores
are fp32 sums of exact bf16 products (<= 64 terms), exp2 / log are ~1e-6 relative and |lse| stays below ~10, so its error is ~1e-5."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import chunk_ref as R  # noqa: E402
from masr_amd import _cabi  # noqa: E402

B_, H = 2, 2


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def inputs(T, hd, seed=0, lo=None):
    """q, k, v, dout bf16 [B, T, H, hd] and ragged klens from T / 2 upward (the first utterance keeps `lo` keys where given)"""
    g = torch.Generator(device="cuda").manual_seed(T * 7 + hd + seed)
    q, k, v, dout = (torch.randn(B_, T, H, hd, device="cuda", generator=g).bfloat16() for _ in range(4))
    klens = torch.randint(max(1, T // 2), T + 1, (B_,), device="cuda", generator=g).int()
    if lo is not None:
        klens[0] = lo
    return q, k, v, dout, klens


def run(q, k, v, dout, klens, c, left, causal=0, drop=0.0, seed=0, site=0, chunk_dev=None, Tk=None, fill=0.0, expect=0):
    """-> dict o, dq, dk, dv (bf16), lse (fp32)"""
    T, hd = q.shape[1], q.shape[3]
    out = {n: torch.full_like(t, fill) for n, t in (("o", q), ("dq", q), ("dk", k), ("dv", v))}
    out["lse"] = torch.full((B_, H, T), fill, device="cuda")
    rc = _cabi.lib().masr_test_attention_chunk(P(q), P(k), P(v), P(dout), P(out["o"]), P(out["dq"]), P(out["dk"]), P(out["dv"]), P(out["lse"]), P(klens),
                                               B_, H, T, k.shape[1] if Tk is None else Tk, hd, causal, drop, seed, site, c, left, P(chunk_dev), S())
    torch.cuda.synchronize()
    assert rc == expect, _cabi.lib().masr_last_error()
    return out


def plain(q, k, v, dout, klens, causal):
    T, hd = q.shape[1], q.shape[3]
    out = {n: torch.zeros_like(t) for n, t in (("o", q), ("dq", q), ("dk", k), ("dv", v))}
    out["lse"] = torch.zeros(B_, H, T, device="cuda")
    delta = torch.zeros(B_, H, T, device="cuda")
    _cabi.check(_cabi.lib().masr_test_attention(P(q), P(k), P(v), P(dout), P(out["o"]), P(out["dq"]), P(out["dk"]), P(out["dv"]), P(out["lse"]), P(delta),
                                                P(klens), B_, H, T, T, hd, causal, S()))
    torch.cuda.synchronize()
    return out


def check_against_reference(got, ref, what):
    worst = {}
    for n, rtol, atol in (("o", 2e-2, 2e-2), ("dq", 3e-2, 4e-2), ("dk", 3e-2, 4e-2), ("dv", 3e-2, 4e-2), ("lse", 0.0, 1e-3)):
        a, r = got[n].double().cpu(), ref[n]
        assert bool(torch.isfinite(a).all()), (what, n)
        worst[n] = float(((a - r).abs() - rtol * r.abs()).max())
        assert worst[n] <= atol, f"{what}: {n} misses by {worst[n]:.4g} > atol {atol}"
    print(what, {n: f"{w:.3g}" for n, w in worst.items()})


# (hd, T): 4-wave ring | 8-wave forward and the two-tile backward at one, just over one and just over two 64-row blocks | more blocks than
# ring stages, the dK/dV statistics refreshed inside the loop | the register-staged bodies
SHAPES = [(64, 40), (64, 64), (64, 65), (64, 130), (64, 300), (64, 700), (32, 100), (16, 10), (16, 70)]


@pytest.mark.parametrize("left", [-1, 1])
@pytest.mark.parametrize("ci", range(6))
@pytest.mark.parametrize("hd,T", SHAPES)
def test_chunked_attention_matches_the_fp64_reference(hd, T, ci, left):
    c = (1, 3, 24, 64, T, T + 7)[ci]
    q, k, v, dout, klens = inputs(T, hd)
    got = run(q, k, v, dout, klens, c, left, fill=7.0)
    check_against_reference(got, R.attention(q, k, v, dout, klens.tolist(), c, left), f"hd {hd} T {T} c {c} left {left}")
    for b in range(B_):                                          # keys behind klen: exactly zero gradient
        assert bool((got["dk"][b, int(klens[b]):] == 0).all()) and bool((got["dv"][b, int(klens[b]):] == 0).all())


@pytest.mark.parametrize("left", [-1, 1, 2])
@pytest.mark.parametrize("T", [300, 700])
def test_long_sequences_skip_blocks_from_both_ends(T, left):
    q, k, v, dout, klens = inputs(T, 64, seed=1)
    got = run(q, k, v, dout, klens, 16, left, fill=7.0)
    check_against_reference(got, R.attention(q, k, v, dout, klens.tolist(), 16, left), f"T {T} c 16 left {left}")


@pytest.mark.parametrize("hd,T", [(64, 40), (64, 130), (64, 300), (32, 100), (16, 70)])
def test_rows_without_a_visible_key_are_exact_zeros(hd, T):
    q, k, v, dout, klens = inputs(T, hd, seed=2, lo=T // 2)
    c = 8
    got = run(q, k, v, dout, klens, c, 0, fill=7.0)
    ref = R.attention(q, k, v, dout, klens.tolist(), c, 0)
    empty = ref["empty"].cuda()                                  # [B, T]
    assert int(empty[0].sum()) >= T // 2 - c                     # (padding rows whose own chunk starts at or behind klen)
    assert bool((got["o"][empty] == 0).all()) and bool((got["dq"][empty] == 0).all())
    assert bool((got["lse"].permute(0, 2, 1)[empty] == 0).all())
    check_against_reference(got, ref, f"hd {hd} T {T} c {c} left 0, klen {T // 2}")


@pytest.mark.parametrize("hd,T,c,left", [(64, 40, 8, -1), (64, 130, 24, -1), (64, 130, 24, 1), (64, 300, 16, 2), (32, 100, 10, 1), (16, 70, 7, -1)])
def test_masked_keys_get_exactly_nothing_from_queries_that_cannot_see_them(hd, T, c, left):
    """only dout of a set of queries changes; the dk / dv rows of the keys none of them sees keep their bits"""
    q, k, v, dout, klens = inputs(T, hd, seed=3)
    i0 = (T // 2 // c) * c                                       # a chunk boundary
    d2 = dout.clone()
    if left < 0:                                                 # the queries before i0 see no key from i0 on
        d2[:, :i0] = (d2[:, :i0].float() * 1.5 + 0.25).bfloat16()
        unseen = slice(i0, T)
    else:                                                        # the queries from i0 on see no key before their window
        d2[:, i0:] = (d2[:, i0:].float() * 1.5 + 0.25).bfloat16()
        unseen = slice(0, max(i0 - left * c, 0))
    assert unseen.stop > unseen.start
    a, b = run(q, k, v, dout, klens, c, left), run(q, k, v, d2, klens, c, left)
    assert same(a["dk"][:, unseen], b["dk"][:, unseen]) and same(a["dv"][:, unseen], b["dv"][:, unseen])
    assert not same(a["dk"], b["dk"]) and not same(a["dv"], b["dv"])


@pytest.mark.parametrize("hd,T,c,left", [(64, 40, 8, -1), (64, 130, 24, 1), (64, 300, 16, -1), (64, 700, 16, 2), (32, 100, 10, -1), (16, 70, 7, 1)])
def test_keys_behind_the_last_visible_one_do_not_reach_a_query(hd, T, c, left):
    q, k, v, dout, klens = inputs(T, hd, seed=4)
    klens[:] = T
    hi = (T // 2 // c + 1) * c                                   # the queries < hi see no key >= hi
    k2, v2 = k.clone(), v.clone()
    k2[:, hi:] = (k2[:, hi:].float() * -2.0 + 1.0).bfloat16()
    v2[:, hi:] = (v2[:, hi:].float() * 3.0 - 1.0).bfloat16()
    a, b = run(q, k, v, dout, klens, c, left), run(q, k2, v2, dout, klens, c, left)
    assert same(a["o"][:, :hi], b["o"][:, :hi]) and same(a["lse"][:, :, :hi], b["lse"][:, :, :hi]) and same(a["dq"][:, :hi], b["dq"][:, :hi])
    assert not same(a["o"][:, hi:], b["o"][:, hi:])


@pytest.mark.parametrize("hd,T", [(64, 40), (64, 65), (64, 130), (64, 300), (32, 100), (16, 70)])
def test_one_chunk_is_no_mask_and_chunks_of_one_are_the_causal_mask_bit_for_bit(hd, T):
    q, k, v, dout, klens = inputs(T, hd, seed=5)
    want = plain(q, k, v, dout, klens, 0)
    for c in (T, T + 7):
        got = run(q, k, v, dout, klens, c, -1)
        assert all(same(got[n], want[n]) for n in want), c
    want, got = plain(q, k, v, dout, klens, 1), run(q, k, v, dout, klens, 1, -1)
    assert all(same(got[n], want[n]) for n in want)


@pytest.mark.parametrize("hd,T,c,left", [(64, 130, 24, 1), (64, 300, 16, 2), (64, 40, 8, -1), (16, 70, 7, -1)])
def test_dropout_draws_the_keep_bits_of_the_unshifted_indices(hd, T, c, left):
    p, seed, site = 0.1, 4321, 7
    q, k, v, dout, klens = inputs(T, hd, seed=6)
    got = run(q, k, v, dout, klens, c, left, drop=p, seed=seed, site=site)
    keep = torch.empty(B_ * H * T * T, device="cuda")
    _cabi.check(_cabi.lib().masr_test_dropout_mask(seed, site, keep.numel(), p, P(keep), S()))
    check_against_reference(got, R.attention(q, k, v, dout, klens.tolist(), c, left, keep=keep.view(B_, H, T, T)), f"dropout hd {hd} T {T} c {c} left {left}")


@pytest.mark.parametrize("hd,T,c,left", [(64, 130, 24, 1), (64, 40, 3, -1), (32, 100, 10, 0), (16, 70, 7, 2)])
def test_the_chunk_read_from_device_memory_gives_the_same_bits(hd, T, c, left):
    q, k, v, dout, klens = inputs(T, hd, seed=7)
    want = run(q, k, v, dout, klens, c, left, drop=0.1, seed=9, site=3)
    got = run(q, k, v, dout, klens, 12345, left, drop=0.1, seed=9, site=3, chunk_dev=torch.tensor([c], dtype=torch.int32, device="cuda"))
    assert all(same(got[n], want[n]) for n in want)
    # a 0 read there is full context: the kernels without the mask
    got = run(q, k, v, dout, klens, 5, left, chunk_dev=torch.zeros(1, dtype=torch.int32, device="cuda"))
    want = plain(q, k, v, dout, klens, 0)
    assert all(same(got[n], want[n]) for n in want)


def test_refusals_leave_the_outputs_unwritten():
    q, k, v, dout, klens = inputs(40, 64, seed=8)
    dev = torch.tensor([4], dtype=torch.int32, device="cuda")
    for kw, msg in ((dict(c=4, left=-1, causal=1), b"causal"), (dict(c=0, left=-1, causal=1, chunk_dev=dev), b"causal"), (dict(c=4, left=-1, Tk=39), b"Tq == Tk"),
                    (dict(c=4, left=-2), b"left >= -1"), (dict(c=-1, left=-1), b"chunk >= 0")):
        out = run(q, k, v, dout, klens, fill=-7.25, expect=-1, **kw)
        assert msg in _cabi.lib().masr_last_error(), (kw, _cabi.lib().masr_last_error())
        assert all(bool((t == -7.25).all()) for t in out.values()), kw
