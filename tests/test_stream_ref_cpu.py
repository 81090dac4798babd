"""The streaming first pass without a GPU: the restatement of tests/stream_ref.py -- windowed front-end, per-layer caches, the key
range with the empty-row rule, greedy with carry -- equals the chunk-masked full pass of tests/chunk_ref.py on the padded batch in fp64, whatever
the pieces; a halo of 4 input frames does not; the `valid` bookkeeping; the Tester's argument errors; Tester.MODES against the CLI's choices."""
from types import SimpleNamespace

import pytest
import torch

import hybrid_ref
import stream_ref as S
from masr_amd import tester as tester_mod
from masr_amd.tester import stream_decode_args
from oracle import ref_cpu
from oracle.make_goldens import TINY, ODIM, synth_batch

ILENS = ([160, 140, 120, 100], [150, 97, 64, 41], [67, 30])
POLICIES = ((1, -1), (4, -1), (4, 1), (8, 0), (16, -1), (7, 2), (64, -1))
TOL = 1e-10


@pytest.fixture(scope="module")
def p64():
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7), ODIM, seed=3)
    return {k: v.detach().double() for k, v in hybrid_ref.leafify(sd, TINY).items()}


def batch(ilens):
    xs, il, _, _ = synth_batch(11, ilens, [3] * len(ilens))
    return xs.double(), [int(i) for i in il]


def worst_on_valid(a, b, enc_lens):
    return max(float((a[u, :n] - b[u, :n]).abs().max()) for u, n in enumerate(enc_lens) if n)


FULL = {}


def full(p64, ilens, c, left):
    """the chunk-masked full pass, computed once per (batch, policy) and shared"""
    key = (tuple(ilens), c, left)
    if key not in FULL:
        xs, il = batch(ilens)
        with torch.no_grad():
            FULL[key] = S.full_pass(p64, TINY, xs, il, c, left)
    return FULL[key]


@pytest.mark.parametrize("c,left", POLICIES)
@pytest.mark.parametrize("ilens", ILENS)
def test_stream_equals_the_chunk_masked_full_pass(p64, ilens, c, left):
    xs, il = batch(ilens)
    mem, z, enc_lens = full(p64, ilens, c, left)
    lp = torch.log_softmax(z, -1)
    T = xs.shape[1]
    first = None
    for piece in (T, 64, 7, 1):
        with torch.no_grad():
            st = S.stream(p64, TINY, xs, il, c, left, piece)
        m2, z2 = st.result()
        assert st.emitted == T // 4 == m2.shape[1]
        assert worst_on_valid(m2, mem, enc_lens) <= TOL, (piece, worst_on_valid(m2, mem, enc_lens))
        assert worst_on_valid(torch.log_softmax(z2, -1), lp, enc_lens) <= TOL
        assert bool(torch.isfinite(m2).all())                    # padding rows included (rows without a key: the out-projection's bias)
        if first is None:
            first = (m2, z2, st.tokens, st.frames)
        else:                                                    # the same outputs however the audio was cut
            assert torch.equal(m2, first[0]) and torch.equal(z2, first[1]) and st.tokens == first[2] and st.frames == first[3]
    # streamed greedy = the best path of the full logits
    am = z.argmax(-1)
    for u, n in enumerate(enc_lens):
        assert (first[2][u], first[3][u]) == S.best_path(am[u].tolist(), n)


@pytest.mark.parametrize("c,left", ((4, -1), (8, 0), (16, -1)))
def test_a_halo_of_four_frames_is_not_enough(p64, c, left):
    ilens = ILENS[0]
    xs, il = batch(ilens)
    mem, z, enc_lens = full(p64, ilens, c, left)
    with torch.no_grad():
        st = S.stream(p64, TINY, xs, il, c, left, 64, halo=4)
    miss = worst_on_valid(torch.log_softmax(st.result()[1], -1), torch.log_softmax(z, -1), enc_lens)
    print(f"halo 4, c {c} left {left}: log-probs differ by {miss:.3g}")
    assert miss > 1e-2


def test_valid_bookkeeping(p64):
    """an utterance that ends inside a piece, one that ends exactly at a piece border, and a nonzero valid after an end"""
    ilens = [96, 64, 50]                                         # pieces of 32: 64 ends at a border, 50 inside the second piece
    xs, il = batch(ilens)
    with torch.no_grad():
        want = S.stream(p64, TINY, xs, il, 4, -1, 96)
        st = S.StreamRef(p64, TINY, 3, 4, -1)
        noise = torch.randn(3, 96, xs.shape[2], dtype=xs.dtype, generator=torch.Generator().manual_seed(1))
        dirty = xs.clone()
        for u, n in enumerate(il):
            dirty[u, n:] = noise[u, n:]                          # what stands behind an utterance's end is the engine's to zero
        st.feed(dirty[:, :32], [32, 32, 32])
        st.feed(dirty[:, 32:64], [32, 32, 18])                   # 50 ends inside; 64 has all 32 valid: not ended yet
        assert st.ended == [False, False, True]
        with pytest.raises(ValueError, match="has ended"):
            st.feed(dirty[:, 64:], [32, 0, 5], last=True)
        st.feed(dirty[:, 64:], [32, 0, 0], last=True)            # 64 ends exactly at the border: its next piece gives 0
        assert st.len == ilens and st.ended == [True] * 3
    assert torch.equal(st.result()[1], want.result()[1]) and st.tokens == want.tokens
    with pytest.raises(ValueError, match=r"\[0, n\]"):
        S.StreamRef(p64, TINY, 3, 4, -1).feed(xs[:, :8], [9, 8, 8])


def test_tester_argument_errors():
    hybrid = dict(TINY, ctc_weight=0.3)
    paras = lambda **kw: SimpleNamespace(**kw)
    pol = dict(size=8, left=-1, dynamic=0)
    for mode in ("stream_ctc_greedy", "stream_ctc_beam"):
        assert stream_decode_args(hybrid, paras(), mode, pol) == 32
        assert stream_decode_args(hybrid, paras(stream_piece=7), mode, pol) == 7
        with pytest.raises(ValueError, match="--decode_chunk"):
            stream_decode_args(hybrid, paras(), mode, None)
        with pytest.raises(ValueError, match="--decode_chunk"):
            stream_decode_args(hybrid, paras(), mode, dict(size=0, left=-1, dynamic=1))
        with pytest.raises(ValueError, match="needs a CTC output layer"):
            stream_decode_args(TINY, paras(), mode, pol)
        with pytest.raises(ValueError, match="--stream_piece"):
            stream_decode_args(hybrid, paras(stream_piece=0), mode, pol)
        with pytest.raises(NotImplementedError, match="BLSTM"):
            stream_decode_args(hybrid, paras(), mode, None, model_name="blstm")


def test_modes_equal_the_cli_choices():
    import train
    act = next(a for a in train.build_parser()._actions if a.dest == "decode_mode")
    assert set(act.choices) == set(tester_mod.Tester.MODES)
    assert {"stream_ctc_greedy", "stream_ctc_beam"} <= set(tester_mod.Tester.MODES)
    a = train.build_parser().parse_args(["--config", "x", "--accent", "af", "--algo", "no", "--test", "--decode_mode", "stream_ctc_beam", "--stream_piece", "48"])
    assert a.stream_piece == 48
