"""The chunk mask without a GPU: properties of the restatement (tests/chunk_ref.py) that the GPU tests compare the kernels and the engine
with, that the batch of tests/test_hip_chunk.py can tell a chunked encoder from a full-context one, the asr_model.chunk validator, the
--decode_chunk / --decode_left argument errors and the BLSTM trainer's refusal."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import masr_amd  # noqa: F401
import chunk_ref as R
import hybrid_ref
from masr_amd.blstm_trainer import get_trainer
from masr_amd.engine import chunk_of
from masr_amd.tester import decode_chunk_policy
from oracle import ref_cpu
from oracle.make_goldens import TINY, ODIM, synth_batch

# the cases tests/test_hip_chunk.py runs on the GPU: a ragged TINY batch of 40 encoder frames (ten chunks of 4) under these policies, with the
# bounds that test copies from tests/test_hip_engine.py for the comparison with the bf16-emulating oracle: loss 2e-4, logits 4e-3 (rel. l2).
# Those are the bounds an engine that accepted the key and ignored it would have to miss.  (Against the fp32 oracle the loss bound is 1e-3.)
GPU_SEED, GPU_ILENS, GPU_OLENS, GPU_EPS, GPU_W = 11, [160, 140, 120, 100], [9, 7, 5, 3], 0.2, 0.3
GPU_POLICIES = [dict(size=4, left=-1, dynamic=0), dict(size=4, left=1, dynamic=0)]
LOSS_TOL, LOGIT_TOL = 2e-4, 4e-3


def test_visible_set_against_three_nested_loops():
    for T, klen, c, left in [(10, 10, 3, -1), (10, 7, 3, 0), (17, 12, 4, 1), (16, 16, 4, 2), (9, 5, 1, -1), (9, 9, 1, 0), (12, 6, 5, 0), (8, 8, 0, -1), (8, 3, 0, 2)]:
        want = np.zeros((T, T), bool)
        for i in range(T):
            for j in range(T):
                ok = j < klen
                if c > 0:
                    ok = ok and j < (i // c + 1) * c and (left < 0 or j >= (i // c - left) * c)
                want[i, j] = ok
        np.testing.assert_array_equal(R.visible(T, klen, c, left), want)


def test_one_chunk_is_no_mask_and_chunks_of_one_are_the_causal_mask():
    for T, klen in [(10, 10), (10, 6), (33, 20)]:
        pad_only = np.broadcast_to(np.arange(T)[None, :] < klen, (T, T))
        for c in (T, T + 7, 1000):
            np.testing.assert_array_equal(R.visible(T, klen, c, -1), pad_only)
        np.testing.assert_array_equal(R.visible(T, klen, 0, -1), pad_only)
    for T in (1, 7, 40):
        causal = ref_cpu.generate_square_subsequent_mask(T).numpy() == 0
        np.testing.assert_array_equal(R.visible(T, T, 1, -1), causal)


def test_rows_without_a_visible_key_are_padding_rows_behind_the_window():
    for T, klen, c, left in [(40, 20, 8, 0), (40, 17, 8, 1), (30, 30, 4, 0), (64, 3, 16, -1)]:
        vis = R.visible(T, klen, c, left)
        empty = ~vis.any(-1)
        want = np.array([left >= 0 and max(i // c - left, 0) * c >= klen for i in range(T)])
        np.testing.assert_array_equal(empty, want)
        assert not empty[:klen].any()


def test_draw_is_half_full_context_and_reaches_every_chunk():
    draws = [R.chunk_draw(seed, step, 250) for seed in range(64) for step in range(64)]
    full = sum(d == 0 for d in draws) / len(draws)
    assert 0.4 <= full <= 0.6, full
    assert set(draws) == set(range(26))
    assert all(R.chunk_draw(s, 0, Tp) == 0 for s in range(50) for Tp in (0, 1))
    assert all(0 <= R.chunk_draw(s, 3, 9) <= 5 for s in range(200))             # r <= Tp / 2 = 4: chunks 2 .. 5, or none


def test_attention_reference_agrees_with_autograd_and_zeroes_empty_rows():
    g = torch.Generator().manual_seed(0)
    B, T, H, hd = 2, 23, 2, 8
    q, k, v, dout = (torch.randn(B, T, H, hd, generator=g, dtype=torch.float64) for _ in range(4))
    keep = (torch.rand(B, H, T, T, generator=g) > 0.2).double() / 0.8
    klens = [23, 11]
    for c, left in ((4, -1), (4, 1), (5, 0)):
        out = R.attention(q, k, v, dout, klens, c, left, keep=keep)
        vis = torch.from_numpy(np.stack([R.visible(T, n, c, left) for n in klens]))[:, None]
        empty = ~vis.any(-1)
        assert bool(empty.any()) == (left >= 0)                    # (klen 11: the padding rows from chunk 3 + left on)
        qa, ka, va = (t.clone().permute(0, 2, 1, 3).requires_grad_(True) for t in (q, k, v))
        s = (qa @ ka.transpose(-1, -2)) / hd ** 0.5
        s = s.masked_fill(~(vis | empty[..., None]), float("-inf"))
        p = torch.softmax(s, -1).masked_fill(empty[..., None], 0.0)               # WeNet: zero the rows behind the softmax
        o = (p * keep) @ va
        o.backward(dout.permute(0, 2, 1, 3))
        for n, t in (("o", o.detach()), ("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
            torch.testing.assert_close(out[n], t.permute(0, 2, 1, 3), rtol=1e-10, atol=1e-12)
        e = out["empty"]
        assert bool((out["o"][e] == 0).all()) and bool((out["dq"][e] == 0).all()) and bool((out["lse"].permute(0, 2, 1)[e] == 0).all())
        assert all(bool(torch.isfinite(t).all()) for t in out.values())


def test_front_end_reads_input_frames_up_to_4t_plus_9():
    """what the future-independence test of tests/test_hip_chunk.py relies on: encoder-input frame t depends on the input frames <= 4 t + 9 (four
    3 x 3 convs and two 2 x 2 pools), so a change from frame 4 E + 6 on leaves the frames < E alone -- and frame E does read frame 4 E + 6"""
    sd = ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)
    xs, il, _, _ = synth_batch(11, [160], [5])
    for E in (8, 24):
        x2 = xs.clone()
        x2[:, 4 * E + 6:] += 1.0
        a, _ = ref_cpu.extract_feat(sd, xs, il)
        b, _ = ref_cpu.extract_feat(sd, x2, il)
        assert torch.equal(a[:, :E], b[:, :E])
        x3 = xs.clone()
        x3[:, 4 * E + 5] += 1.0                                   # = 4 (E - 1) + 9: the last frame that frame E - 1 reads
        c, _ = ref_cpu.extract_feat(sd, x3, il)
        assert not torch.equal(a[:, E - 1], c[:, E - 1]) and torch.equal(a[:, :E - 1], c[:, :E - 1])


@pytest.fixture(scope="module")
def losses():
    """oracle losses of the GPU test's batch: {(hybrid?, policy index or None): loss}, and the plain model's logits under ("logit", ...)"""
    xs, il, ys, ol = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    plain = ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)
    hyb = hybrid_ref.with_head(plain, ODIM, seed=3)
    out = {}
    for pi, pol in [(None, None)] + list(enumerate(GPU_POLICIES)):
        with R.chunked_oracle(pol["size"], pol["left"]) if pol else R.chunked_oracle(0):
            with torch.no_grad():
                logit, gold = ref_cpu.model_forward(plain, TINY, xs, il, ys, ol.clone())
                out[(False, pi)] = float(ref_cpu.label_smoothed_ce(logit, gold, GPU_EPS)[0])
                out[("logit", pi)] = logit
                l_ctc, _ = hybrid_ref.ctc_term(hyb, TINY, xs, il, ys, ol)
                out[(True, pi)] = (1 - GPU_W) * out[(False, pi)] + GPU_W * float(l_ctc)
    return out


def test_full_context_through_the_chunked_encoder_is_the_oracle(losses):
    xs, il, ys, ol = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    sd = ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)
    with torch.no_grad():
        logit, gold = ref_cpu.model_forward(sd, TINY, xs, il, ys, ol.clone())
    assert abs(float(ref_cpu.label_smoothed_ce(logit, gold, GPU_EPS)[0]) - losses[(False, None)]) <= 1e-6 * losses[(False, None)]


@pytest.mark.parametrize("pi", range(len(GPU_POLICIES)))
def test_the_gpu_batch_tells_a_chunked_encoder_from_a_full_context_one(losses, pi):
    """The hybrid model's loss (its CTC term reads every encoder frame) moves by at least 10 x the loss bound.  The plain model's loss does not:
    its decoder averages the memory through cross-attention and the label-smoothed CE of random weights moves by 2e-4 .. 8e-4 under any chunk
    (every seeded batch and policy tried) -- there the logits tell the two apart, by at least 10 x their bound."""
    full, chunked = losses[(True, None)], losses[(True, pi)]
    print(f"hybrid {GPU_POLICIES[pi]}: loss {chunked:.6f}, full context {full:.6f}, apart by {abs(chunked - full) / full:.2e} relative")
    assert abs(chunked - full) >= 10 * LOSS_TOL * full
    lf, lc = losses[("logit", None)], losses[("logit", pi)]
    apart = float((lc - lf).norm() / lf.norm())
    print(f"plain {GPU_POLICIES[pi]}: logits apart by {apart:.3f} (rel. l2), loss by {abs(losses[(False, pi)] - losses[(False, None)]) / losses[(False, None)]:.2e}")
    assert apart >= 10 * LOGIT_TOL


HK = {"idim": 83}


def test_chunk_of_accepts():
    assert chunk_of(HK) is None and chunk_of(dict(HK, chunk=None)) is None
    assert chunk_of(dict(HK, chunk={})) is None and chunk_of(dict(HK, chunk=dict(size=0, left=3))) is None      # nothing to mask = off
    assert chunk_of(dict(HK, chunk=dict(size=16))) == dict(size=16, left=-1, dynamic=0)
    assert chunk_of(dict(HK, chunk=dict(size=16, left=2, dynamic=1))) == dict(size=16, left=2, dynamic=1)
    assert chunk_of(dict(HK, chunk=dict(dynamic=True))) == dict(size=0, left=-1, dynamic=1)
    assert chunk_of(dict(HK, chunk=dict(size=np.int64(4), left=0))) == dict(size=4, left=0, dynamic=0)


@pytest.mark.parametrize("pol,key", [(dict(size=-1), "size"), (dict(size=4, left=-2), "left"), (dict(size=4, dynamic=2), "dynamic"), (dict(size=1.5), "size"),
                                     (dict(size=True), "size"), (dict(size=4, left="all"), "left"), (dict(size=4, right=1), "right"), (dict(size=2 ** 31), "size")])
def test_chunk_of_rejects(pol, key):
    with pytest.raises(ValueError, match=key):
        chunk_of(dict(HK, chunk=pol))


def test_chunk_of_rejects_a_non_mapping():
    with pytest.raises(ValueError, match="mapping"):
        chunk_of(dict(HK, chunk=16))


def test_decode_chunk_arguments():
    paras = lambda **kw: SimpleNamespace(**kw)
    yaml_pol = dict(HK, chunk=dict(size=16, left=2, dynamic=1))
    assert decode_chunk_policy(HK, paras()) == (None, False)
    assert decode_chunk_policy(yaml_pol, paras(decode_chunk=None, decode_left=None)) == (dict(size=16, left=2, dynamic=1), False)
    assert decode_chunk_policy(HK, paras(decode_chunk=8)) == (dict(size=8, left=-1, dynamic=0), True)
    assert decode_chunk_policy(HK, paras(decode_chunk=8, decode_left=1)) == (dict(size=8, left=1, dynamic=0), True)
    assert decode_chunk_policy(yaml_pol, paras(decode_chunk=4)) == (dict(size=4, left=2, dynamic=1), True)
    assert decode_chunk_policy(yaml_pol, paras(decode_left=-1)) == (dict(size=16, left=-1, dynamic=1), True)
    assert decode_chunk_policy(dict(HK, chunk=dict(size=16)), paras(decode_chunk=0)) == (None, True)           # one checkpoint, scored with full context
    for kw, msg in ((dict(decode_chunk=-1), "--decode_chunk"), (dict(decode_chunk=8, decode_left=-2), "--decode_left"), (dict(decode_left=1), "needs a chunk")):
        with pytest.raises(ValueError, match=msg):
            decode_chunk_policy(HK, paras(**kw))
    with pytest.raises(ValueError, match="transformer only"):
        decode_chunk_policy(HK, paras(decode_chunk=8), model_name="blstm")
    assert decode_chunk_policy(yaml_pol, paras(), model_name="blstm") == (None, False)


def test_train_py_takes_the_two_flags():
    import train
    a = train.build_parser().parse_args(["--config", "x", "--accent", "af", "--algo", "no", "--test", "--decode_chunk", "8", "--decode_left", "1"])
    assert (a.decode_chunk, a.decode_left) == (8, 1)
    a = train.build_parser().parse_args(["--config", "x", "--accent", "af", "--algo", "no"])
    assert a.decode_chunk is None and a.decode_left is None


def test_blstm_trainer_refuses_the_key():
    with pytest.raises(ValueError, match="transformer only"):
        get_trainer(object, {"asr_model": {"chunk": dict(size=16)}}, None, None)
