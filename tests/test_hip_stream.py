"""The streaming first pass through the engine (include/masr.h masr_stream_*) on the GPU, TINY hybrid model: the streamed head
logits against the bf16-emulating chunked oracle with the full-pass engine's own error as the yardstick, bit-identity over the piece size and
finality of emitted rows, the streamed greedy decode and the final beam against their restatements, the stream's lifecycle and the Tester."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import chunk_ref as R  # noqa: E402
import ctc_beam_ref as cr  # noqa: E402
import hybrid_ref  # noqa: E402
import stream_ref  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from masr_amd._cabi import MasrError  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, JOINT_DELTA, joint_state_dict, make_tester  # noqa: E402

POLICIES = ((8, -1), (8, 1), (4, 0))
BATCHES = ([160, 140, 120, 100], [150, 97, 64, 41])


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def sdh():
    return hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7), ODIM, seed=3)


def engine(sd, c, left, odim=ODIM):
    cfg = dict(TINY, dropout=0.0, pos_dropout=0.0, ctc_weight=0.3)
    if c:
        cfg["chunk"] = dict(size=c, left=left)
    e = MasrEngine(cfg, odim)
    e.load_state_dict(sd)
    return e


def streamed(eng, xs, il, piece, odim=ODIM):
    """-> (head logits [B, T / 4, odim] (a copy), greedy (tokens, frames) per utterance)"""
    greedy = eng.recog_stream(xs, il, piece)
    z, enc_lens, frames = eng.stream_logits()
    assert frames == xs.shape[1] // 4 and enc_lens.cpu().tolist() == [int(i) // 4 for i in il]
    return z[:, :frames, :odim].clone().cpu(), greedy


def valid_rows(lp, enc_lens):
    """[B, T', C] -> the valid frames of every utterance, stacked"""
    return torch.cat([lp[b, :n] for b, n in enumerate(enc_lens)])


@pytest.mark.parametrize("c,left", POLICIES)
@pytest.mark.parametrize("ilens", BATCHES)
def test_streamed_logits_against_the_chunked_oracle(sdh, ilens, c, left):
    """rel-l2 of the log-probabilities over the valid frames; the yardstick is the full-pass engine's error on the same batch and policy
    (recog_ctc_beam + last_ctc_beam_logits): both make the same roundings in another summation order, so the stream may miss by 1.5 x that"""
    xs, il, _, _ = synth_batch(11, ilens, [3] * len(ilens))
    B, T = xs.shape[:2]
    eng = engine(sdh, c, left)
    with R.chunked_oracle(c, left), ref_cpu.bf16_emulation(), torch.no_grad():
        lp, lens = hybrid_ref.ctc_log_probs(hybrid_ref.leafify(sdh, TINY), TINY, xs, il)
    lens = lens.tolist()
    ref = valid_rows(lp.transpose(0, 1), lens)
    z, _ = streamed(eng, xs, il, 64)
    assert bool(torch.isfinite(z).all())
    err_stream = rel_l2(valid_rows(torch.log_softmax(z, -1), lens), ref)
    eng.recog_ctc_beam(xs, il, 4)
    zf, _ = eng.last_ctc_beam_logits(B, T, 4)
    err_full = rel_l2(valid_rows(torch.log_softmax(zf[:, :, :ODIM].cpu(), -1), lens), ref)
    worst = float((valid_rows(torch.log_softmax(z, -1), lens) - ref).abs().max())
    apart = rel_l2(valid_rows(z, lens), valid_rows(zf[:, :, :ODIM].cpu(), lens))
    print(f"ilens {ilens} policy {{{c}, {left}}}: stream {err_stream:.6e}, full pass {err_full:.6e} (rel-l2 of the log-probs); worst abs {worst:.3e}; "
          f"stream against full pass {apart:.3e} (rel-l2 of the logits)")
    assert err_stream <= 1.5 * err_full, (err_stream, err_full)


@pytest.mark.parametrize("c,left", ((16, -1), (16, 2)))
def test_key_ranges_split_over_the_waves_against_the_chunked_oracle(sdh, c, left):
    """the same comparison and bound at 150 encoder frames: with left = -1 the later chunks' key ranges are two and three 64-key blocks, which
    attn_stream_kernel splits over its waves and merges; with left = 2 the range starts inside the cache (lo > 0)"""
    ilens = [600, 410]
    xs, il, _, _ = synth_batch(15, ilens, [3] * len(ilens))
    B, T = xs.shape[:2]
    eng = engine(sdh, c, left)
    with R.chunked_oracle(c, left), ref_cpu.bf16_emulation(), torch.no_grad():
        lp, lens = hybrid_ref.ctc_log_probs(hybrid_ref.leafify(sdh, TINY), TINY, xs, il)
    lens = lens.tolist()
    ref = valid_rows(lp.transpose(0, 1), lens)
    z, _ = streamed(eng, xs, il, 100)
    assert bool(torch.isfinite(z).all())
    err_stream = rel_l2(valid_rows(torch.log_softmax(z, -1), lens), ref)
    eng.recog_ctc_beam(xs, il, 4)
    zf = eng.last_ctc_beam_logits(B, T, 4)[0][:, :, :ODIM].cpu()
    err_full = rel_l2(valid_rows(torch.log_softmax(zf, -1), lens), ref)
    print(f"ilens {ilens} policy {{{c}, {left}}}: stream {err_stream:.6e}, full pass {err_full:.6e} (rel-l2 of the log-probs); "
          f"stream against full pass {rel_l2(valid_rows(z, lens), valid_rows(zf, lens)):.3e} (rel-l2 of the logits)")
    assert err_stream <= 1.5 * err_full, (err_stream, err_full)


@pytest.mark.parametrize("c,left", POLICIES)
def test_pieces_do_not_change_a_bit_and_emitted_rows_are_final(sdh, c, left):
    ilens = BATCHES[0]
    xs, il, _, _ = synth_batch(11, ilens, [3] * len(ilens))
    B, T = xs.shape[:2]
    eng = engine(sdh, c, left)
    z0, g0 = streamed(eng, xs, il, T)
    for piece in (64, 7):
        z, g = streamed(eng, xs, il, piece)
        assert same_bits(z, z0) and g == g0, piece
    # only the first 4e + 8 frames: the rows < e are final
    e = c
    n0 = 4 * e + 8
    eng.stream_begin(B, T)
    assert eng.stream_feed(xs[:, :n0]) == e
    head = eng.stream_logits()[0][:, :e, :ODIM].clone().cpu()
    assert same_bits(head, z0[:, :e])
    assert eng.stream_feed(xs[:, n0:], [max(0, int(l) - n0) for l in il], last=True) == T // 4
    assert same_bits(eng.stream_logits()[0][:, :T // 4, :ODIM].cpu(), z0)
    # ... also when the rest is noise; the rows from e on do change
    noise = torch.randn(B, T - n0, xs.shape[2], generator=torch.Generator().manual_seed(5))
    eng.stream_begin(B, T)
    eng.stream_feed(xs[:, :n0])
    eng.stream_feed(noise, last=True)
    zn = eng.stream_logits()[0][:, :T // 4, :ODIM].cpu()
    assert same_bits(zn[:, :e], z0[:, :e])
    assert not same_bits(zn[:, e:2 * e], z0[:, e:2 * e])


DECODE_BATCHES = ((12, [128, 100, 72, 60]), (13, [96, 80, 64]), (14, [160, 96, 64, 40]))


def oracle_log_probs(sdj, xs, il, c, left):
    with R.chunked_oracle(c, left), ref_cpu.bf16_emulation(), torch.no_grad():
        lp, lens = hybrid_ref.ctc_log_probs(hybrid_ref.leafify(sdj, TINY), TINY, xs, il)
    return lp.transpose(0, 1).contiguous()[..., :C_SMALL], lens.tolist()


@pytest.mark.parametrize("c,left", POLICIES)
def test_streamed_greedy_vs_the_best_path_of_the_chunked_oracle(c, left):
    """the peaked hybrid model of decode_util.py; utterances whose every per-frame top-1 / top-2 gap exceeds JOINT_DELTA are compared"""
    sdj = joint_state_dict(TINY, 7)
    eng = engine(sdj, c, left, odim=C_SMALL)
    ok = n = 0
    for seed, ilens in DECODE_BATCHES:
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        got = eng.recog_stream(xs, il, 48)
        lp, lens = oracle_log_probs(sdj, xs, il, c, left)
        for b, T_b in enumerate(lens):
            n += 1
            top = lp[b, :T_b].topk(2, -1).values
            if not float((top[:, 0] - top[:, 1]).min()) > JOINT_DELTA:
                continue
            ok += 1
            assert got[b] == stream_ref.best_path(lp[b].argmax(-1).tolist(), T_b), (seed, b)
    print(f"streamed greedy under {{{c}, {left}}}: {ok} of {n} utterances above the gap; tokens and frames identical")
    assert ok >= 0.5 * n, (ok, n)


def test_the_final_beam_is_the_search_on_the_streams_logits():
    """stream_ctc_beam = masr_ctc_beam_search on stream_logits, bit for bit; and = ctc_beam_ref on the chunked oracle under the gap filter and
    score tolerance of tests/test_hip_chunk.py::test_ctc_beam_under_a_chunk_vs_the_restatement"""
    sdj = joint_state_dict(TINY, 7)
    eng = engine(sdj, 8, -1, odim=C_SMALL)
    L = _cabi.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    for K, nbest in ((4, 3), (1, 1)):
        ok = n = 0
        for seed, ilens in DECODE_BATCHES:
            xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
            B, T = xs.shape[:2]
            eng.recog_stream(xs, il, 64)
            tok, lens, scores = eng.stream_ctc_beam(K, nbest, raw=True)
            z, enc_lens, _ = eng.stream_logits()
            cap = T // 4
            wb = int(L.masr_ctc_beam_work_bytes(B, cap, C_SMALL, K))
            work = torch.empty(wb, dtype=torch.uint8, device="cuda")
            t2, l2, s2 = torch.empty_like(tok), torch.empty_like(lens), torch.empty_like(scores)
            _cabi.check(L.masr_ctc_beam_search(P(z), z.shape[2], P(enc_lens), B, cap, C_SMALL, K, nbest, 0, C_SMALL - 1, P(work), wb, P(t2), P(l2), P(s2),
                                               eng.stream()))
            torch.cuda.synchronize()
            assert torch.equal(tok, t2) and torch.equal(lens, l2) and same_bits(scores, s2)
            got = _cabi.nbest_lists(tok, lens, scores)
            lp, elens = oracle_log_probs(sdj, xs, il, 8, -1)
            for b, r in enumerate(cr.ctc_beam_ref_batch(lp.numpy(), elens, K, 0, C_SMALL - 1, nbest)):
                n += 1
                if not r["min_gap"] > JOINT_DELTA:
                    continue
                ok += 1
                hyp, s = got[b][0]
                pre, want = r["nbest"][0]
                assert tuple(hyp) == pre and abs(s - want) <= 0.1 + 3e-3 * abs(want), (K, seed, b, hyp, pre, s, want)
        print(f"stream_ctc_beam under a chunk of 8, K = {K}: {ok} of {n} utterances above the gap; best hypothesis identical")
        assert ok >= 0.5 * n, (K, ok, n)


def test_stream_lifecycle(sdh):
    xs, il, ys, ol = synth_batch(11, [64, 52, 40, 33], [9, 7, 5, 3])
    eng = engine(sdh, 8, -1)
    eng.stream_begin(4, 64)
    eng.stream_feed(xs[:, :40])
    eng.run_batch(xs, il, ys, ol, train=False)                   # plans the workspace: the stream is over
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_feed(xs[:, 40:], last=True)
    eng.stream_begin(4, 64)
    eng.stream_feed(xs, last=True)
    with pytest.raises(MasrError, match="last piece"):
        eng.stream_feed(xs[:, :4])
    eng.stream_begin(4, 64)
    with pytest.raises(MasrError, match="last piece"):
        eng.stream_ctc_beam(4)                                   # allowed after `last` only
    with pytest.raises(MasrError, match="max_frames"):
        eng.stream_feed(xs[:, :40]), eng.stream_feed(xs[:, :40])
    eng.set_chunk(None)
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_feed(xs[:, :8])
    with pytest.raises(MasrError, match="chunk"):
        eng.stream_begin(4, 64)                                  # the policy is off
    with pytest.raises(MasrError, match="CTC head"):
        e2 = MasrEngine(dict(TINY, chunk=dict(size=8)), ODIM)
        e2.stream_begin(4, 64)


@pytest.mark.parametrize("mode", ["stream_ctc_greedy", "stream_ctc_beam"])
def test_tester_runs_the_stream_modes(tmp_path, monkeypatch, mode):
    from masr_amd.tester import Tester
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "greedy", {"beam_size": 4}, hybrid=True)
    t.paras.decode_mode, t.paras.decode_suffix, t.paras.decode_chunk, t.paras.decode_left = mode, f"{mode}_decode", 8, -1
    t = Tester(t.config, t.paras, {"af": "african", "au": "australia", "ca": "canada"})
    assert t.stream_piece == 32
    t.load_data(); t.set_model(); t.exec()
    assert t.chunk_last == 8
    assert len((log_dir / f"{mode}_decode" / "best-hyp").read_text().splitlines()) == 6
