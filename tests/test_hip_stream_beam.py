"""The resumable CTC prefix beam inside the stream (include/masr.h masr_stream_beam_*) on the GPU, the peaked TINY hybrid model of
decode_util.py: the final result against masr_stream_ctc_beam and among the piece sizes, the partial after every feed against
masr_ctc_beam_search on a clone of the stream's logits with enc_lens = min(klen, emitted), the n-gram LM and the phrase list against their
one-shot searches, the beam's lifecycle and the Tester's mode.  Every equality is bit for bit: both sides run one kernel text on the same
fp32 logits."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_ref  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from masr_amd._cabi import MasrError  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle.make_goldens import TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, joint_state_dict, make_tester  # noqa: E402
from test_hip_stream import engine, same_bits  # noqa: E402
from test_hip_ctc_lm_beam import model_free as lm_search  # noqa: E402
from test_hip_ctc_bias_beam import PHRASES, _arpa, _phrase_file, model_free as bias_search, runner_up_phrases  # noqa: E402

CASES = [([160, 140, 120, 100], 8, -1), ([160, 140, 120, 100], 4, 0), ([150, 97, 64, 41], 8, -1), ([150, 97, 64, 41], 4, 0), ([600, 410], 16, 2)]
LM_W, BONUS, BIAS_W = 0.8, 0.4, 2.0


def P(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def sdj():
    return joint_state_dict(TINY, 7)


@pytest.fixture(scope="module")
def small_lm():
    return NGramLM(3, C_SMALL, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL, 3, 2)))


def equal(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def plain_search(eng, z, enc_lens, K, nbest):
    """masr_ctc_beam_search, run by the test, on device logits [B, cap, ld] -> device (tokens, lens, scores)"""
    L = _cabi.lib()
    B, cap, ld = z.shape
    wb = int(L.masr_ctc_beam_work_bytes(B, cap, C_SMALL, K))
    work = torch.empty(wb, dtype=torch.uint8, device=z.device)
    tok = torch.empty(B, nbest, cap, dtype=torch.int32, device=z.device)
    ln, sc = torch.empty(B, nbest, dtype=torch.int32, device=z.device), torch.empty(B, nbest, device=z.device)
    _cabi.check(L.masr_ctc_beam_search(P(z), ld, P(enc_lens), B, cap, C_SMALL, K, nbest, 0, C_SMALL - 1, P(work), wb, P(tok), P(ln), P(sc), eng.stream()))
    torch.cuda.synchronize()
    return tok, ln, sc


def feeds(xs, il, piece):
    """(piece of xs, valid, last) of every feed"""
    T = xs.shape[1]
    for t0 in range(0, T, piece):
        t1 = min(T, t0 + piece)
        yield xs[:, t0:t1], [max(0, min(int(l), t1) - t0) for l in il.tolist()], t1 == T


def stream_with_beam(eng, xs, il, piece, K, partial=None, open_after=0, **fused):
    """the batch streamed in pieces with the beam opened in front of feed number `open_after` (it runs the frames emitted by then at once);
    partial(emitted) is called after every feed from then on -> the final result of the beam (raw, nbest = K)"""
    B, T = xs.shape[:2]
    eng.stream_begin(B, T)
    for i, (x, valid, last) in enumerate(feeds(xs, il, piece)):
        if i == open_after:
            eng.stream_beam_open(K, **fused)
        emitted = eng.stream_feed(x, valid, last=last)
        if partial is not None and i >= open_after:
            partial(emitted)
    return eng.stream_beam_result(K, raw=True)


@pytest.mark.parametrize("ilens,c,left", CASES)
def test_final_result_and_partials(sdj, ilens, c, left):
    xs, il, _, _ = synth_batch(11, ilens, [3] * len(ilens))
    T = xs.shape[1]
    eng = engine(sdj, c, left, odim=C_SMALL)
    for K in (1, 4):
        finals, n_partials = [], 0
        for piece in (T, 64, 7):
            def partial(emitted):
                nonlocal n_partials
                got = eng.stream_beam_result(K, raw=True)
                z, klen, fr = eng.stream_logits()
                assert fr == emitted
                want = plain_search(eng, z.clone(), torch.clamp(klen, max=emitted), K, K)
                assert equal(got, want), (K, piece, emitted)
                n_partials += 1

            fin = stream_with_beam(eng, xs, il, piece, K, partial)
            assert equal(fin, eng.stream_ctc_beam(K, K, raw=True)), (K, piece)
            assert equal(fin, eng.stream_beam_result(K, raw=True)), (K, piece)      # the one-shot beside it disturbed nothing
            assert (fin[1][:, 0] >= 0).all()
            finals.append(fin)
        assert equal(finals[0], finals[1]) and equal(finals[0], finals[2]), K
        assert n_partials > 3


def test_a_partial_does_not_depend_on_the_audio_behind_it(sdj):
    ilens = [160, 140, 120, 100]
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    B, T = xs.shape[:2]
    eng = engine(sdj, 8, -1, odim=C_SMALL)
    noise = xs.clone()
    noise[:, 96:] = torch.randn(B, T - 96, xs.shape[2], generator=torch.Generator().manual_seed(5))
    runs = []
    for src in (xs, noise):
        seen = []
        fin = stream_with_beam(eng, src, torch.full_like(il, T), 48, 4, lambda e: seen.append((e, [t.clone() for t in eng.stream_beam_result(4, raw=True)])))
        runs.append((seen, fin))
    (a, fa), (b, fb) = runs
    assert [e for e, _ in a] == [e for e, _ in b] and a[1][0] > 0
    for (e, x), (_, y) in zip(a[:2], b[:2]):                        # the feeds that end at input frames 48 and 96
        assert equal(x, y), e
    assert not equal(fa, fb)                                        # the noise did change what came after


def test_lm_and_phrase_list(sdj, small_lm):
    ilens = [160, 140, 120, 100]
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    eng = engine(sdj, 8, -1, odim=C_SMALL)
    K = 8
    phrases = runner_up_phrases(eng.recog_ctc_beam(xs, il, 8, 8), bias_ref.toy_phrases(C_SMALL, 6, 0, 3))
    bias = ContextBias(C_SMALL, phrases)
    plain = None
    for lm, bs in ((None, None), (small_lm, None), (None, bias), (small_lm, bias)):
        fused = dict(lm=lm, lm_w=LM_W, len_bonus=BONUS, bias=bs, bias_w=BIAS_W)
        finals = [stream_with_beam(eng, xs, il, piece, K, **fused) for piece in (64, 7)]
        assert equal(finals[0], finals[1])
        z, klen, _ = eng.stream_logits()
        z, klen = z.clone(), klen.clone()
        if bs is not None:
            want = bias_search(z, klen, C_SMALL, K, K, lm, LM_W, BONUS, bs, BIAS_W)
        elif lm is not None:
            want = lm_search(z, klen, C_SMALL, K, K, lm, LM_W, BONUS)
        else:
            want = plain = plain_search(eng, z, klen, K, K)
        assert len(finals[0]) == len(want) == 3 + (lm is not None or bs is not None) + (bs is not None)
        assert equal(finals[0], want), (lm is not None, bs is not None)
        if plain is not want:
            assert not same_bits(finals[0][2], plain[2])            # the LM / the list is not a no-op on this model
    # the lists as the one-shot decoders return them
    lists, partials = eng.recog_stream(xs, il, 64, K, nbest=2, sync_beam=True, lm=small_lm, lm_w=LM_W, len_bonus=BONUS, bias=bias, bias_w=BIAS_W)
    assert len(lists) == 4 and all(len(u) == 2 and len(u[0]) == 4 for u in lists)
    assert len(partials) == 3 and partials[-1] == [u[0][0] for u in lists]
    # the stable prefix of the partial K-best only grows and ends as a prefix of the final best hypothesis
    B, T = xs.shape[:2]
    eng.stream_begin(B, T)
    eng.stream_beam_open(K)
    before = [[] for _ in range(B)]
    for x, valid, last in feeds(xs, il, 32):
        eng.stream_feed(x, valid, last=last)
        now = [_cabi.stable_prefix(u) for u in eng.stream_beam_result(K)]
        assert all(n[:len(b)] == b for n, b in zip(now, before))
        before = now
    best = [u[0][0] for u in eng.stream_beam_result(1)]
    assert all(h[:len(b)] == b for h, b in zip(best, before))


def test_lifecycle(sdj):
    ilens = [160, 140, 120, 100]
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    B, T = xs.shape[:2]
    eng = engine(sdj, 8, -1, odim=C_SMALL)
    # a stream that never had a beam, before this engine touched the beam API
    g0 = eng.recog_stream(xs, il, 64)
    z0 = eng.stream_logits()[0].clone()
    with pytest.raises(MasrError, match="no open beam"):
        eng.stream_beam_result(1)
    eng.recog_ctc_beam(xs, il, 4)                                # plans the workspace: the stream is over
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_beam_open(4)
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_beam_result(1)
    # opened after two feeds, the beam catches up
    want = stream_with_beam(eng, xs, il, 48, 4)
    late = stream_with_beam(eng, xs, il, 48, 4, open_after=2)
    assert equal(want, late)
    # opened after the last piece, it runs all the frames at once: the final result
    eng.stream_beam_open(4)
    assert equal(eng.stream_beam_result(4, raw=True), want)
    assert equal(eng.stream_beam_result(4, raw=True), eng.stream_ctc_beam(4, 4, raw=True))
    # opened before the first chunk: the empty prefix
    eng.stream_begin(B, T)
    eng.stream_beam_open(4)
    tok, ln, sc = eng.stream_beam_result(1, raw=True)
    assert (ln == 0).all() and (sc == 0).all() and (tok == -1).all()
    # refusals of the open leave the open beam as it was
    eng.recog_stream(xs, il, 48)
    eng.stream_begin(B, T)
    eng.stream_beam_open(4)
    eng.stream_feed(xs[:, :96])
    kept = [t.clone() for t in eng.stream_beam_result(4, raw=True)]
    with pytest.raises(ValueError, match="beam_size"):
        eng.stream_beam_open(65)
    with pytest.raises(MasrError, match="classes"):
        eng.stream_beam_open(4, bias=ContextBias(C_SMALL + 1, [[3, 4]]))
    with pytest.raises(ValueError, match="nbest"):
        eng.stream_beam_result(5)
    assert equal(kept, eng.stream_beam_result(4, raw=True))
    # a masr_recog* call in between ends both
    eng.recog_ctc_beam(xs, il, 4)
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_feed(xs[:, 96:], last=True)
    with pytest.raises(MasrError, match="no open stream"):
        eng.stream_beam_result(1)
    # and a stream without a beam runs as it did before the beam API was touched
    assert eng.recog_stream(xs, il, 64) == g0
    assert same_bits(eng.stream_logits()[0], z0)
    eng.stream_begin(B, T)
    with pytest.raises(MasrError, match="no open beam"):            # a new stream has no beam
        eng.stream_beam_result(1)


def test_tester_writes_what_stream_ctc_beam_writes(tmp_path, monkeypatch):
    from masr_amd.tester import Tester
    hyps = {}
    for mode in ("stream_ctc_beam", "stream_sync_ctc_beam"):
        t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "greedy", {"beam_size": 4}, hybrid=True)
        t.paras.decode_mode, t.paras.decode_suffix, t.paras.decode_chunk, t.paras.decode_left = mode, f"{mode}_decode", 8, -1
        t.paras.lm_model_path = t.paras.context_path = None
        t = Tester(t.config, t.paras, {"af": "african", "au": "australia", "ca": "canada"})
        assert t.stream_piece == 32
        t.load_data(); t.set_model(); t.exec()
        assert t.chunk_last == 8
        hyps[mode] = (log_dir / f"{mode}_decode" / "best-hyp").read_text()
    assert len(hyps["stream_ctc_beam"].splitlines()) == 6
    assert hyps["stream_sync_ctc_beam"] == hyps["stream_ctc_beam"]


@pytest.mark.parametrize("with_lm,with_ctx", [(True, True), (True, False), (False, True)])
def test_tester_with_an_lm_and_a_phrase_list(tmp_path, monkeypatch, with_lm, with_ctx):
    """--lm_model_path / --context_path: best-hyp holds what the engine's recog_stream gives with that LM, that list and the block's weights"""
    from masr_amd.tester import Tester
    from oracle.make_goldens import ODIM
    arpa = str(_arpa(tmp_path)) if with_lm else None
    ctx = _phrase_file(tmp_path, PHRASES) if with_ctx else None
    mode = "stream_sync_ctc_beam"
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "greedy", {"beam_size": 8, "lm_w": 0.6, "len_bonus": -0.2, "bias_w": 2.5}, hybrid=True)
    t.paras.decode_mode, t.paras.decode_suffix, t.paras.decode_chunk, t.paras.decode_left = mode, f"{mode}_decode", 8, -1
    t.paras.lm_model_path, t.paras.context_path = arpa, ctx
    t = Tester(t.config, t.paras, {"af": "african", "au": "australia", "ca": "canada"})
    t.load_data(); t.set_model(); t.exec()
    assert (t.lm_weight, t.len_bonus) == ((0.6, -0.2) if with_lm else (0.0, 0.0)) and t.bias_weight == (2.5 if with_ctx else 0.0)
    lines = (log_dir / f"{mode}_decode" / "best-hyp").read_text().splitlines()
    lm = NGramLM.from_arpa(arpa, t.id2ch) if with_lm else None
    bias = ContextBias(ODIM, PHRASES) if with_ctx else None
    plain, want = [], []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        eng = t.asr_model.engine
        want += [u[0][0] for u in eng.recog_stream(xs, il, t.stream_piece, 8, sync_beam=True, lm=lm, lm_w=t.lm_weight, len_bonus=t.len_bonus, bias=bias,
                                                   bias_w=t.bias_weight)[0]]
        plain += [u[0][0] for u in eng.recog_stream(xs, il, t.stream_piece, 8)]
    assert len(lines) == len(want) == 6
    for line, hyp in zip(lines, want):
        assert line.split("\t")[1].split() == [str(v) for v in hyp], (line, hyp)
    print(f"lm {with_lm} phrases {with_ctx}: {sum(w != p for w, p in zip(want, plain))} of 6 best hypotheses differ from the plain beam's")
