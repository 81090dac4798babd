"""The phrase-biased CTC prefix beam through the models: MasrEngine.recog_ctc_beam_bias / recog_rescore_bias
(masr_recog_ctc_beam_bias, masr_recog_rescore_bias), BlstmEngine.ctc_beam(bias=...) and the Tester's `bias_ctc_beam` / `bias_rescore` modes,
each with and without the n-gram LM.

The search itself is pinned by tests/test_hip_ctc_bias_beam_kernel.py; here every model-level call is compared bit for bit with the model-free
search on the logits the call itself produced (the hybrid transformer's head logits in the workspace, the BLSTM's last_logits()), with the
unbiased calls at bias_w = 0, and -- for the two-pass decode -- with its own first pass and with rescore_nbest on that pass's lists."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_ref  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib, nbest_lists_bias  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402
from masr_amd.blstm_engine import BlstmEngine  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle import blstm_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, ODIM, TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, joint_engine, joint_state_dict, make_tester  # noqa: E402

BLSTM_HEAD_SCALE = 30.0                                           # test_hip_ctc_beam_decode.py's: the tiny random model's rows spread
LM_W, BONUS, BIAS_W = 0.8, 0.4, 2.0


def p(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def model_free(logits, enc_lens, Cn, K, nbest, lm, lm_w, bonus, bias, bias_w):
    """masr_ctc_beam_search_bias on device logits [B, Tp, ld] -> device (tokens, lens, scores, am, nbias)"""
    l = lib()
    B, Tp, ld = logits.shape
    dev = logits.device
    nb = int(l.masr_ctc_beam_bias_work_bytes(B, Tp, Cn, K))
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    tok = torch.empty(B, nbest, Tp, dtype=torch.int32, device=dev)
    ln, nbias = torch.empty(B, nbest, dtype=torch.int32, device=dev), torch.empty(B, nbest, dtype=torch.int32, device=dev)
    sc, am = torch.empty(B, nbest, device=dev), torch.empty(B, nbest, device=dev)
    rc = l.masr_ctc_beam_search_bias(p(logits), ld, p(enc_lens), B, Tp, Cn, K, nbest, 0, Cn - 1, lm.h if lm is not None else None, lm_w, bonus, bias.h,
                                     bias_w, p(work), nb, p(tok), p(ln), p(sc), p(am), p(nbias), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok, ln, sc, am, nbias


@pytest.fixture(scope="module")
def small_lm():
    return NGramLM(3, C_SMALL, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL, 3, 2)))


@pytest.fixture(scope="module")
def hybrid():
    return joint_engine(TINY, joint_state_dict(TINY, 7))


def runner_up_phrases(lists, extra):
    """the hypotheses behind the best one of every utterance as phrases (cut to 64 tokens), and a few more"""
    seen, out = set(), []
    for ph in [h[:64] for u in lists for h, *_ in u[1:]] + extra:
        if ph and tuple(ph) not in seen:
            seen.add(tuple(ph))
            out.append(list(ph))
    return out


def test_hybrid_ctc_beam_bias_is_the_search_on_its_own_logits(hybrid, small_lm):
    eng = hybrid
    xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
    B, T = xs.shape[0], xs.shape[1]
    phrases = runner_up_phrases(eng.recog_ctc_beam(xs, il, 8, 8), bias_ref.toy_phrases(C_SMALL, 6, 0, 3))
    bias, trie = ContextBias(C_SMALL, phrases), bias_ref.build(phrases)
    changed = 0
    for lm in (None, small_lm):
        for K, nbest in ((1, 1), (8, 3), (20, 20)):
            got = eng.recog_ctc_beam_bias(xs, il, K, bias, BIAS_W, lm, LM_W, BONUS, nbest, raw=True)
            logits, lens = eng.last_ctc_beam_logits(B, T, K)
            want = model_free(logits.clone(), lens.clone(), C_SMALL, K, nbest, lm, LM_W, BONUS, bias, BIAS_W)
            for g, w in zip(got, want):
                assert torch.equal(bits(g), bits(w)), (K, nbest)
            assert (got[1][:, 0] >= 0).all() and torch.isfinite(got[2][:, 0]).all()
            # bias_w = 0: the unbiased call, bit for bit
            zero = eng.recog_ctc_beam_bias(xs, il, K, bias, 0.0, lm, LM_W, BONUS, nbest, raw=True)
            plain = eng.recog_ctc_beam(xs, il, K, nbest, raw=True) if lm is None else eng.recog_ctc_beam_lm(xs, il, K, lm, LM_W, BONUS, nbest, raw=True)
            for a, b in zip(plain, zero):
                assert torch.equal(bits(a), bits(b)), (K, nbest)
            changed += not torch.equal(got[0].cpu(), plain[0].cpu())
            lists = nbest_lists_bias(*got)
            assert all(0 < t < C_SMALL - 1 for u in lists for hyp, *_ in u for t in hyp)
            assert all(n == bias_ref.count(trie, hyp) for u in lists for hyp, _, _, n in u)
    assert changed                                               # the phrase list is not a no-op on this model


def test_hybrid_rescore_bias_is_rescore_nbest_on_its_first_pass(hybrid, small_lm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    bias = ContextBias(C_SMALL, runner_up_phrases(eng.recog_ctc_beam(xs, il, 8, 8), [[3, 4], [5]]))
    for lm in (None, small_lm):
        for K, N, att_w, ctc_w in ((8, 4, 0.5, 0.5), (20, 20, 0.7, 0.3), (4, 4, 1.0, 0.0)):
            tok, ln, sc, att, ctc, order = eng.recog_rescore_bias(xs, il, K, bias, BIAS_W, lm, LM_W, BONUS, N, att_w, ctc_w, raw=True)
            tok1, ln1, sc1, _, _ = eng.recog_ctc_beam_bias(xs, il, K, bias, BIAS_W, lm, LM_W, BONUS, N, raw=True)
            o = order.long().cpu()
            for b in range(xs.shape[0]):
                assert sorted(o[b].tolist()) == list(range(N))       # a permutation of the first pass's list
                assert torch.equal(tok.cpu()[b], tok1.cpu()[b][o[b]]) and torch.equal(ln.cpu()[b], ln1.cpu()[b][o[b]])
                assert torch.equal(bits(ctc)[b], bits(sc1)[b][o[b]])  # ctc = the first pass's final scores, bit for bit
            again = eng.rescore_nbest(xs, il, tok1, ln1, sc1, att_w, ctc_w, raw=True)
            for name, a, b in zip(("tokens", "lens", "scores", "att", "ctc", "order"), (tok, ln, sc, att, ctc, order), again):
                assert torch.equal(bits(a), bits(b)), (K, N, name)


def test_engine_refusals(hybrid, small_lm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    bias = ContextBias(C_SMALL, [[3, 4], [5]])
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bias_w"):
            eng.recog_ctc_beam_bias(xs, il, 4, bias, w)
        with pytest.raises(ValueError, match="bias_w"):
            eng.recog_rescore_bias(xs, il, 4, bias, w)
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_ctc_beam_bias(xs, il, 4, bias, 1.0, small_lm, w)
    with pytest.raises(ValueError, match="live ContextBias"):
        eng.recog_ctc_beam_bias(xs, il, 4, None, 1.0)
    with pytest.raises(ValueError, match="len_bonus"):
        eng.recog_ctc_beam_bias(xs, il, 4, bias, 1.0, small_lm, 0.3, float("nan"))
    with pytest.raises(ValueError, match="att_w"):
        eng.recog_rescore_bias(xs, il, 4, bias, 1.0, None, 0.3, 0.0, None, 0.0, 0.5)
    with pytest.raises(ValueError, match="nbest"):
        eng.recog_ctc_beam_bias(xs, il, 4, bias, 1.0, nbest=5)
    bias13 = ContextBias(C_SMALL + 1, [[3, 4]])
    with pytest.raises(MasrError, match="phrase list's classes differ from the model's odim"):
        eng.recog_ctc_beam_bias(xs, il, 4, bias13, 1.0)
    with pytest.raises(MasrError, match="phrase list's classes differ from the model's odim"):
        eng.recog_rescore_bias(xs, il, 4, bias13, 1.0)
    lm13 = NGramLM(2, C_SMALL + 1, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL + 1, 2, 1)))
    with pytest.raises(MasrError, match="language model's classes differ from the model's odim"):
        eng.recog_ctc_beam_bias(xs, il, 4, bias, 1.0, lm13, 0.5)
    plain = MasrEngine(TINY, C_SMALL)
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_ctc_beam_bias(xs, il, 4, bias, 1.0)
    closed = ContextBias(C_SMALL, [[3]])
    closed.close()
    with pytest.raises(ValueError, match="live ContextBias"):
        eng.recog_ctc_beam_bias(xs, il, 4, closed, 1.0)
    l = lib()                                                    # the C entry points vet the same before anything is launched
    il64 = torch.as_tensor(il, dtype=torch.int64)
    out = [torch.full((3, 4, 12), 77, dtype=torch.int32, device="cuda"), torch.full((3, 4), 77, dtype=torch.int32, device="cuda"),
           torch.full((3, 4), 77.0, device="cuda"), torch.full((3, 4), 77.0, device="cuda"), torch.full((3, 4), 77, dtype=torch.int32, device="cuda")]
    xd = xs.cuda().float().contiguous()

    def call(lm=None, b=bias.h, lm_w=0.3, bonus=0.0, bias_w=1.0, outs=None):
        return l.masr_recog_ctc_beam_bias(eng.h, lm, b, p(xd), C.c_void_p(il64.data_ptr()), 3, 48, 4, 4, lm_w, bonus, bias_w,
                                          *(outs or [p(t) for t in out]), None)
    for kw, msg in ((dict(bias_w=-1.0), b"bias_w must be finite and >= 0"), (dict(bias_w=float("nan")), b"bias_w must be finite and >= 0"),
                    (dict(b=None), b"null phrase list"), (dict(b=bias13.h), b"phrase list's classes differ"),
                    (dict(lm=small_lm.h, lm_w=-1.0), b"lm_w"), (dict(lm=small_lm.h, bonus=float("inf")), b"len_bonus"),
                    (dict(outs=[p(t) for t in out[:4]] + [None]), b"null pointer"), (dict(outs=[p(t) for t in out[:3]] + [None, p(out[4])]), b"null pointer")):
        assert call(**kw) == -1, kw
        assert msg in l.masr_last_error(), (kw, l.masr_last_error())
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out)
    assert call(lm_w=-1.0, bonus=float("nan")) == 0              # without an LM its weights are ignored
    torch.cuda.synchronize()
    assert (out[1][:, 0] >= 0).all() and (out[4][:, 0] >= 0).all()


def _blstm_sd():
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    sd["head.weight"] = sd["head.weight"] * BLSTM_HEAD_SCALE
    return sd


def _arpa(tmp_path, seed=5):
    m10 = lm_ref.toy_lm_log10(ODIM, 3, seed, n_sent=120, max_len=10, active=40)
    path = tmp_path / "toy.arpa"
    path.write_text(lm_ref.arpa_text(m10, lm_ref.units(ODIM)))
    return path


def _phrase_file(tmp_path, phrases):
    path = tmp_path / "phrases.txt"
    path.write_text("\n".join(" ".join(str(t) for t in ph) for ph in phrases[:len(phrases) // 2]) + "\n\n" +
                    "\n".join(" ".join(str(t) for t in ph) for ph in phrases[len(phrases) // 2:]) + "\n")
    return str(path)


def test_blstm_ctc_beam_bias_is_the_search_on_last_logits():
    eng = BlstmEngine(BLSTM_TINY, ODIM)
    eng.load_state_dict(_blstm_sd())
    lm = NGramLM(3, ODIM, *lm_ref.to_arrays(lm_ref.toy_lm(ODIM, 3, 5, n_sent=120, max_len=10, active=40)))
    xs, il, _, _ = synth_batch(22, [57, 57, 44, 12], [3] * 4)
    phrases = runner_up_phrases(eng.ctc_beam(xs, il, 8, 8), bias_ref.toy_phrases(ODIM, 20, 1, 4))
    bias, trie = ContextBias(ODIM, phrases), bias_ref.build(phrases)
    changed = 0
    for use_lm in (None, lm):
        kw = {} if use_lm is None else dict(lm=use_lm, lm_w=LM_W, len_bonus=BONUS)
        for K, nbest in ((1, 1), (8, 3)):
            got = eng.ctc_beam(xs, il, K, nbest, bias=bias, bias_w=BIAS_W, **kw)
            logits, lens = eng.last_logits()
            want = nbest_lists_bias(*model_free(logits.contiguous(), lens, ODIM, K, nbest, use_lm, LM_W, BONUS, bias, BIAS_W))
            assert got == want and all(len(u) >= 1 and len(u[0]) == 4 for u in got)
            assert all(0 < t < ODIM - 1 for u in got for hyp, *_ in u for t in hyp)
            assert all(n == bias_ref.count(trie, hyp) and isinstance(n, int) for u in got for hyp, _, _, n in u)
            zero = eng.ctc_beam(xs, il, K, nbest, bias=bias, bias_w=0.0, **kw)
            plain = eng.ctc_beam(xs, il, K, nbest, **kw)           # bias None: today's behaviour
            assert [[e[:len(q)] for e, q in zip(u, v)] for u, v in zip(zero, plain)] == plain
            changed += [u[0][0] for u in got] != [u[0][0] for u in plain]
    assert changed
    with pytest.raises(ValueError, match="bias_w"):
        eng.ctc_beam(xs, il, 4, bias=bias, bias_w=-1.0)
    with pytest.raises(ValueError, match="live ContextBias"):
        eng.ctc_beam(xs, il, 4, bias="phrases", bias_w=1.0)
    with pytest.raises(MasrError, match="blank must be 0 with a phrase list"):
        eng.ctc_beam(xs, il, 4, blank=1, bias=bias, bias_w=1.0)


def _run(t):
    t.load_data(); t.set_model(); t.exec()


def _lines(log_dir, mode):
    lines = (log_dir / f"{mode}_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6 and all("\t" in l for l in lines)
    for l in lines:
        assert all(0 < int(x) < ODIM - 1 for x in l.split("\t")[1].split())
    return lines


def _fmt(y, hyp):
    return "{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(str(v) for v in hyp))


PHRASES = bias_ref.toy_phrases(ODIM, 40, 2, 4)


@pytest.mark.parametrize("with_lm", [False, True])
def test_tester_blstm_bias_ctc_beam(tmp_path, monkeypatch, with_lm):
    arpa = str(_arpa(tmp_path)) if with_lm else None
    ctx = _phrase_file(tmp_path, PHRASES)
    bd = {"beam_size": 8, "lm_w": 0.6, "len_bonus": 0.5, "bias_w": 2.5}
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "bias_ctc_beam", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path, t.paras.context_path = arpa, ctx
    _run(t)
    lines = _lines(log_dir, "bias_ctc_beam")
    assert t.bias.phrases == len(PHRASES) and t.bias_weight == 2.5
    assert (t.lm.order == 3 and t.lm_weight == 0.6 and t.len_bonus == 0.5) if with_lm else (t.lm is None and t.lm_weight == 0.0 and t.len_bonus == 0.0)
    lm = NGramLM.from_arpa(arpa, t.id2ch, 0, ODIM - 1) if with_lm else None
    bias = ContextBias(ODIM, PHRASES)
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        lists = t.asr_model.ctc_beam_decode(xs, il, 8, 1, lm, 0.6 if with_lm else 0.0, 0.5 if with_lm else 0.0, bias=bias, bias_weight=2.5)
        want += [_fmt(y, n[0][0]) for n, y in zip(lists, ys)]
    assert lines == want
    first = t.bias
    t._bias_ctc_settings()                                       # the phrase list is built once per Tester
    assert t.bias is first
    if with_lm:
        return
    # the BLSTM has no decoder to rescore with; settings are vetted before anything is decoded
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "bias_rescore", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path, t.paras.context_path = None, ctx
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="BLSTM has none"):
        t.exec()
    bad_file = tmp_path / "bad.txt"
    bad_file.write_text("3 4\n5 999\n")
    for block, path, exc, pat in (({"beam_size": 8, "bias_w": -1}, ctx, ValueError, "bias_w"), ({"beam_size": 65}, ctx, ValueError, r"\[1, 64\]"),
                                  (None, ctx, ValueError, "beam_decode"), (bd, None, NotImplementedError, "no phrase list given; pass --context_path"),
                                  (bd, str(bad_file), ValueError, r"bad\.txt:2: unit ids must lie in")):
        t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "bias_ctc_beam", block, blstm_sd=_blstm_sd(), bs=4)
        t.paras.lm_model_path, t.paras.context_path = None, path
        t.load_data(); t.set_model()
        with pytest.raises(exc, match=pat):
            t.exec()
        assert not (log_dir / "bias_ctc_beam_decode" / "best-hyp").exists()


@pytest.mark.parametrize("with_lm", [False, True])
def test_tester_transformer_bias_modes(tmp_path, monkeypatch, with_lm):
    arpa = str(_arpa(tmp_path)) if with_lm else None
    ctx = _phrase_file(tmp_path, PHRASES)

    def tester(mode, block, hybrid=True, path=ctx):
        t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, mode, block, hybrid=hybrid, bs=4)
        t.paras.lm_model_path, t.paras.context_path = arpa, path
        return t, log_dir, sd, cfg

    bd = {"beam_size": 8, "nbest": 4, "lm_w": 0.6, "len_bonus": -0.2, "ctc_w": 0.4, "bias_w": 2.5}
    lm_w, bonus = (0.6, -0.2) if with_lm else (0.0, 0.0)
    for mode in ("bias_ctc_beam", "bias_rescore"):
        t, log_dir, sd, cfg = tester(mode, bd)
        _run(t)
        lines = _lines(log_dir, mode)
        lm = NGramLM.from_arpa(arpa, t.id2ch) if with_lm else None
        bias = ContextBias(ODIM, PHRASES)
        want = []
        for idxs in t.eval_set.iter_indices():
            xs, il, ys, _ = t.eval_set.materialize(idxs)
            if mode == "bias_ctc_beam":
                lists = t.asr_model.engine.recog_ctc_beam_bias(xs, il, 8, bias, 2.5, lm, lm_w, bonus)
            else:
                lists = t.asr_model.engine.recog_rescore_bias(xs, il, 8, bias, 2.5, lm, lm_w, bonus, 4, 0.6, 0.4)
                assert t.nbest == 4 and t.ctc_weight == 0.4 and abs(t.att_weight - 0.6) < 1e-12
            want += [_fmt(y, n[0][0]) for n, y in zip(lists, ys)]
        assert lines == want, mode
        if with_lm:
            continue
        # a plain transformer has no CTC output layer
        t, _, _, _ = tester(mode, bd, hybrid=False)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match="needs a CTC output layer"):
            t.exec()
        t, _, _, _ = tester(mode, bd, path=None)
        t.load_data(); t.set_model()
        with pytest.raises(NotImplementedError, match="no phrase list given; pass --context_path"):
            t.exec()
        for block, pat in (({"beam_size": 8, "bias_w": -0.5}, "bias_w"), ({"beam_size": 8, "bias_w": float("inf")}, "bias_w"), ({"beam_size": 0}, r"\[1, 64\]")):
            t, _, _, _ = tester(mode, block)
            t.load_data(); t.set_model()
            with pytest.raises(ValueError, match=pat):
                t.exec()
    if not with_lm:
        # bias_rescore vets nbest and the att / ctc weights as rescore does
        for block, pat in (({"beam_size": 8, "nbest": 9}, "nbest"), ({"beam_size": 8, "ctc_w": 1.0}, "att_w"), ({"beam_size": 8, "ctc_w": -1}, "ctc_w")):
            t, _, _, _ = tester("bias_rescore", block)
            t.load_data(); t.set_model()
            with pytest.raises(ValueError, match=pat):
                t.exec()
