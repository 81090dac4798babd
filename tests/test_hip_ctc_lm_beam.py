"""The LM-fused CTC prefix beam through the models: MasrEngine.recog_ctc_beam_lm / recog_rescore_lm (masr_recog_ctc_beam_lm,
masr_recog_rescore_lm), BlstmEngine.ctc_beam(lm=...) and the Tester's `lm_ctc_beam` / `lm_rescore` modes.

The search itself is pinned by tests/test_hip_ctc_lm_beam_kernel.py; here every model-level call is compared bit for bit with the model-free
search on the logits the call itself produced (the hybrid transformer's head logits in the workspace, the BLSTM's last_logits()), with
recog_ctc_beam at lm_w = 0, and -- for the two-pass decode -- with its own first pass and with rescore_nbest on that pass's lists."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import lm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib, nbest_lists_lm  # noqa: E402
from masr_amd.blstm_engine import BlstmEngine  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle import blstm_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, ODIM, TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, joint_engine, joint_state_dict, make_tester  # noqa: E402

BLSTM_HEAD_SCALE = 30.0                                           # test_hip_ctc_beam_decode.py's: the tiny random model's rows spread
LM_W, BONUS = 0.8, 0.4


def p(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def model_free(logits, enc_lens, Cn, K, nbest, lm, lm_w, bonus):
    """masr_ctc_beam_search_lm on device logits [B, Tp, ld] -> device (tokens, lens, scores, am)"""
    l = lib()
    B, Tp, ld = logits.shape
    dev = logits.device
    nb = int(l.masr_ctc_beam_lm_work_bytes(B, Tp, Cn, K))
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    tok = torch.empty(B, nbest, Tp, dtype=torch.int32, device=dev)
    ln = torch.empty(B, nbest, dtype=torch.int32, device=dev)
    sc, am = torch.empty(B, nbest, device=dev), torch.empty(B, nbest, device=dev)
    rc = l.masr_ctc_beam_search_lm(p(logits), ld, p(enc_lens), B, Tp, Cn, K, nbest, 0, Cn - 1, lm.h, lm_w, bonus, p(work), nb, p(tok), p(ln), p(sc),
                                   p(am), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok, ln, sc, am


@pytest.fixture(scope="module")
def small_lm():
    return NGramLM(3, C_SMALL, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL, 3, 2)))


@pytest.fixture(scope="module")
def hybrid():
    return joint_engine(TINY, joint_state_dict(TINY, 7))


def test_hybrid_ctc_beam_lm_is_the_search_on_its_own_logits(hybrid, small_lm):
    eng = hybrid
    changed = 0
    for K, nbest in ((1, 1), (8, 3), (20, 20)):
        xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
        B, T = xs.shape[0], xs.shape[1]
        got = eng.recog_ctc_beam_lm(xs, il, K, small_lm, LM_W, BONUS, nbest, raw=True)
        logits, lens = eng.last_ctc_beam_logits(B, T, K)
        want = model_free(logits.clone(), lens.clone(), C_SMALL, K, nbest, small_lm, LM_W, BONUS)
        for g, w in zip(got, want):
            assert torch.equal(bits(g), bits(w)), (K, nbest)
        assert (got[1][:, 0] >= 0).all() and torch.isfinite(got[2][:, 0]).all()
        # lm_w = 0, no bonus: recog_ctc_beam, bit for bit
        plain = eng.recog_ctc_beam(xs, il, K, nbest, raw=True)
        zero = eng.recog_ctc_beam_lm(xs, il, K, small_lm, 0.0, 0.0, nbest, raw=True)
        for a, b in zip(plain, zero[:3]):
            assert torch.equal(bits(a), bits(b)), (K, nbest)
        assert torch.equal(bits(zero[3]), bits(zero[2]))
        changed += not torch.equal(got[0].cpu(), plain[0].cpu())
        lists = nbest_lists_lm(*got)
        assert all(0 < t < C_SMALL - 1 for u in lists for hyp, _, _ in u for t in hyp)
    assert changed                                               # the LM is not a no-op on this model


def test_hybrid_rescore_lm_is_rescore_nbest_on_its_first_pass(hybrid, small_lm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    for K, N, att_w, ctc_w in ((8, 4, 0.5, 0.5), (20, 20, 0.7, 0.3), (4, 4, 1.0, 0.0)):
        tok, ln, sc, att, ctc, order = eng.recog_rescore_lm(xs, il, K, small_lm, LM_W, BONUS, N, att_w, ctc_w, raw=True)
        tok1, ln1, sc1, _ = eng.recog_ctc_beam_lm(xs, il, K, small_lm, LM_W, BONUS, N, raw=True)
        o = order.long().cpu()
        for b in range(xs.shape[0]):
            assert sorted(o[b].tolist()) == list(range(N))       # a permutation of the first pass's list
            assert torch.equal(tok.cpu()[b], tok1.cpu()[b][o[b]]) and torch.equal(ln.cpu()[b], ln1.cpu()[b][o[b]])
            assert torch.equal(bits(ctc)[b], bits(sc1)[b][o[b]])  # ctc = the first pass's fused scores, bit for bit
        again = eng.rescore_nbest(xs, il, tok1, ln1, sc1, att_w, ctc_w, raw=True)
        for name, a, b in zip(("tokens", "lens", "scores", "att", "ctc", "order"), (tok, ln, sc, att, ctc, order), again):
            assert torch.equal(bits(a), bits(b)), (K, N, name)


def test_engine_refusals(hybrid, small_lm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_ctc_beam_lm(xs, il, 4, small_lm, w)
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_rescore_lm(xs, il, 4, small_lm, w)
    with pytest.raises(ValueError, match="len_bonus"):
        eng.recog_ctc_beam_lm(xs, il, 4, small_lm, 0.3, float("nan"))
    with pytest.raises(ValueError, match="att_w"):
        eng.recog_rescore_lm(xs, il, 4, small_lm, 0.3, 0.0, None, 0.0, 0.5)
    with pytest.raises(ValueError, match="nbest"):
        eng.recog_ctc_beam_lm(xs, il, 4, small_lm, 0.3, 0.0, 5)
    lm13 = NGramLM(2, C_SMALL + 1, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL + 1, 2, 1)))
    with pytest.raises(MasrError, match="odim"):
        eng.recog_ctc_beam_lm(xs, il, 4, lm13, 0.5)
    with pytest.raises(MasrError, match="odim"):
        eng.recog_rescore_lm(xs, il, 4, lm13, 0.5)
    plain = MasrEngine(TINY, C_SMALL)
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_ctc_beam_lm(xs, il, 4, small_lm, 0.5)
    l = lib()                                                    # the C entry points vet the same before anything is launched
    il64 = torch.as_tensor(il, dtype=torch.int64)
    out = [torch.zeros(3, 4, 12, dtype=torch.int32, device="cuda"), torch.zeros(3, 4, dtype=torch.int32, device="cuda"),
           torch.zeros(3, 4, device="cuda"), torch.zeros(3, 4, device="cuda")]
    xd = xs.cuda().float().contiguous()
    for w, b, msg in ((-1.0, 0.0, b"lm_w"), (float("nan"), 0.0, b"lm_w"), (0.3, float("inf"), b"len_bonus")):
        assert l.masr_recog_ctc_beam_lm(eng.h, small_lm.h, p(xd), C.c_void_p(il64.data_ptr()), 3, 48, 4, 4, w, b, *[p(t) for t in out], None) == -1
        assert msg in l.masr_last_error()
    assert l.masr_recog_ctc_beam_lm(eng.h, None, p(xd), C.c_void_p(il64.data_ptr()), 3, 48, 4, 4, 0.3, 0.0, *[p(t) for t in out], None) == -1
    assert b"null language model" in l.masr_last_error()


def _blstm_sd():
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    sd["head.weight"] = sd["head.weight"] * BLSTM_HEAD_SCALE
    return sd


def _arpa(tmp_path, seed=5):
    m10 = lm_ref.toy_lm_log10(ODIM, 3, seed, n_sent=120, max_len=10, active=40)
    path = tmp_path / "toy.arpa"
    path.write_text(lm_ref.arpa_text(m10, lm_ref.units(ODIM)))
    return path


def test_blstm_ctc_beam_lm_is_the_search_on_last_logits():
    eng = BlstmEngine(BLSTM_TINY, ODIM)
    eng.load_state_dict(_blstm_sd())
    lm = NGramLM(3, ODIM, *lm_ref.to_arrays(lm_ref.toy_lm(ODIM, 3, 5, n_sent=120, max_len=10, active=40)))
    xs, il, _, _ = synth_batch(22, [57, 57, 44, 12], [3] * 4)
    for K, nbest in ((1, 1), (8, 3)):
        got = eng.ctc_beam(xs, il, K, nbest, lm=lm, lm_w=LM_W, len_bonus=BONUS)
        logits, lens = eng.last_logits()
        want = nbest_lists_lm(*model_free(logits.contiguous(), lens, ODIM, K, nbest, lm, LM_W, BONUS))
        assert got == want and all(len(u) >= 1 and len(u[0]) == 3 for u in got)
        assert all(0 < t < ODIM - 1 for u in got for hyp, _, _ in u for t in hyp)
        zero = eng.ctc_beam(xs, il, K, nbest, lm=lm, lm_w=0.0, len_bonus=0.0)
        assert [[(h, s) for h, s, _ in u] for u in zero] == eng.ctc_beam(xs, il, K, nbest)
    with pytest.raises(ValueError, match="lm_w"):
        eng.ctc_beam(xs, il, 4, lm=lm, lm_w=-1.0)
    with pytest.raises(ValueError, match="len_bonus"):
        eng.ctc_beam(xs, il, 4, lm=lm, lm_w=0.3, len_bonus=float("inf"))
    with pytest.raises(MasrError, match="blank must be 0"):
        eng.ctc_beam(xs, il, 4, blank=1, lm=lm, lm_w=0.3)


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


def test_tester_blstm_lm_ctc_beam(tmp_path, monkeypatch):
    arpa = str(_arpa(tmp_path))
    bd = {"beam_size": 8, "lm_w": 0.6, "len_bonus": 0.5}
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "lm_ctc_beam", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = arpa
    _run(t)
    lines = _lines(log_dir, "lm_ctc_beam")
    assert t.lm.order == 3 and t.lm_weight == 0.6 and t.len_bonus == 0.5
    lm = NGramLM.from_arpa(arpa, t.id2ch, 0, ODIM - 1)
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        want += [_fmt(y, n[0][0]) for n, y in zip(t.asr_model.ctc_beam_decode(xs, il, 8, 1, lm, 0.6, 0.5), ys)]
    assert lines == want
    first = t.lm
    t._lm_ctc_settings()                                         # the LM is built once per Tester
    assert t.lm is first
    # the BLSTM has no decoder to rescore with; settings are vetted before anything is decoded
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_rescore", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = arpa
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="BLSTM has none"):
        t.exec()
    for block, exc, pat in (({"beam_size": 8, "lm_w": -1}, ValueError, "lm_w"), ({"beam_size": 8, "lm_w": float("nan")}, ValueError, "lm_w"),
                            ({"beam_size": 8, "len_bonus": float("inf")}, ValueError, "len_bonus"), ({"beam_size": 65}, ValueError, r"\[1, 64\]"),
                            (None, ValueError, "beam_decode")):
        t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "lm_ctc_beam", block, blstm_sd=_blstm_sd(), bs=4)
        t.paras.lm_model_path = arpa
        t.load_data(); t.set_model()
        with pytest.raises(exc, match=pat):
            t.exec()
        assert not (log_dir / "lm_ctc_beam_decode" / "best-hyp").exists()
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_ctc_beam", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = None
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="no language model given; pass --lm_model_path"):
        t.exec()


def test_tester_transformer_lm_modes(tmp_path, monkeypatch):
    arpa = str(_arpa(tmp_path))

    def tester(mode, block, hybrid=True, path=arpa):
        t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, mode, block, hybrid=hybrid, bs=4)
        t.paras.lm_model_path = path
        return t, log_dir, sd, cfg

    bd = {"beam_size": 8, "nbest": 4, "lm_w": 0.6, "len_bonus": -0.2, "ctc_w": 0.4}
    for mode in ("lm_ctc_beam", "lm_rescore"):
        t, log_dir, sd, cfg = tester(mode, bd)
        _run(t)
        lines = _lines(log_dir, mode)
        lm = NGramLM.from_arpa(arpa, t.id2ch)
        want = []
        for idxs in t.eval_set.iter_indices():
            xs, il, ys, _ = t.eval_set.materialize(idxs)
            if mode == "lm_ctc_beam":
                lists = t.asr_model.engine.recog_ctc_beam_lm(xs, il, 8, lm, 0.6, -0.2)
            else:
                lists = t.asr_model.engine.recog_rescore_lm(xs, il, 8, lm, 0.6, -0.2, 4, 0.6, 0.4)
                assert t.nbest == 4 and t.ctc_weight == 0.4 and abs(t.att_weight - 0.6) < 1e-12
            want += [_fmt(y, n[0][0]) for n, y in zip(lists, ys)]
        assert lines == want, mode
        # a plain transformer has no CTC output layer
        t, _, _, _ = tester(mode, bd, hybrid=False)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match="needs a CTC output layer"):
            t.exec()
        t, _, _, _ = tester(mode, bd, path=None)
        t.load_data(); t.set_model()
        with pytest.raises(NotImplementedError, match="no language model given; pass --lm_model_path"):
            t.exec()
        for block, pat in (({"beam_size": 8, "lm_w": -0.5}, "lm_w"), ({"beam_size": 8, "lm_w": float("inf")}, "lm_w"),
                           ({"beam_size": 8, "len_bonus": float("nan")}, "len_bonus"), ({"beam_size": 0}, r"\[1, 64\]")):
            t, _, _, _ = tester(mode, block)
            t.load_data(); t.set_model()
            with pytest.raises(ValueError, match=pat):
                t.exec()
    # lm_rescore vets nbest and the att / ctc weights as rescore does
    for block, pat in (({"beam_size": 8, "nbest": 9}, "nbest"), ({"beam_size": 8, "ctc_w": 1.0}, "att_w"), ({"beam_size": 8, "ctc_w": -1}, "ctc_w"),
                       ({"beam_size": 8, "att_w": float("nan")}, "att_w")):
        t, _, _, _ = tester("lm_rescore", block)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match=pat):
            t.exec()
