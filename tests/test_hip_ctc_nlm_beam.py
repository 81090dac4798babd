"""The CTC prefix beam with the LSTM LM through the models: MasrEngine.recog_ctc_beam_nlm / recog_rescore_nlm
(masr_recog_ctc_beam_nlm, masr_recog_rescore_nlm), BlstmEngine.ctc_beam(lm=an LstmLM) and the Tester's `nlm_ctc_beam` / `nlm_rescore` modes.

The search itself is pinned by tests/test_hip_ctc_nlm_beam_kernel.py; here every model-level call is compared bit for bit with the model-free
search on the logits the call itself produced (the hybrid transformer's head logits in the workspace, the BLSTM's last_logits()), with the
n-gram search at lm_w = 0, and -- for the two-pass decode -- with its own first pass and with rescore_nbest on that pass's lists.  The model
paths replay one captured frame per encoder frame: repeated calls on a side stream that change the weights, K and the LM must give what a
fresh engine gives with direct launches."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import lm_ref  # noqa: E402
import nlm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib, nbest_lists_lm  # noqa: E402
from masr_amd.blstm_engine import BlstmEngine  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from masr_amd.nlm import LstmLM  # noqa: E402
from oracle import blstm_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, ODIM, TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, joint_engine, joint_state_dict, make_tester  # noqa: E402

BLSTM_HEAD_SCALE = 30.0                                           # test_hip_ctc_beam_decode.py's: the tiny random model's rows spread
LM_W, BONUS = 0.8, 0.4


def p(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def make_nlm(Cn=C_SMALL, seed=3, dims=(16, 24, 2)):
    return LstmLM.from_state_dict(nlm_ref.to_state_dict(nlm_ref.toy_nlm(Cn, *dims, seed)))


def model_free(logits, enc_lens, Cn, K, nbest, nlm, lm_w, bonus):
    """masr_ctc_beam_search_nlm on device logits [B, Tp, ld] -> device (tokens, lens, scores, am)"""
    l = lib()
    B, Tp, ld = logits.shape
    dev = logits.device
    nb = int(l.masr_ctc_beam_nlm_work_bytes(nlm.h, B, Tp, Cn, K))
    assert nb > 0, l.masr_last_error()
    work = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev)
    tok = torch.empty(B, nbest, Tp, dtype=torch.int32, device=dev)
    ln = torch.empty(B, nbest, dtype=torch.int32, device=dev)
    sc, am = torch.empty(B, nbest, device=dev), torch.empty(B, nbest, device=dev)
    rc = l.masr_ctc_beam_search_nlm(p(logits), ld, p(enc_lens), B, Tp, Cn, K, nbest, 0, Cn - 1, nlm.h, lm_w, bonus, p(work), nb, p(tok), p(ln), p(sc),
                                    p(am), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return tok, ln, sc, am


@pytest.fixture(scope="module")
def small_nlm():
    return make_nlm()


@pytest.fixture(scope="module")
def hybrid():
    return joint_engine(TINY, joint_state_dict(TINY, 7))


def test_hybrid_ctc_beam_nlm_is_the_search_on_its_own_logits(hybrid, small_nlm):
    eng = hybrid
    ngram = NGramLM(3, C_SMALL, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL, 3, 2)))
    changed = 0
    for K, nbest in ((1, 1), (8, 3), (20, 20)):
        xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
        B, T = xs.shape[0], xs.shape[1]
        got = eng.recog_ctc_beam_nlm(xs, il, K, small_nlm, LM_W, BONUS, nbest, raw=True)
        logits, lens = eng.last_ctc_beam_logits(B, T, K)
        want = model_free(logits.clone(), lens.clone(), C_SMALL, K, nbest, small_nlm, LM_W, BONUS)
        for g, w in zip(got, want):
            assert torch.equal(bits(g), bits(w)), (K, nbest)
        assert (got[1][:, 0] >= 0).all() and torch.isfinite(got[2][:, 0]).all()
        # lm_w = 0: the n-gram search at lm_w = 0 with the same bonus, and without a bonus recog_ctc_beam, bit for bit
        zero_b = eng.recog_ctc_beam_nlm(xs, il, K, small_nlm, 0.0, BONUS, nbest, raw=True)
        for a, b in zip(eng.recog_ctc_beam_lm(xs, il, K, ngram, 0.0, BONUS, nbest, raw=True), zero_b):
            assert torch.equal(bits(a), bits(b)), (K, nbest)
        plain = eng.recog_ctc_beam(xs, il, K, nbest, raw=True)
        zero = eng.recog_ctc_beam_nlm(xs, il, K, small_nlm, 0.0, 0.0, nbest, raw=True)
        for a, b in zip(plain, zero[:3]):
            assert torch.equal(bits(a), bits(b)), (K, nbest)
        assert torch.equal(bits(zero[3]), bits(zero[2]))
        changed += not torch.equal(got[0].cpu(), plain[0].cpu())
        lists = nbest_lists_lm(*got)
        assert all(0 < t < C_SMALL - 1 for u in lists for hyp, _, _ in u for t in hyp)
    assert changed                                               # the LM is not a no-op on this model


def test_hybrid_rescore_nlm_is_rescore_nbest_on_its_first_pass(hybrid, small_nlm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    for K, N, att_w, ctc_w in ((8, 4, 0.5, 0.5), (20, 20, 0.7, 0.3), (4, 4, 1.0, 0.0)):
        tok, ln, sc, att, ctc, order = eng.recog_rescore_nlm(xs, il, K, small_nlm, LM_W, BONUS, N, att_w, ctc_w, raw=True)
        tok1, ln1, sc1, _ = eng.recog_ctc_beam_nlm(xs, il, K, small_nlm, LM_W, BONUS, N, raw=True)
        o = order.long().cpu()
        for b in range(xs.shape[0]):
            assert sorted(o[b].tolist()) == list(range(N))       # a permutation of the first pass's list
            assert torch.equal(tok.cpu()[b], tok1.cpu()[b][o[b]]) and torch.equal(ln.cpu()[b], ln1.cpu()[b][o[b]])
            assert torch.equal(bits(ctc)[b], bits(sc1)[b][o[b]])  # ctc = the first pass's fused scores, bit for bit
        again = eng.rescore_nbest(xs, il, tok1, ln1, sc1, att_w, ctc_w, raw=True)
        for name, a, b in zip(("tokens", "lens", "scores", "att", "ctc", "order"), (tok, ln, sc, att, ctc, order), again):
            assert torch.equal(bits(a), bits(b)), (K, N, name)


def test_repeated_calls_never_replay_stale_values():
    """one engine on a side stream (the frame graph is captured and replayed there): calls that change lm_w, len_bonus, K, nbest and the LM -- one
    LM destroyed and another (one layer, another seed) created, possibly at its address -- and that alternate between the one-pass and the
    two-pass plan give what a fresh engine gives on the default stream (direct launches)"""
    sd = joint_state_dict(TINY, 7)
    xs, il, _, _ = synth_batch(11, [64, 52, 40, 33], [3] * 4)
    seq = [(8, 3, 0.8, 0.4), (8, 3, 0.2, 0.4), (8, 3, 0.2, -0.3), (4, 4, 0.2, -0.3), (8, 8, 0.8, 0.4), (8, 3, 0.8, 0.4)]

    def decode(e, lm, s):
        K, N, w, b = s
        return [t.cpu().clone() for t in e.recog_ctc_beam_nlm(xs, il, K, lm, w, b, N, raw=True)]

    def rescore(e, lm, s):
        K, N, w, b = s
        return [t.cpu().clone() for t in e.recog_rescore_nlm(xs, il, K, lm, w, b, N, 0.6, 0.4, raw=True)]

    lm1 = make_nlm(seed=3)
    ref = joint_engine(TINY, sd)
    want = [decode(ref, lm1, s) for s in seq]
    want_rs = rescore(ref, lm1, seq[0])
    e = joint_engine(TINY, sd)
    rescore(e, lm1, (8, 8, 0.8, 0.4))                            # grows the workspace to its final size on the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [decode(e, lm1, s) for s in seq]
        got_rs = rescore(e, lm1, seq[0])
        got_again = decode(e, lm1, seq[0])
        side.synchronize()
        lm1.close()                                              # destroy, then another LM (other shape and values) in its place
        lm2 = make_nlm(seed=4, dims=(16, 24, 1))
        got2 = decode(e, lm2, seq[0])
    side.synchronize()
    want2 = decode(joint_engine(TINY, sd), lm2, seq[0])
    for i, (g, w) in enumerate(zip(got + [got_again], want + [want[0]])):
        for a, b in zip(g, w):
            assert torch.equal(bits(a), bits(b)), i
    for a, b in zip(got_rs, want_rs):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(got2, want2):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(got2[0], got[0][0]) or not torch.equal(bits(got2[2]), bits(got[0][2]))     # the second LM is another LM


def test_engine_refusals(hybrid, small_nlm):
    eng = hybrid
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_ctc_beam_nlm(xs, il, 4, small_nlm, w)
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_rescore_nlm(xs, il, 4, small_nlm, w)
    with pytest.raises(ValueError, match="len_bonus"):
        eng.recog_ctc_beam_nlm(xs, il, 4, small_nlm, 0.3, float("nan"))
    with pytest.raises(ValueError, match="att_w"):
        eng.recog_rescore_nlm(xs, il, 4, small_nlm, 0.3, 0.0, None, 0.0, 0.5)
    with pytest.raises(ValueError, match="nbest"):
        eng.recog_ctc_beam_nlm(xs, il, 4, small_nlm, 0.3, 0.0, 5)
    with pytest.raises(ValueError, match="live LstmLM"):
        eng.recog_ctc_beam_nlm(xs, il, 4, None, 0.3)
    lm13 = make_nlm(C_SMALL + 1, 1, (8, 8, 1))
    with pytest.raises(MasrError, match="odim"):
        eng.recog_ctc_beam_nlm(xs, il, 4, lm13, 0.5)
    with pytest.raises(MasrError, match="odim"):
        eng.recog_rescore_nlm(xs, il, 4, lm13, 0.5)
    plain = MasrEngine(TINY, C_SMALL)
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_ctc_beam_nlm(xs, il, 4, small_nlm, 0.5)
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_rescore_nlm(xs, il, 4, small_nlm, 0.5)
    l = lib()                                                    # the C entry points vet the same before anything is launched
    il64 = torch.as_tensor(il, dtype=torch.int64)
    out = [torch.full((3, 4, 12), 77, dtype=torch.int32, device="cuda"), torch.full((3, 4), 77, dtype=torch.int32, device="cuda"),
           torch.full((3, 4), 77.0, device="cuda"), torch.full((3, 4), 77.0, device="cuda")]
    rs = out + [torch.full((3, 4), 77.0, device="cuda"), torch.full((3, 4), 77, dtype=torch.int32, device="cuda")]
    xd = xs.cuda().float().contiguous()
    ilp = C.c_void_p(il64.data_ptr())
    eng.recog_rescore_nlm(xs, il, 4, small_nlm, 0.3)            # binds a workspace large enough for both calls below
    for lm, w, b, msg in ((small_nlm.h, -1.0, 0.0, b"lm_w"), (small_nlm.h, float("nan"), 0.0, b"lm_w"), (small_nlm.h, 0.3, float("inf"), b"len_bonus"),
                          (None, 0.3, 0.0, b"null language model"), (lm13.h, 0.3, 0.0, b"classes differ from the model's odim")):
        assert l.masr_recog_ctc_beam_nlm(eng.h, lm, p(xd), ilp, 3, 48, 4, 4, w, b, *[p(t) for t in out], None) == -1
        assert msg in l.masr_last_error(), l.masr_last_error()
        assert l.masr_recog_rescore_nlm(eng.h, lm, p(xd), ilp, 3, 48, 4, 4, w, b, 0.5, 0.5, *[p(t) for t in rs], None) == -1
        assert msg in l.masr_last_error(), l.masr_last_error()
    assert l.masr_ctc_beam_nlm_workspace_bytes(eng.h, None, 3, 48, 4) < 0 and b"null language model" in l.masr_last_error()
    assert l.masr_rescore_nlm_workspace_bytes(eng.h, None, 3, 48, 4, 4, 12) < 0 and b"null language model" in l.masr_last_error()
    assert l.masr_ctc_beam_nlm_workspace_bytes(plain.h, small_nlm.h, 3, 48, 4) < 0 and b"no CTC head" in l.masr_last_error()
    assert l.masr_ctc_beam_nlm_workspace_bytes(eng.h, small_nlm.h, 3, 48, 4) > l.masr_ctc_beam_workspace_bytes(eng.h, 3, 48, 4) > 0
    assert l.masr_rescore_nlm_workspace_bytes(eng.h, small_nlm.h, 3, 48, 4, 4, 12) > l.masr_rescore_workspace_bytes(eng.h, 3, 48, 4, 4, 12) > 0
    # a workspace bound for the plain search is too small for this one: -2, nothing launched
    small = joint_engine(TINY, joint_state_dict(TINY, 7))
    need = int(l.masr_ctc_beam_workspace_bytes(small.h, 3, 48, 4))
    small.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert l.masr_bind(small.h, p(small.params), p(small.grads), p(small.pe), p(small.ws), need) == 0
    assert l.masr_recog_ctc_beam_nlm(small.h, small_nlm.h, p(xd), ilp, 3, 48, 4, 4, 0.3, 0.0, *[p(t) for t in out], None) == -2
    assert b"masr_ctc_beam_nlm_workspace_bytes" in l.masr_last_error()
    torch.cuda.synchronize()
    for t in rs:
        assert (t == 77).all()


def _blstm_sd():
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    sd["head.weight"] = sd["head.weight"] * BLSTM_HEAD_SCALE
    return sd


def _checkpoint(tmp_path, C_=ODIM, name="toy_nlm.pt"):
    path = tmp_path / name
    if not path.exists():
        torch.save(nlm_ref.to_state_dict(nlm_ref.toy_nlm(C_, 24, 40, 2, 5)), path)
    return str(path)


def test_blstm_ctc_beam_nlm_is_the_search_on_last_logits():
    eng = BlstmEngine(BLSTM_TINY, ODIM)
    eng.load_state_dict(_blstm_sd())
    nlm = make_nlm(ODIM, 5, (24, 40, 2))
    xs, il, _, _ = synth_batch(22, [57, 57, 44, 12], [3] * 4)
    for K, nbest in ((1, 1), (8, 3)):
        got = eng.ctc_beam(xs, il, K, nbest, lm=nlm, lm_w=LM_W, len_bonus=BONUS)
        logits, lens = eng.last_logits()
        want = nbest_lists_lm(*model_free(logits.contiguous(), lens, ODIM, K, nbest, nlm, LM_W, BONUS))
        assert got == want and all(len(u) >= 1 and len(u[0]) == 3 for u in got)
        assert all(0 < t < ODIM - 1 for u in got for hyp, _, _ in u for t in hyp)
        zero = eng.ctc_beam(xs, il, K, nbest, lm=nlm, lm_w=0.0, len_bonus=0.0)
        assert [[(h, s) for h, s, _ in u] for u in zero] == eng.ctc_beam(xs, il, K, nbest)
    with pytest.raises(ValueError, match="lm_w"):
        eng.ctc_beam(xs, il, 4, lm=nlm, lm_w=-1.0)
    with pytest.raises(ValueError, match="len_bonus"):
        eng.ctc_beam(xs, il, 4, lm=nlm, lm_w=0.3, len_bonus=float("inf"))
    with pytest.raises(MasrError, match="blank must be 0"):
        eng.ctc_beam(xs, il, 4, blank=1, lm=nlm, lm_w=0.3)
    with pytest.raises(MasrError, match="classes differ"):
        eng.ctc_beam(xs, il, 4, lm=make_nlm(C_SMALL), lm_w=0.3)


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


def test_tester_blstm_nlm_ctc_beam(tmp_path, monkeypatch):
    ckpt = _checkpoint(tmp_path)
    bd = {"beam_size": 8, "lm_w": 0.6, "len_bonus": 0.5, "lm_start": "eos"}
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "nlm_ctc_beam", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = ckpt
    _run(t)
    lines = _lines(log_dir, "nlm_ctc_beam")
    assert t.lm_weight == 0.6 and t.len_bonus == 0.5 and t.nlm.start_id == t.eos_id
    nlm = LstmLM.load(ckpt, start_id=t.eos_id)
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        want += [_fmt(y, n[0][0]) for n, y in zip(t.asr_model.ctc_beam_decode(xs, il, 8, 1, nlm, 0.6, 0.5), ys)]
    assert lines == want
    first = t.nlm
    t._nlm_ctc_settings()                                        # the LM is built once per Tester
    assert t.nlm is first
    # the BLSTM has no decoder to rescore with; settings are vetted before anything is decoded
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "nlm_rescore", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = ckpt
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="BLSTM has none"):
        t.exec()
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "nlm_ctc_beam", bd, blstm_sd=_blstm_sd(), bs=4)
    t.paras.lm_model_path = _checkpoint(tmp_path, ODIM + 1, "wide.pt")     # (the BLSTM's sos = eos = ODIM - 1 is a class of this LM)
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match=f"the LSTM LM has {ODIM + 1} classes, the model {ODIM} output units"):
        t.exec()
    assert not (log_dir / "nlm_ctc_beam_decode" / "best-hyp").exists()


def test_tester_transformer_nlm_modes(tmp_path, monkeypatch):
    ckpt = _checkpoint(tmp_path)

    def tester(mode, block, hybrid=True, path=ckpt):
        t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, mode, block, hybrid=hybrid, bs=4)
        t.paras.lm_model_path = path
        return t, log_dir, sd, cfg

    bd = {"beam_size": 8, "nbest": 4, "lm_w": 0.6, "len_bonus": -0.2, "ctc_w": 0.4}
    for mode in ("nlm_ctc_beam", "nlm_rescore"):
        t, log_dir, sd, cfg = tester(mode, bd)
        _run(t)
        lines = _lines(log_dir, mode)
        assert t.nlm.start_id == t.sos_id
        nlm = LstmLM.load(ckpt, start_id=t.sos_id)
        want = []
        for idxs in t.eval_set.iter_indices():
            xs, il, ys, _ = t.eval_set.materialize(idxs)
            if mode == "nlm_ctc_beam":
                lists = t.asr_model.engine.recog_ctc_beam_nlm(xs, il, 8, nlm, 0.6, -0.2)
            else:
                lists = t.asr_model.engine.recog_rescore_nlm(xs, il, 8, nlm, 0.6, -0.2, 4, 0.6, 0.4)
                assert t.nbest == 4 and t.ctc_weight == 0.4 and abs(t.att_weight - 0.6) < 1e-12
            want += [_fmt(y, n[0][0]) for n, y in zip(lists, ys)]
        assert lines == want, mode
        # a plain transformer has no CTC output layer
        t, _, _, _ = tester(mode, bd, hybrid=False)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match="needs a CTC output layer"):
            t.exec()
        t, _, _, _ = tester(mode, bd, path=_checkpoint(tmp_path, C_SMALL, "small.pt"))
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match=f"the LSTM LM has {C_SMALL} classes, the model {ODIM} output units"):
            t.exec()
