"""The joint CTC/attention beam with the LSTM LM, a length bonus and an N-best list through the model (masr_recog_beam_ctc_nlm,
MasrEngine.recog_beam_ctc_nlm, Tester --decode_mode nlm_joint_beam) against the CPU restatement of tests/nlm_joint_beam_ref.py, the
joint LM beam and the joint beam at lm_w = 0 (bit for bit), and itself (batch order, repeated calls on one stream).  The twin of
test_hip_joint_lm_beam.py.

The model, JOINT_DELTA and the score tolerance 0.1 + 3e-3 |ref| are test_hip_joint_beam.py's (decode_util.py); the settings and the batches are
joint_lm_beam_ref's; the LMs are nlm_ref.toy_nlm(12, 16, 24, 2, seed) with the seeds of nlm_joint_beam_ref, picked on the CPU restatement
alone: an utterance is compared when its every decision gap exceeds JOINT_DELTA, every setting must have one such utterance per K and at least
half must qualify overall per K.  Counted on the restatement under the engine's bf16 operand rounding (tests/test_nlm_joint_beam_ref_cpu.py
asserts it), per setting in the order of SETTINGS / HKUST_SETTINGS:
  tiny, LM seed 4     K = 4: 31 of 45 (7, 5, 5, 7, 7)      K = 20: 26 of 45 (8, 5, 3, 9, 1)
  hkust, LM seed 25   K = 4:  9 of 16 (3, 2, 2, 2) or 12 of 16 (3, 3, 3, 3) with the BLAS's threading: near-ties at -50 .. -85 nats
                      (seed 0: 10 of 16 (3, 2, 3, 2) where seed 25 has 12; seed 4 leaves two settings without a qualifying utterance)
At K = 20 the winning hypotheses of this toy model are one or two tokens long, at K = 4 five to eight: the recurrent state's chain is tested
at K = 4, where (OWN_SLOT_SETTING) reading a row's own slot instead of its parent's changes the lists of four qualifying utterances on the CPU."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import hybrid_ref  # noqa: E402
import joint_lm_beam_ref as jl  # noqa: E402
import lm_ref  # noqa: E402
import nlm_joint_beam_ref as nj  # noqa: E402
import nlm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from masr_amd.nlm import LstmLM  # noqa: E402
from oracle import blstm_cpu, ref_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, JOINT_DELTA as DELTA  # noqa: E402
from decode_util import joint_engine, joint_state_dict, make_tester  # noqa: E402
from test_hip_engine import HKUST  # noqa: E402


def make_nlm(seed=nj.NLM_SEED_TINY, layers=nj.NLM_SHAPE[2]):
    d = nj.tiny_nlm(C_SMALL, seed, layers)
    return d, LstmLM.from_state_dict(nlm_ref.to_state_dict(d))


@pytest.fixture(scope="module")
def tiny():
    sd = joint_state_dict(TINY, 7)
    return sd, joint_engine(TINY, sd)


@pytest.fixture(scope="module")
def lms():
    return make_nlm()


@pytest.fixture(scope="module")
def ngram():
    return NGramLM(jl.LM_ORDER, C_SMALL, *lm_ref.to_arrays(lm_ref.toy_lm(C_SMALL, jl.LM_ORDER, jl.LM_SEED)))


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in nj.TINY_BATCHES]


def decode(eng, lm, xs, il, K, setting, **kw):
    aw, cw, lw, bo, N = setting
    return eng.recog_beam_ctc_nlm(xs, il, K, lm, lw, bo, N, att_weight=aw, ctc_weight=cw, **kw)


_REF = {}


def reference(sd, cfg, lm_dict, name, xs, il, K, setting):
    """the restatement under the engine's bf16 operand rounding; computed once per case and shared"""
    key = (name, K, setting)
    if key not in _REF:
        aw, cw, lw, bo, N = setting
        with ref_cpu.bf16_emulation():
            _REF[key] = nj.search(hybrid_ref.leafify(sd, cfg), cfg, xs, il, K, N, aw, cw, lm_dict, lw, bo)
    return _REF[key]


def _vs_cpu(eng, lm, sd, cfg, lm_dict, name, xs, il, K, setting):
    got = decode(eng, lm, xs, il, K, setting)
    ref = reference(sd, cfg, lm_dict, name, xs, il, K, setting)
    for b, (g, r) in enumerate(zip(got, ref)):              # every figure first, then the assertions
        print(f"  {name} utt {b}: gap {nj.min_gap(r):.3f}; " + "; ".join(
            f"{gt} {gs:.4f} / {rt} {rs:.4f}" for (gt, gs), (rt, rs) in zip(g, r["nbest"])))
    ok, worst = 0, 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        assert not any(math.isnan(s) for _, s in g)
        if nj.min_gap(r) <= DELTA:
            continue
        ok += 1
        assert [t for t, _ in g] == [t for t, _ in r["nbest"]], (K, setting, b, g, r["nbest"], nj.min_gap(r))      # all N entries: tokens and lens
        for (_, gs), (_, rs) in zip(g, r["nbest"]):
            worst = max(worst, abs(gs - rs))
            assert abs(gs - rs) <= 0.1 + 3e-3 * abs(rs), (K, setting, b, gs, rs)
    print(f"K = {K}, {setting}: {ok} of {len(ref)} utterances qualify; entries identical, worst score diff {worst:.2e}")
    return ok, len(ref)


@pytest.mark.parametrize("K", nj.TINY_KS)
def test_vs_cpu_restatement_tiny(tiny, lms, batches, K):
    sd, e = tiny
    lm_dict, lm = lms
    ok = n = 0
    for s in nj.SETTINGS:
        oks = 0
        for i, (xs, il) in enumerate(batches):
            a, b = _vs_cpu(e, lm, sd, TINY, lm_dict, f"tiny{i}", xs, il, K, s)
            oks += a; n += b
        assert oks >= 1, s
        ok += oks
    assert ok >= 0.5 * n, (ok, n)


def test_vs_cpu_restatement_hkust_geometry():
    lm_dict, lm = make_nlm(nj.NLM_SEED_HKUST)
    sd = joint_state_dict(HKUST, 3)
    e = joint_engine(HKUST, sd)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor(nj.HKUST_ILENS)
    ok = n = 0
    for s in nj.HKUST_SETTINGS:
        a, b = _vs_cpu(e, lm, sd, HKUST, lm_dict, "hkust", xs, il, 4, s)
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_the_lm_and_its_state_matter(tiny, lms, batches):
    """at OWN_SLOT_SETTING: a qualifying utterance whose lists the own-slot mutation changes on the CPU gets the honest restatement's lists
    from the engine (so not the mutated ones), and the engine's tokens differ from its own at lm_w = 0 on a qualifying utterance"""
    sd, e = tiny
    lm_dict, lm = lms
    K, s = nj.OWN_SLOT_K, nj.OWN_SLOT_SETTING
    aw, cw, lw, bo, N = s
    tell_own = tell_lm = 0
    for i, (xs, il) in enumerate(batches):
        ref = reference(sd, TINY, lm_dict, f"tiny{i}", xs, il, K, s)
        with ref_cpu.bf16_emulation():
            wrong = nj.search(hybrid_ref.leafify(sd, TINY), TINY, xs, il, K, N, aw, cw, lm_dict, lw, bo, own_slot=True)
        got = decode(e, lm, xs, il, K, s)
        zero = decode(e, lm, xs, il, K, (aw, cw, 0.0, bo, N))
        for b, (r, w, g, z) in enumerate(zip(ref, wrong, got, zero)):
            if nj.min_gap(r) <= DELTA:
                continue
            if [t for t, _ in r["nbest"]] != [t for t, _ in w["nbest"]]:
                tell_own += 1
                assert [t for t, _ in g] == [t for t, _ in r["nbest"]] != [t for t, _ in w["nbest"]], (i, b, g, r["nbest"], w["nbest"])
            tell_lm += g[0][0] != z[0][0]
    print(f"K = {K}, {s}: the own-slot mutation shows on {tell_own} qualifying utterances, the LM changes the tokens of {tell_lm}")
    assert tell_own >= 1 and tell_lm >= 1


def test_weight_zero_is_the_joint_lm_beam_at_zero_bit_for_bit(tiny, lms, ngram, batches):
    """lm_w = 0: any LM weighs nothing, so tokens, lens and score bits are masr_recog_beam_ctc_lm's with an n-gram LM at lm_w = 0, for every
    (len_bonus, N) of the settings; with len_bonus = 0 and N = 1 the scores are masr_recog_beam_ctc's"""
    _, e = tiny
    _, lm = lms
    for K in (1, 4, 20):
        for aw, cw, _, bo, N in nj.SETTINGS:
            s = (aw, cw, 0.0, bo, min(N, K))
            for xs, il in batches:
                got = decode(e, lm, xs, il, K, s, raw=True)
                want = e.recog_beam_ctc_lm(xs, il, K, ngram, 0.0, bo, min(N, K), att_weight=aw, ctc_weight=cw, raw=True)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (K, s)
                assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), (K, s, got[2], want[2])
        for aw, cw in ((0.5, 0.5), (0.7, 0.3), (0.0, 1.0)):
            for xs, il in batches:
                _, s0 = e.recog_beam(xs, il, K, att_weight=aw, ctc_weight=cw)
                got = decode(e, lm, xs, il, K, (aw, cw, 0.0, 0.0, 1))
                assert [g[0][1] if g else -math.inf for g in got] == s0.tolist(), (K, aw, cw)


def test_batch_permutation(tiny, lms):
    _, e = tiny
    _, lm = lms
    xs, il, _, _ = synth_batch(31, [64, 40, 52, 33, 60], [3] * 5)
    K, s = 6, (0.7, 0.3, 0.3, 1.0, 3)
    r1 = decode(e, lm, xs, il, K, s, raw=True)
    r2 = decode(e, lm, xs, il, K, s, raw=True)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    perm = [3, 0, 4, 2, 1]
    rp = decode(e, lm, xs[perm], il[perm], K, s, raw=True)
    assert all(torch.equal(a, b[perm]) for a, b in zip(rp, r1))      # tokens, lens and score bits
    tok, lens, sc = (t.cpu() for t in r1)
    assert ((lens >= -1) & (lens <= (il // 4)[:, None])).all() and (lens[:, 0] >= 0).all()
    for b in range(5):
        for n in range(3):
            L = int(lens[b, n])
            if L < 0:
                assert sc[b, n] == -math.inf and (tok[b, n] == -1).all()
            else:
                assert (tok[b, n, L:] == -1).all() and ((tok[b, n, :L] > 0) & (tok[b, n, :L] < C_SMALL - 1)).all()


def test_repeated_calls_never_replay_stale_values(tiny, batches):
    """one engine on a side stream (the step graph is captured and replayed there): calls that change lm_w, len_bonus, att_w, N and the LM --
    one LM destroyed and another (one layer, another seed) created, possibly at its address -- give what a fresh engine gives on the default
    stream (direct launches); a joint n-gram decode in between keeps its own graph"""
    sd, _ = tiny
    xs, il = batches[0]
    xs = xs.cuda()
    K = 4
    d1, lm1 = make_nlm()
    seq = [(0.7, 0.3, 0.3, 1.0, 2), (0.7, 0.3, 0.6, 1.0, 2), (0.7, 0.3, 0.6, 2.0, 2), (0.5, 0.3, 0.6, 2.0, 2), (0.5, 0.3, 0.6, 2.0, 1),
           (0.7, 0.3, 0.3, 1.0, 2)]
    fresh = joint_engine(TINY, sd)
    assert torch.cuda.current_stream().cuda_stream == 0
    want = [decode(fresh, lm1, xs, il, K, s) for s in seq]
    assert len({repr(w) for w in want}) >= 4                  # the changes matter
    e = joint_engine(TINY, sd)
    decode(e, lm1, xs, il, K, seq[0])                         # grows the workspace to its final size on the default stream
    decode(e, lm1, xs, il, K, seq[0][:4] + (K,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [decode(e, lm1, xs, il, K, s) for s in seq]
        side.synchronize()
        lm1.close()                                          # destroy, then another LM (other shape and values) in its place
        d2, lm2 = make_nlm(seed=nj.NLM_SEED_TINY + 1, layers=1)
        got2 = decode(e, lm2, xs, il, K, seq[0])
    side.synchronize()
    assert got == want
    want2 = decode(fresh, lm2, xs, il, K, seq[0])
    assert got2 == want2
    assert want2 != want[0]


def test_refusals(tiny, lms):
    sd, _ = tiny
    _, lm = lms
    e = joint_engine(TINY, sd)                               # a fresh workspace
    xs, il, _, _ = synth_batch(11, [40], [3])
    l = lib()
    xs_d = xs.cuda().contiguous()
    buf = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    fn = "masr_recog_beam_ctc_nlm"

    def call(eng, lmh, K, N, aw, cw, lw, bo, ilv=il):
        return l.masr_recog_beam_ctc_nlm(eng.h, lmh, p(xs_d), p(ilv), 1, 40, K, N, 0.0, 1.0, aw, cw, lw, bo, p(buf), p(buf), p(buf), None)

    def err():
        return l.masr_last_error().decode()

    plain = MasrEngine(TINY, C_SMALL)
    plain.load_state_dict({k: v for k, v in sd.items() if k not in hybrid_ref.HEAD})
    with pytest.raises(MasrError, match="no CTC head"):
        decode(plain, lm, xs, il, 4, (0.5, 0.5, 0.3, 0.0, 1))
    assert l.masr_beam_ctc_nlm_workspace_bytes(plain.h, lm.h, 1, 40, 4, 1, 10) < 0
    assert err() == "masr_beam_ctc_nlm_workspace_bytes: the model has no CTC head (masr_create_ctc)"
    decode(e, lm, xs, il, 1, (0.5, 0.5, 0.3, 0.0, 1))         # binds a workspace sized for K = 1
    buf.fill_(77)
    nan, inf = float("nan"), float("inf")
    lm13 = LstmLM.from_state_dict(nlm_ref.to_state_dict(nlm_ref.toy_nlm(C_SMALL + 1, 8, 8, 1, 1)))
    for args, msg in (((None, 4, 1, 0.5, 0.5, 0.3, 0.0), "null language model"),
                      ((lm13.h, 4, 1, 0.5, 0.5, 0.3, 0.0), "the language model's classes differ from the model's odim"),
                      ((lm.h, 4, 1, 0.5, 0.5, -1.0, 0.0), "lm_w must be finite and >= 0"),
                      ((lm.h, 4, 1, 0.5, 0.5, nan, 0.0), "lm_w must be finite and >= 0"),
                      ((lm.h, 4, 1, 0.5, 0.5, 0.3, inf), "len_bonus must be finite"),
                      ((lm.h, 4, 0, 0.5, 0.5, 0.3, 0.0), "N must be in [1, K]"),
                      ((lm.h, 4, 5, 0.5, 0.5, 0.3, 0.0), "N must be in [1, K]"),
                      ((lm.h, 4, 1, 0.5, 0.0, 0.3, 0.0), "ctc_w must be finite and > 0"),
                      ((lm.h, 4, 1, 0.5, nan, 0.3, 0.0), "ctc_w must be finite and > 0"),
                      ((lm.h, 4, 1, -0.1, 0.5, 0.3, 0.0), "att_w must be finite and >= 0"),
                      ((lm.h, 0, 1, 0.5, 0.5, 0.3, 0.0), "beam size K must be in [1, 64]"),
                      ((lm.h, 65, 1, 0.5, 0.5, 0.3, 0.0), "beam size K must be in [1, 64]")):
        assert call(e, *args) == -1 and err() == f"{fn}: {msg}", (args, err())
    assert call(plain, lm.h, 4, 1, 0.5, 0.5, 0.3, 0.0) == -1 and err() == f"{fn}: the model has no CTC head (masr_create_ctc)"
    il_bad = torch.tensor([3], dtype=torch.int64)
    assert call(e, lm.h, 4, 1, 0.5, 0.5, 0.3, 0.0, il_bad) != 0 and "ilens must be in [4, T]" in err()
    torch.cuda.synchronize()
    assert (buf == 77).all()                                 # nothing was launched: no output was written
    assert l.masr_beam_ctc_nlm_workspace_bytes(e.h, None, 1, 40, 4, 1, 10) < 0 and err() == "masr_beam_ctc_nlm_workspace_bytes: null language model"
    for bad in ((0, 40, 4, 1, 10), (1, 3, 4, 1, 10), (1, 40, 4, 5, 10), (1, 40, 4, 0, 10), (1, 40, 65, 1, 10), (1, 40, 4, 1, 0)):
        assert l.masr_beam_ctc_nlm_workspace_bytes(e.h, lm.h, *bad) < 0
        assert err() == "masr_beam_ctc_nlm_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1"
    # the workspace: the joint LM beam's plus the header's formula, each entry rounded up to 256 bytes (Cp = 128, Hp = 32, L = 2)
    r256 = lambda n: (n + 255) // 256 * 256                   # noqa: E731
    for B, K, N in ((1, 1, 1), (3, 20, 5)):
        R, Ll = B * K, nj.NLM_SHAPE[2]
        extra = l.masr_beam_ctc_nlm_workspace_bytes(e.h, lm.h, B, 40, K, N, 10) - l.masr_beam_ctc_lm_workspace_bytes(e.h, B, 40, K, N, 10)
        assert extra == r256(R * 128 * 4) + r256(2 * Ll * R * 32 * 2) + r256(2 * Ll * R * 32 * 4) + r256(R * 32 * 2), (B, K, extra)
    # a workspace one byte short of what the plan places (the query less its 4096 bytes of slack): -2 under the new query's name, nothing launched;
    # the query's own size decodes
    need = int(l.masr_beam_ctc_nlm_workspace_bytes(e.h, lm.h, 1, 40, 4, 2, 10))       # ilens 40 -> enc_len 10 = Lmax
    small = joint_engine(TINY, sd)
    torch.cuda.synchronize()
    for nbytes, rc_want in ((need - 4096 - 1, -2), (need, 0)):
        small.ws = torch.empty(nbytes, dtype=torch.uint8, device=small.device)
        assert l.masr_bind(small.h, p(small.params), p(small.grads), p(small.pe), p(small.ws), small.ws.numel()) == 0
        small.mark_dirty(); small.refresh()
        buf.fill_(77)
        rc = l.masr_recog_beam_ctc_nlm(small.h, lm.h, p(xs_d), p(il), 1, 40, 4, 2, 0.0, 1.0, 0.5, 0.5, 0.3, 0.0, p(buf), p(buf[64:]), p(buf[128:]),
                                       small.stream())
        torch.cuda.synchronize()
        assert rc == rc_want, (nbytes, rc, err())
        if rc_want:
            assert err() == "masr_recog: workspace too small (masr_beam_ctc_nlm_workspace_bytes(nlm, B, T, K, N, Lmax))"
            assert (buf == 77).all()
    with pytest.raises(ValueError, match="nbest"):
        e.recog_beam_ctc_nlm(xs, il, 4, lm, nbest=5)
    with pytest.raises(ValueError, match="lm_w"):
        e.recog_beam_ctc_nlm(xs, il, 4, lm, lm_w=-1.0)
    with pytest.raises(ValueError, match="len_bonus"):
        e.recog_beam_ctc_nlm(xs, il, 4, lm, len_bonus=inf)
    with pytest.raises(ValueError, match="live LstmLM"):
        e.recog_beam_ctc_nlm(xs, il, 4, None)


# ---------------------------------------------------------------- Tester
def _checkpoint(tmp_path, C_=ODIM, name="toy_nlm.pt"):
    path = tmp_path / name
    if not path.exists():
        torch.save(nlm_ref.to_state_dict(nlm_ref.toy_nlm(C_, 24, 40, 2, 5)), path)
    return str(path)


def test_tester_nlm_joint_beam_end_to_end(tmp_path, monkeypatch):
    block = {"beam_size": 6, "att_w": 0.6, "ctc_w": 0.4, "lm_w": 0.4, "len_bonus": 0.5, "nbest": 3, "lm_start": "eos"}
    t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, "nlm_joint_beam", block, hybrid=True)
    t.load_data(); t.set_model()
    t.paras.lm_model_path = _checkpoint(tmp_path)
    t.exec()
    assert (t.att_weight, t.ctc_weight, t.lm_weight, t.len_bonus, t.nbest) == (0.6, 0.4, 0.4, 0.5, 3) and t.nlm.start_id == ODIM - 1
    lines = (log_dir / "nlm_joint_beam_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6
    eng = MasrEngine(cfg["asr_model"], ODIM)
    eng.load_state_dict(sd)
    want = []
    for idxs in t.eval_set.iter_indices():                     # the Tester's own batches; the best entry is written
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        lists = eng.recog_beam_ctc_nlm(xs, il, 6, t.nlm, 0.4, 0.5, 3, att_weight=0.6, ctc_weight=0.4)
        want += ["{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(str(v) for v in (h[0][0] if h else []))) for h, y in zip(lists, ys)]
    assert lines == want
    assert any(l.split("\t")[1] for l in lines)
    # defaults: lm_w 0.3, len_bonus 0, nbest 1, att_w = 1 - ctc_w, lm_start sos
    t2, _, _, _ = make_tester(tmp_path, monkeypatch, "nlm_joint_beam", {"beam_size": 4, "ctc_w": 0.3}, hybrid=True)
    t2.load_data(); t2.set_model()
    t2.paras.lm_model_path = t.paras.lm_model_path
    t2._nlm_joint_settings()
    assert (t2.lm_weight, t2.len_bonus, t2.nbest, t2.nlm.start_id) == (0.3, 0.0, 1, 0) and t2.att_weight == pytest.approx(0.7)


def test_tester_nlm_joint_beam_settings_are_vetted_at_exec(tmp_path, monkeypatch):
    ok = {"beam_size": 4, "ctc_w": 0.3}

    def tester(block, hybrid=True, path=True, **kw):
        t, _, _, _ = make_tester(tmp_path, monkeypatch, "nlm_joint_beam", block, hybrid=hybrid, **kw)
        t.load_data(); t.set_model()
        t.paras.lm_model_path = _checkpoint(tmp_path) if path else None
        return t

    with pytest.raises(NotImplementedError, match="no language model given; pass --lm_model_path"):
        tester(ok, path=False).exec()
    with pytest.raises(ValueError, match="needs a CTC output layer"):
        tester(ok, hybrid=False).exec()
    for block in ({"beam_size": 4}, {"beam_size": 4, "ctc_w": 0.0}):
        with pytest.raises(ValueError, match="nlm_beam"):
            tester(block).exec()
    for bad in ({"lm_w": -0.1}, {"lm_w": float("nan")}, {"len_bonus": float("inf")}, {"nbest": 0}, {"nbest": 5}, {"att_w": -1.0}, {"ctc_w": 1.5},
                {"beam_size": 65}, {"lm_start": "bos"}):
        with pytest.raises(ValueError, match="beam_decode"):
            tester(dict(ok, **bad)).exec()
    with pytest.raises(ValueError, match="beam_decode"):
        tester(None).exec()
    t = tester(ok)
    t.paras.lm_model_path = _checkpoint(tmp_path, C_SMALL, "small.pt")
    with pytest.raises(ValueError, match=f"the LSTM LM has {C_SMALL} classes, the model {ODIM} output units"):
        t.exec()


def test_tester_nlm_joint_beam_refuses_the_blstm(tmp_path, monkeypatch):
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "nlm_joint_beam", {"beam_size": 4, "ctc_w": 0.3}, blstm_sd=sd)
    t.load_data(); t.set_model()
    t.paras.lm_model_path = str(tmp_path / "any.pt")
    with pytest.raises(NotImplementedError, match="nlm_joint_beam"):
        t.exec()
