"""The joint CTC/attention beam with an n-gram LM, a length bonus and an N-best list through the model (masr_recog_beam_ctc_lm,
MasrEngine.recog_beam_ctc_lm, Tester --decode_mode lm_joint_beam) against the CPU restatement of tests/joint_lm_beam_ref.py, the
joint beam without an LM, and itself (batch order, list length, repeated calls on one stream).

The model, JOINT_DELTA and the score tolerance are test_hip_joint_beam.py's (decode_util.py); the LM, the settings and the batches are
joint_lm_beam_ref's, whose qualifying share tests/test_joint_lm_beam_ref_cpu.py asserts on the restatement alone."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import hybrid_ref  # noqa: E402
import joint_lm_beam_ref as jl  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle import blstm_cpu, ref_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, JOINT_DELTA as DELTA  # noqa: E402
from decode_util import joint_engine, joint_state_dict, make_tester  # noqa: E402
from test_hip_engine import HKUST  # noqa: E402


def make_lm(seed=jl.LM_SEED):
    d = lm_ref.toy_lm(C_SMALL, jl.LM_ORDER, seed)
    return d, NGramLM(jl.LM_ORDER, C_SMALL, *lm_ref.to_arrays(d))


@pytest.fixture(scope="module")
def tiny():
    sd = joint_state_dict(TINY, 7)
    return sd, joint_engine(TINY, sd)


@pytest.fixture(scope="module")
def lms():
    return make_lm()


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in jl.TINY_BATCHES]


def decode(eng, lm, xs, il, K, setting, **kw):
    aw, cw, lw, bo, N = setting
    return eng.recog_beam_ctc_lm(xs, il, K, lm, lw, bo, N, att_weight=aw, ctc_weight=cw, **kw)


_REF = {}


def reference(sd, cfg, lm_dict, name, xs, il, K, setting):
    """the restatement under the engine's bf16 operand rounding; computed once per case and shared"""
    key = (name, K, setting)
    if key not in _REF:
        aw, cw, lw, bo, N = setting
        with ref_cpu.bf16_emulation():
            _REF[key] = jl.search(hybrid_ref.leafify(sd, cfg), cfg, xs, il, K, N, aw, cw, lm_dict, lw, bo)
    return _REF[key]


def _vs_cpu(eng, lm, sd, cfg, lm_dict, name, xs, il, K, setting):
    got = decode(eng, lm, xs, il, K, setting)
    ref = reference(sd, cfg, lm_dict, name, xs, il, K, setting)
    for b, (g, r) in enumerate(zip(got, ref)):              # every figure first, then the assertions
        print(f"  {name} utt {b}: gap {jl.min_gap(r):.3f}; " + "; ".join(
            f"{gt} {gs:.4f} / {rt} {rs:.4f}" for (gt, gs), (rt, rs) in zip(g, r["nbest"])))
    ok, worst = 0, 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        assert not any(math.isnan(s) for _, s in g)
        if jl.min_gap(r) <= DELTA:
            continue
        ok += 1
        assert [t for t, _ in g] == [t for t, _ in r["nbest"]], (K, setting, b, g, r["nbest"], jl.min_gap(r))      # all N entries: tokens and lens
        for (_, gs), (_, rs) in zip(g, r["nbest"]):
            worst = max(worst, abs(gs - rs))
            assert abs(gs - rs) <= 0.1 + 3e-3 * abs(rs), (K, setting, b, gs, rs)
    print(f"K = {K}, {setting}: {ok} of {len(ref)} utterances qualify; entries identical, worst score diff {worst:.2e}")
    return ok, len(ref)


@pytest.mark.parametrize("K", jl.TINY_KS)
def test_vs_cpu_restatement_tiny(tiny, lms, batches, K):
    sd, e = tiny
    lm_dict, lm = lms
    ok = n = 0
    for s in jl.SETTINGS:
        oks = 0
        for i, (xs, il) in enumerate(batches):
            a, b = _vs_cpu(e, lm, sd, TINY, lm_dict, f"tiny{i}", xs, il, K, s)
            oks += a; n += b
        assert oks >= 1, s
        ok += oks
    assert ok >= 0.5 * n, (ok, n)


def test_vs_cpu_restatement_hkust_geometry(lms):
    lm_dict, lm = lms
    sd = joint_state_dict(HKUST, 3)
    e = joint_engine(HKUST, sd)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor(jl.HKUST_ILENS)
    ok = n = 0
    for s in jl.HKUST_SETTINGS:
        a, b = _vs_cpu(e, lm, sd, HKUST, lm_dict, "hkust", xs, il, 4, s)
        assert a >= 1, s
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_without_lm_bonus_and_list_it_is_the_joint_beam(tiny, lms, batches):
    """lm_w = 0, len_bonus = 0, N = 1: masr_recog_beam_ctc's scores as floats, and its tokens on these seeds (the two pre-beams order by lp
    and by logit: they differ only where rounding ties two logits' lp)"""
    _, e = tiny
    _, lm = lms
    for K in (1, 4, 20):
        for aw, cw in ((0.5, 0.5), (0.7, 0.3), (0.0, 1.0)):
            for xs, il in batches:
                t0, s0 = e.recog_beam(xs, il, K, att_weight=aw, ctc_weight=cw)
                got = decode(e, lm, xs, il, K, (aw, cw, 0.0, 0.0, 1))
                assert [g[0][0] if g else [] for g in got] == t0, (K, aw, cw)
                assert [g[0][1] if g else -math.inf for g in got] == s0.tolist(), (K, aw, cw)


def test_list_entries_and_the_best_of_a_full_list(tiny, lms, batches):
    sd, e = tiny
    lm_dict, lm = lms
    checked = 0
    for K in jl.TINY_KS:
        for s in jl.SETTINGS[:3]:
            for i, (xs, il) in enumerate(batches):
                one = decode(e, lm, xs, il, K, s[:4] + (1,))
                full = decode(e, lm, xs, il, K, s[:4] + (K,))
                ref = reference(sd, TINY, lm_dict, f"tiny{i}", xs, il, K, s[:4] + (1,))
                for b, (o, f, r) in enumerate(zip(one, full, ref)):
                    assert 1 <= len(f) <= K and len(o) == 1
                    assert len({tuple(t) for t, _ in f}) == len(f), (K, s, b, f)              # distinct sequences
                    assert all(f[j][1] >= f[j + 1][1] for j in range(len(f) - 1)), (K, s, b, f)   # non-increasing scores
                    if jl.min_gap(r) > DELTA:               # entry 0 of the N = K call is the N = 1 call's result
                        assert f[0] == o[0], (K, s, b, f[0], o[0])
                        checked += 1
    assert checked >= 20, checked


def test_batch_permutation_and_single_utterances(tiny, lms):
    sd, e = tiny
    lm_dict, lm = lms
    xs, il, _, _ = synth_batch(31, [64, 40, 52, 33, 60], [3] * 5)
    K, s = 6, (0.7, 0.3, 0.3, 1.0, 3)
    r1 = decode(e, lm, xs, il, K, s, raw=True)
    r2 = decode(e, lm, xs, il, K, s, raw=True)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    perm = [3, 0, 4, 2, 1]
    rp = decode(e, lm, xs[perm], il[perm], K, s, raw=True)
    assert all(torch.equal(a, b[perm]) for a, b in zip(rp, r1))      # tokens, lens and score bits
    tok, lens, sc = (t.cpu() for t in r1)
    assert ((lens >= -1) & (lens <= (il // 4)[:, None])).all()
    for b in range(5):
        for n in range(3):
            L = int(lens[b, n])
            if L < 0:
                assert sc[b, n] == -math.inf and (tok[b, n] == -1).all()
            else:
                assert (tok[b, n, L:] == -1).all() and ((tok[b, n, :L] > 0) & (tok[b, n, :L] < C_SMALL - 1)).all()
    ref = reference(sd, TINY, lm_dict, "perm", xs, il, K, s)
    n_ok = 0
    for b in range(5):                                       # alone: the encoder's tiling moves the memory by bf16 rounding
        alone = decode(e, lm, xs[b:b + 1], il[b:b + 1], K, s)[0]
        L0 = int(lens[b, 0])
        assert abs(alone[0][1] - float(sc[b, 0])) <= 0.1 + 3e-3 * abs(float(sc[b, 0])), b
        if jl.min_gap(ref[b]) > DELTA:
            assert alone[0][0] == tok[b, 0, :L0].tolist(), b
            n_ok += 1
    print(f"{n_ok} of 5 utterances qualify for the single-utterance comparison")


def test_repeated_calls_never_replay_stale_values(tiny, batches):
    """one engine on a side stream (the step graph is captured and replayed there): calls that change lm_w, len_bonus, att_w, N and the LM --
    one LM destroyed and another created, possibly at its address -- give what a fresh engine gives on the default stream (direct launches)"""
    sd, _ = tiny
    xs, il = batches[0]
    xs = xs.cuda()
    K = 4
    d1, lm1 = make_lm()
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
        lm1.close()                                          # destroy, then another LM (other values) in its place
        d2, lm2 = make_lm(seed=3)
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

    def call(eng, lmh, K, N, aw, cw, lw, bo, ilv=il):
        return l.masr_recog_beam_ctc_lm(eng.h, lmh, p(xs_d), p(ilv), 1, 40, K, N, 0.0, 1.0, aw, cw, lw, bo, p(buf), p(buf), p(buf), None)

    plain = MasrEngine(TINY, C_SMALL)
    plain.load_state_dict({k: v for k, v in sd.items() if k not in hybrid_ref.HEAD})
    with pytest.raises(MasrError, match="no CTC head"):
        decode(plain, lm, xs, il, 4, (0.5, 0.5, 0.3, 0.0, 1))
    assert l.masr_beam_ctc_lm_workspace_bytes(plain.h, 1, 40, 4, 1, 10) < 0 and b"no CTC head" in l.masr_last_error()
    decode(e, lm, xs, il, 1, (0.5, 0.5, 0.3, 0.0, 1))         # binds a workspace sized for K = 1
    buf.fill_(77)
    nan, inf = float("nan"), float("inf")
    for args, msg in (((lm.h, 4, 1, 0.5, 0.0, 0.3, 0.0), b"ctc_w"), ((lm.h, 4, 1, 0.5, -0.1, 0.3, 0.0), b"ctc_w"), ((lm.h, 4, 1, 0.5, nan, 0.3, 0.0), b"ctc_w"),
                      ((lm.h, 4, 1, -0.1, 0.5, 0.3, 0.0), b"att_w"), ((lm.h, 4, 1, inf, 0.5, 0.3, 0.0), b"att_w"),
                      ((None, 4, 1, 0.5, 0.5, 0.3, 0.0), b"null language model"),
                      ((lm.h, 4, 1, 0.5, 0.5, -0.3, 0.0), b"lm_w"), ((lm.h, 4, 1, 0.5, 0.5, nan, 0.0), b"lm_w"), ((lm.h, 4, 1, 0.5, 0.5, inf, 0.0), b"lm_w"),
                      ((lm.h, 4, 1, 0.5, 0.5, 0.3, nan), b"len_bonus"), ((lm.h, 4, 1, 0.5, 0.5, 0.3, -inf), b"len_bonus"),
                      ((lm.h, 4, 0, 0.5, 0.5, 0.3, 0.0), b"N must be in [1, K]"), ((lm.h, 4, 5, 0.5, 0.5, 0.3, 0.0), b"N must be in [1, K]"),
                      ((lm.h, 0, 1, 0.5, 0.5, 0.3, 0.0), b"beam size K must be in [1, 64]"), ((lm.h, 65, 1, 0.5, 0.5, 0.3, 0.0), b"beam size K must be in [1, 64]")):
        assert call(e, *args) == -1 and msg in l.masr_last_error(), (args, l.masr_last_error())
    d13, lm13 = lm_ref.toy_lm(13, 2, 1), None
    lm13 = NGramLM(2, 13, *lm_ref.to_arrays(d13))
    assert call(e, lm13.h, 4, 1, 0.5, 0.5, 0.3, 0.0) == -1 and b"classes differ" in l.masr_last_error()
    il_bad = torch.tensor([3], dtype=torch.int64)
    assert call(e, lm.h, 4, 1, 0.5, 0.5, 0.3, 0.0, il_bad) != 0 and b"ilens must be in [4, T]" in l.masr_last_error()
    xl = torch.zeros(1, 4000, 83, device="cuda:0")               # K = 64 over 1000 frames: far beyond the K = 1 workspace
    il_l = torch.tensor([4000], dtype=torch.int64)
    assert l.masr_recog_beam_ctc_lm(e.h, lm.h, p(xl), p(il_l), 1, 4000, 64, 4, 0.0, 1.0, 0.5, 0.5, 0.3, 0.0, p(buf), p(buf), p(buf), None) == -2
    assert b"masr_beam_ctc_lm_workspace_bytes" in l.masr_last_error()
    torch.cuda.synchronize()
    assert (buf == 77).all()                                 # nothing was launched: no output was written
    for bad in ((0, 40, 4, 1, 10), (1, 3, 4, 1, 10), (1, 40, 4, 5, 10), (1, 40, 4, 0, 10), (1, 40, 65, 1, 10), (1, 40, 4, 1, 0)):
        assert l.masr_beam_ctc_lm_workspace_bytes(e.h, *bad) < 0
    # the plan holds the joint beam's buffers, the fused rows and the list
    assert l.masr_beam_ctc_lm_workspace_bytes(e.h, 16, 1000, 20, 20, 250) > l.masr_beam_ctc_workspace_bytes(e.h, 16, 1000, 20, 250)
    with pytest.raises(ValueError, match="nbest"):
        e.recog_beam_ctc_lm(xs, il, 4, lm, nbest=5)
    with pytest.raises(ValueError, match="lm_w"):
        e.recog_beam_ctc_lm(xs, il, 4, lm, lm_w=-1.0)


# ---------------------------------------------------------------- Tester
def _arpa(tmp_path):
    path = tmp_path / "toy.arpa"
    if not path.exists():
        path.write_text(lm_ref.arpa_text(lm_ref.toy_lm_log10(ODIM, 3, 5, n_sent=120, max_len=10, active=40), lm_ref.units(ODIM)))
    return str(path)


def test_tester_lm_joint_beam_end_to_end(tmp_path, monkeypatch):
    block = {"beam_size": 6, "att_w": 0.6, "ctc_w": 0.4, "lm_w": 0.4, "len_bonus": 0.5, "nbest": 3}
    t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, "lm_joint_beam", block, hybrid=True)
    t.load_data(); t.set_model()
    t.paras.lm_model_path = _arpa(tmp_path)
    t.exec()
    assert (t.att_weight, t.ctc_weight, t.lm_weight, t.len_bonus, t.nbest) == (0.6, 0.4, 0.4, 0.5, 3)
    lines = (log_dir / "lm_joint_beam_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6
    eng = MasrEngine(cfg["asr_model"], ODIM)
    eng.load_state_dict(sd)
    want = []
    for idxs in t.eval_set.iter_indices():                     # the Tester's own batches; the best entry is written
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        lists = eng.recog_beam_ctc_lm(xs, il, 6, t.lm, 0.4, 0.5, 3, att_weight=0.6, ctc_weight=0.4)
        want += ["{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(str(v) for v in (h[0][0] if h else []))) for h, y in zip(lists, ys)]
    assert lines == want
    # defaults: lm_w 0.3, len_bonus 0, nbest 1, att_w = 1 - ctc_w
    t2, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_joint_beam", {"beam_size": 4, "ctc_w": 0.3}, hybrid=True)
    t2.load_data(); t2.set_model()
    t2.paras.lm_model_path = t.paras.lm_model_path
    t2._lm_joint_settings()
    assert (t2.lm_weight, t2.len_bonus, t2.nbest) == (0.3, 0.0, 1) and t2.att_weight == pytest.approx(0.7)


def test_tester_lm_joint_beam_settings_are_vetted_at_exec(tmp_path, monkeypatch):
    ok = {"beam_size": 4, "ctc_w": 0.3}

    def tester(block, hybrid=True, path=True, **kw):
        t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_joint_beam", block, hybrid=hybrid, **kw)
        t.load_data(); t.set_model()
        t.paras.lm_model_path = _arpa(tmp_path) if path else None
        return t

    with pytest.raises(NotImplementedError, match="no language model given; pass --lm_model_path"):
        tester(ok, path=False).exec()
    with pytest.raises(ValueError, match="needs a CTC output layer"):
        tester(ok, hybrid=False).exec()
    for block in ({"beam_size": 4}, {"beam_size": 4, "ctc_w": 0.0}):
        with pytest.raises(ValueError, match="lm_beam"):
            tester(block).exec()
    for bad in ({"lm_w": -0.1}, {"lm_w": float("nan")}, {"len_bonus": float("inf")}, {"nbest": 0}, {"nbest": 5}, {"att_w": -1.0}, {"ctc_w": 1.5},
                {"beam_size": 65}):
        with pytest.raises(ValueError, match="beam_decode"):
            tester(dict(ok, **bad)).exec()
    with pytest.raises(ValueError, match="beam_decode"):
        tester(None).exec()


def test_tester_lm_joint_beam_refuses_the_blstm(tmp_path, monkeypatch):
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_joint_beam", {"beam_size": 4, "ctc_w": 0.3}, blstm_sd=sd)
    t.load_data(); t.set_model()
    t.paras.lm_model_path = str(tmp_path / "any.arpa")
    with pytest.raises(NotImplementedError, match="lm_joint_beam"):
        t.exec()
