"""GPU joint CTC/attention beam search (masr_recog_beam_ctc, MasrEngine.recog_beam(..., ctc_weight), Tester with beam_decode.ctc_w)
against the CPU restatement of tests/joint_beam_ref.py and the attention-only beam."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import hybrid_ref  # noqa: E402
import joint_beam_ref as jr  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from decode_util import JOINT_DELTA as DELTA  # noqa: E402
from decode_util import joint_engine, joint_state_dict, make_tester  # noqa: E402
from test_hip_engine import HKUST  # noqa: E402

# The model, DELTA and the tolerances: decode_util.py (JOINT_DELTA).
WEIGHTS = [(0.5, 0.5), (0.7, 0.3), (0.0, 1.0)]


@pytest.fixture(scope="module")
def tiny():
    sd = joint_state_dict(TINY, 7)
    return sd, joint_engine(TINY, sd)


def _vs_cpu(eng, sd, cfg, xs, il, K, aw, cw, **kw):
    toks, sc = eng.recog_beam(xs, il, K, att_weight=aw, ctc_weight=cw, **kw)
    assert not torch.isnan(sc).any()
    with ref_cpu.bf16_emulation():
        ref = jr.joint_beam_search(hybrid_ref.leafify(sd, cfg), cfg, xs, il, K, aw, cw, **kw)
    ok, worst = 0, 0.0
    for b, r in enumerate(ref):
        if jr.min_gap(r) <= DELTA:
            continue
        ok += 1
        assert toks[b] == r["tokens"], (K, aw, cw, b, toks[b], r["tokens"], jr.min_gap(r))
        if r["score"] == -math.inf:
            assert float(sc[b]) == -math.inf
            continue
        worst = max(worst, abs(float(sc[b]) - r["score"]))
        assert abs(float(sc[b]) - r["score"]) <= 0.1 + 3e-3 * abs(r["score"]), (K, b, float(sc[b]), r["score"])
    print(f"K = {K}, att_w = {aw}, ctc_w = {cw}: {ok} of {len(ref)} utterances qualify; tokens identical, worst score diff {worst:.2e}")
    return ok, len(ref), toks, ref


TINY_BATCHES = ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60]))


@pytest.mark.parametrize("K", [4, 20])
def test_joint_vs_cpu_restatement_tiny(tiny, K):
    sd, e = tiny
    ok = n = 0
    for w in WEIGHTS:
        okw = 0
        for seed, ilens in TINY_BATCHES:
            xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
            a, b, _, _ = _vs_cpu(e, sd, TINY, xs, il, K, *w)
            okw += a; n += b
        assert okw >= 1, w
        ok += okw
    assert ok >= 0.5 * n, (ok, n)


def test_joint_vs_cpu_restatement_hkust_geometry():
    sd = joint_state_dict(HKUST, 3)
    e = joint_engine(HKUST, sd)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor([96, 88, 80, 72])
    ok = n = 0
    for w in WEIGHTS:
        a, b, _, _ = _vs_cpu(e, sd, HKUST, xs, il, 4, *w)
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_ctc_term_changes_the_result(tiny):
    sd, e = tiny
    changed = 0
    for seed, ilens in TINY_BATCHES:
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        att, _ = e.recog_beam(xs, il, 4)
        _, _, toks, ref = _vs_cpu(e, sd, TINY, xs, il, 4, 0.5, 0.5)
        changed += sum(1 for b, r in enumerate(ref) if jr.min_gap(r) > DELTA and toks[b] != att[b] and toks[b] == r["tokens"])
    assert changed >= 1


def test_joint_batch_independence_and_graph_replay(tiny):
    _, e = tiny
    xs, il, _, _ = synth_batch(31, [64, 40, 52, 33, 60], [3] * 5)
    K, w = 6, dict(att_weight=0.5, ctc_weight=0.5)
    t1, s1 = e.recog_beam(xs, il, K, **w)
    t2, s2 = e.recog_beam(xs, il, K, **w)                      # again (direct launches on this stream; graphs: test_hip_decode_graphs.py)
    assert t1 == t2 and torch.equal(s1, s2)
    perm = [3, 0, 4, 2, 1]
    tp, sp = e.recog_beam(xs[perm], il[perm], K, **w)
    assert tp == [t1[i] for i in perm]
    assert torch.equal(sp, s1[perm])                           # bit for bit
    for b in range(5):                                         # alone: same tokens (the encoder's tiling moves the memory by bf16 rounding)
        ta, _ = e.recog_beam(xs[b:b + 1], il[b:b + 1], K, **w)
        assert ta[0] == t1[b], b
    # a shape change (new capture) and back, other weights in between (their own key): identical bits
    e.recog_beam(xs[:2], il[:2], 3, att_weight=0.7, ctc_weight=0.3)
    e.recog_beam(xs, il, K)
    t3, s3 = e.recog_beam(xs, il, K, **w)
    assert t3 == t1 and torch.equal(s3, s1)
    assert all(len(t) <= int(n) // 4 for t, n in zip(t1, il))


def test_joint_short_utterances(tiny):
    """enc_len 1 - 2 frames with min_step_ratio > 1: no NaN, no hang, the restatement's (possibly empty, -inf) result"""
    sd, e = tiny
    xs, il, _, _ = synth_batch(41, [4, 7, 8, 11], [1] * 4)
    for minr, maxr in ((1.5, 3.0), (2.5, 0.0), (1.0, 2.0)):
        toks, sc = e.recog_beam(xs, il, 4, minr, maxr, att_weight=0.5, ctc_weight=0.5)
        assert not torch.isnan(sc).any()
        with ref_cpu.bf16_emulation():
            ref = jr.joint_beam_search(hybrid_ref.leafify(sd, TINY), TINY, xs, il, 4, 0.5, 0.5, minr, maxr)
        for b, r in enumerate(ref):
            if r["score"] == -math.inf:
                assert toks[b] == [] and float(sc[b]) == -math.inf, (minr, maxr, b, toks[b], float(sc[b]))
            elif jr.min_gap(r) > DELTA:
                assert toks[b] == r["tokens"], (minr, maxr, b, toks[b], r)


def test_joint_long_utterances(tiny):
    """enc_len 275 / 325 frames: the prefix kernel's chains cross its 256-frame LDS chunks in the decode (maxlen kept short by
    max_step_ratio so that the restatement stays cheap)"""
    sd, e = tiny
    xs, il, _, _ = synth_batch(51, [1100, 1300, 1030], [3] * 3)
    ok = 0
    for w in ((0.5, 0.5), (0.0, 1.0)):
        a, _, toks, _ = _vs_cpu(e, sd, TINY, xs, il, 4, *w, max_step_ratio=0.05)
        ok += a
    assert ok >= 1


def test_ctc_weight_zero_is_attention_beam_bits(tiny):
    _, e = tiny
    xs, il, _, _ = synth_batch(17, [48, 64, 33], [3] * 3)
    ta, sa = e.recog_beam(xs, il, 5)
    tb, sb = e.recog_beam(xs, il, 5, att_weight=0.7, ctc_weight=0.0)
    assert ta == tb and torch.equal(sa, sb)


def test_joint_errors(tiny):
    sd, _ = tiny
    e = joint_engine(TINY, sd)                                 # a fresh workspace
    xs, il, _, _ = synth_batch(11, [40], [3])
    l = lib()
    xs_d = xs.cuda().contiguous()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731

    def call(eng, K, aw, cw):
        return l.masr_recog_beam_ctc(eng.h, p(xs_d), p(il), 1, 40, K, 0.0, 1.0, aw, cw, p(buf), p(buf), p(buf), None)

    plain = MasrEngine(TINY, ODIM)
    plain.load_state_dict(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7))
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_beam(xs, il, 4, att_weight=0.5, ctc_weight=0.5)
    assert l.masr_beam_ctc_workspace_bytes(plain.h, 1, 40, 4, 10) < 0 and b"no CTC head" in l.masr_last_error()
    e.recog_beam(xs, il, 1, att_weight=0.5, ctc_weight=0.5)    # binds a workspace sized for K = 1
    for aw, cw, msg in ((0.5, 0.0, b"ctc_w"), (0.5, -0.1, b"ctc_w"), (0.5, float("nan"), b"ctc_w"), (0.5, float("inf"), b"ctc_w"),
                        (-0.1, 0.5, b"att_w"), (float("inf"), 0.5, b"att_w"), (float("nan"), 0.5, b"att_w")):
        assert call(e, 4, aw, cw) != 0 and msg in l.masr_last_error(), (aw, cw)
    with pytest.raises(MasrError, match="ctc_w"):
        e.recog_beam(xs, il, 4, att_weight=0.5, ctc_weight=-1.0)
    for K in (0, 65):
        assert call(e, K, 0.5, 0.5) != 0 and b"beam size K must be in [1, 64]" in l.masr_last_error()
    il_bad = torch.tensor([3], dtype=torch.int64)
    assert l.masr_recog_beam_ctc(e.h, p(xs_d), p(il_bad), 1, 40, 4, 0.0, 1.0, 0.5, 0.5, p(buf), p(buf), p(buf), None) != 0
    assert b"ilens must be in [4, T]" in l.masr_last_error()
    xl = torch.zeros(1, 4000, 83, device="cuda:0")               # K = 64 over 1000 frames: far beyond the K = 1 workspace
    il_l = torch.tensor([4000], dtype=torch.int64)
    assert l.masr_recog_beam_ctc(e.h, p(xl), p(il_l), 1, 4000, 64, 0.0, 1.0, 0.5, 0.5, p(buf), p(buf), p(buf), None) != 0
    assert b"masr_beam_ctc_workspace_bytes" in l.masr_last_error()
    # the CTC states dominate the workspace: 2 R T' P fp32 pairs
    need = l.masr_beam_ctc_workspace_bytes(e.h, 16, 1000, 20, 250) - l.masr_beam_workspace_bytes(e.h, 16, 1000, 20, 250)
    assert need >= 2 * 320 * 250 * 30 * 8


def _tester(tmp_path, monkeypatch, beam_decode, hybrid, **kw):
    return make_tester(tmp_path, monkeypatch, "beam", beam_decode, hybrid=hybrid, **kw)


def test_tester_joint_beam_end_to_end(tmp_path, monkeypatch):
    block = {"beam_size": 8, "att_w": 0.5, "ctc_w": 0.5}
    t, log_dir, sd, cfg = _tester(tmp_path, monkeypatch, block, hybrid=True)
    t.load_data(); t.set_model(); t.exec()
    assert (t.att_weight, t.ctc_weight) == (0.5, 0.5)
    lines = (log_dir / "beam_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6
    eng = MasrEngine(cfg["asr_model"], ODIM)
    eng.load_state_dict(sd)
    want = []
    for idxs in t.eval_set.iter_indices():                     # the Tester's own batches
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        hyps, _ = eng.recog_beam(xs, il, 8, att_weight=0.5, ctc_weight=0.5)
        want += ["{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(str(v) for v in h)) for h, y in zip(hyps, ys)]
    assert lines == want
    # the same block on a plain model: ctc_w is ignored with a notice, the file is the attention beam's
    t, log_dir, _, _ = _tester(tmp_path, monkeypatch, block, hybrid=False)
    t.load_data(); t.set_model(); t.exec()
    assert (t.att_weight, t.ctc_weight) == (1.0, 0.0)
    plain_joint = (log_dir / "beam_decode" / "best-hyp").read_text()
    t, log_dir, _, _ = _tester(tmp_path, monkeypatch, {"beam_size": 8}, hybrid=False)
    t.load_data(); t.set_model(); t.exec()
    assert (log_dir / "beam_decode" / "best-hyp").read_text() == plain_joint


def test_tester_joint_beam_settings(tmp_path, monkeypatch):
    t, _, _, _ = _tester(tmp_path, monkeypatch, {"beam_size": 4, "ctc_w": 0.3}, hybrid=True)
    t.load_data(); t.set_model(); t._beam_settings()
    assert t.ctc_weight == pytest.approx(0.3) and t.att_weight == pytest.approx(0.7)      # att_w defaults to 1 - ctc_w
    t, _, _, _ = _tester(tmp_path, monkeypatch, {"beam_size": 4, "att_w": 0.5}, hybrid=True)
    t.load_data(); t.set_model(); t._beam_settings()
    assert (t.att_weight, t.ctc_weight) == (1.0, 0.0)          # no ctc_w: the attention beam, unchanged
    for bad in ({"ctc_w": -0.5}, {"ctc_w": float("nan")}, {"att_w": -1.0, "ctc_w": 0.5}, {"att_w": float("inf"), "ctc_w": 0.5}, {"ctc_w": 1.5}):
        t, _, _, _ = _tester(tmp_path, monkeypatch, dict(beam_size=4, **bad), hybrid=True)
        t.load_data(); t.set_model()
        with pytest.raises(ValueError, match="beam_decode"):
            t._beam_settings()
