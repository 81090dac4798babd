"""Contextual phrase biasing of the attention beam and the joint beam through the model (masr_recog_beam_bias, masr_recog_beam_ctc_bias,
MasrEngine.recog_beam_bias / recog_beam_ctc_bias, Tester --decode_mode bias_beam / bias_joint_beam) against the CPU restatement
of tests/bias_beam_ref.py under ref_cpu.bf16_emulation() and against the unbiased searches.

The models are decode_util's TINY hybrid model (joint_state_dict(TINY, 7)) and the same without its CTC head, the cases bias_beam_ref's
(tests/test_bias_beam_ref_cpu.py asserts on the restatement alone that they are fit for the purpose).  The comparison rule is the joint
tests', unchanged: utterances whose every decision gap exceeds decode_util.JOINT_DELTA are compared, tokens equal, scores within
0.1 + 3e-3 |score|, and at least 7 of a case's 9 utterances must qualify.  nbias is exact for every returned entry, whatever its gaps."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_beam_ref as bb  # noqa: E402
import bias_ref  # noqa: E402
import hybrid_ref  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle.make_goldens import ODIM, TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, JOINT_DELTA, joint_engine, make_tester  # noqa: E402
from test_hip_ctc_bias_beam import _arpa, _fmt, _phrase_file, _run  # noqa: E402


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def models():
    return bb._models()


@pytest.fixture(scope="module")
def att_eng(models):
    e = MasrEngine(TINY, C_SMALL)
    e.load_state_dict(models["sd_att"])
    return e


@pytest.fixture(scope="module")
def joint_eng(models):
    return joint_engine(TINY, models["sd"])


@pytest.fixture(scope="module")
def lm(models):
    return NGramLM(3, C_SMALL, *lm_ref.to_arrays(models["lm"]))


def att_decode(eng, cs, lm, bias, bias_w=None, batches=None):
    """-> per utterance (tokens, score, nbias)"""
    out = []
    for xs, il in batches or cs["batches"]:
        t, s, n = eng.recog_beam_bias(xs, il, cs["K"], bias, cs["bias_w"] if bias_w is None else bias_w, lm if cs["with_lm"] else None, cs["lm_w"],
                                      min_step_ratio=cs["minr"])
        out += list(zip(t, s.tolist(), n.tolist()))
    return out


def joint_decode(eng, cs, lm, bias, bias_w=None, batches=None):
    """-> per utterance its N-best [(tokens, score, nbias)]"""
    out = []
    for xs, il in batches or cs["batches"]:
        out += eng.recog_beam_ctc_bias(xs, il, cs["K"], bias, cs["bias_w"] if bias_w is None else bias_w, lm if cs["with_lm"] else None, cs["lm_w"],
                                       cs["len_bonus"], cs["N"], cs["minr"], 1.0, cs["att_w"], cs["ctc_w"])
    return out


@pytest.mark.parametrize("name", list(bb.ATT_CASES))
def test_attention_beam_vs_cpu_restatement(att_eng, lm, name):
    cs = bb.make_case("att", name)
    ref = bb.case_results("att", name)
    bias = ContextBias(C_SMALL, cs["phrases"])
    got = att_decode(att_eng, cs, lm, bias)
    for b, (r, (tok, sc, n)) in enumerate(zip(ref, got)):    # every figure first, then the assertions
        print(f"  utt {b}: gap {bb.att_min_gap(r):.3f}, tokens {tok} / {r['tokens']}, score {sc:.4f} / {r['score']:.4f}, nbias {n} / {r['nbias']}")
    ok = 0
    for b, (r, (tok, sc, n)) in enumerate(zip(ref, got)):
        assert n == bias_ref.count(cs["trie"], tok), (name, b, tok, n)
        if bb.att_min_gap(r) <= JOINT_DELTA:
            continue
        ok += 1
        assert tok == r["tokens"] and n == r["nbias"], (name, b, tok, r["tokens"])
        assert abs(sc - r["score"]) <= 0.1 + 3e-3 * abs(r["score"]), (name, b, sc, r["score"])
    print(f"{name}: {ok} of {len(ref)} utterances qualify")
    assert ok >= 7, (name, ok)


@pytest.mark.parametrize("name", list(bb.JOINT_CASES))
def test_joint_beam_vs_cpu_restatement(joint_eng, lm, name):
    cs = bb.make_case("joint", name)
    ref = bb.case_results("joint", name)
    bias = ContextBias(C_SMALL, cs["phrases"])
    got = joint_decode(joint_eng, cs, lm, bias)
    for b, (r, g) in enumerate(zip(ref, got)):
        print(f"  utt {b}: gap {bb.joint_min_gap(r):.3f}, {g} / {r['nbest']}")
    ok = 0
    for b, (r, g) in enumerate(zip(ref, got)):
        for tok, sc, n in g:
            assert n == bias_ref.count(cs["trie"], tok), (name, b, tok, n)
        if bb.joint_min_gap(r) <= JOINT_DELTA:
            continue
        ok += 1
        assert [(t, n) for t, _, n in g] == [(t, n) for t, _, n in r["nbest"]], (name, b, g, r["nbest"])
        for (_, sc, _), (_, rs, _) in zip(g, r["nbest"]):
            assert abs(sc - rs) <= 0.1 + 3e-3 * abs(rs), (name, b, sc, rs)
    print(f"{name}: {ok} of {len(ref)} utterances qualify")
    assert ok >= 7, (name, ok)


def test_biasing_changes_the_result(att_eng, joint_eng, lm):
    """a no-op cannot pass: some case's best hypothesis differs from the unbiased search's, and credited tokens are reported"""
    changed = credited = 0
    for kind, cases, eng, dec in (("att", bb.ATT_CASES, att_eng, att_decode), ("joint", bb.JOINT_CASES, joint_eng, joint_decode)):
        for name in cases:
            cs = bb.make_case(kind, name)
            bias = ContextBias(C_SMALL, cs["phrases"])
            got, plain = dec(eng, cs, lm, bias), dec(eng, cs, lm, bias, bias_w=0.0)
            first = (lambda g: g[0][0] if g else None) if kind == "joint" else (lambda g: g[0])
            changed += sum(first(a) != first(b) for a, b in zip(got, plain))
            credited += sum((a[0][2] if a else 0) if kind == "joint" else a[2] for a in got)
    print(f"biasing changed {changed} best hypotheses; {credited} credited tokens")
    assert changed >= 1 and credited >= 1


def test_bias_weight_zero_is_the_unbiased_search_bit_for_bit(att_eng, joint_eng, lm, models):
    bias = ContextBias(C_SMALL, bb.make_case("att", "k4_lm")["phrases"])
    for xs, il in models["batches"]:
        for K in (1, 4, 20):
            t0, l0, s0 = att_eng.recog_beam_lm(xs, il, K, lm, 0.5), None, None
            t1, l1, s1, n1 = att_eng.recog_beam_bias(xs, il, K, bias, 0.0, lm, 0.5, raw=True)
            toks = [t1[b, :int(l1[b])].tolist() for b in range(len(il))]
            assert toks == t0[0] and (bits(s1) == bits(t0[1])).all(), K
            # without an LM the row is ranked by lp instead of the logit: equal unless rounding ties the lp of two logits (none does here)
            p0 = att_eng.recog_beam(xs, il, K)
            p1 = att_eng.recog_beam_bias(xs, il, K, bias, 0.0)
            assert p1[0] == p0[0] and (bits(p1[1]) == bits(p0[1])).all(), K
        for K, N, s in ((4, 2, (0.7, 0.3, 0.3, 1.0)), (20, 3, (0.5, 0.5, 0.5, -0.5))):
            a = joint_eng.recog_beam_ctc_lm(xs, il, K, lm, s[2], s[3], N, 0.0, 1.0, s[0], s[1], raw=True)
            b = joint_eng.recog_beam_ctc_bias(xs, il, K, bias, 0.0, lm, s[2], s[3], N, 0.0, 1.0, s[0], s[1], raw=True)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (bits(a[2]) == bits(b[2])).all(), (K, N, s)
            live = b[1] >= 0
            assert (b[3][~live] == -1).all() and (b[3][live] >= 0).all()


def test_permuted_batch(att_eng, joint_eng, lm, models):
    xs, il = models["batches"][0]
    perm = [2, 0, 3, 1]
    xp, ip = xs[perm].contiguous(), il[perm].contiguous()
    cs = bb.make_case("att", "k4_lm")
    bias = ContextBias(C_SMALL, cs["phrases"])
    a, b = att_decode(att_eng, cs, lm, bias, batches=[(xs, il)]), att_decode(att_eng, cs, lm, bias, batches=[(xp, ip)])
    # (T is the longest utterance's either way; the padding behind a shorter one is masked)
    assert [a[i] for i in perm] == b
    cj = bb.make_case("joint", "k6_lm")
    bj = ContextBias(C_SMALL, cj["phrases"])
    a, b = joint_decode(joint_eng, cj, lm, bj, batches=[(xs, il)]), joint_decode(joint_eng, cj, lm, bj, batches=[(xp, ip)])
    assert [a[i] for i in perm] == b


@pytest.mark.parametrize("kind", ["att", "joint"])
def test_repeated_calls_never_replay_stale_values(models, lm, kind):
    """one engine on a side stream (the step graph is captured and replayed there): calls that change bias_w and the list -- one list destroyed and
    another created, possibly at its address -- give what a fresh engine gives on the default stream (direct launches).  The attention beam
    captures anew for another bias_w, the joint beam replays its graph and reads the new value from the device"""
    cs = bb.make_case(kind, "k4_lm" if kind == "att" else "k6_lm")
    other = bb.make_case(kind, "k4")["phrases"] + [[9, 8, 7]]
    make = (lambda: joint_engine(TINY, models["sd"])) if kind == "joint" else (lambda: att_eng_new(models))
    dec = joint_decode if kind == "joint" else att_decode
    batch = [(models["batches"][0][0].cuda(), models["batches"][0][1])]
    seq = [1.5, 4.0, 0.0, 1.5, 0.75]
    fresh = make()
    assert torch.cuda.current_stream().cuda_stream == 0
    b1 = ContextBias(C_SMALL, cs["phrases"])
    want = [dec(fresh, cs, lm, b1, w, batch) for w in seq]
    assert want[0] == want[3] and len({repr(w) for w in want}) >= 3       # the changes matter
    e = make()
    dec(e, cs, lm, b1, 1.5, batch)                          # grows the workspace to its final size on the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [dec(e, cs, lm, b1, w, batch) for w in seq]
        side.synchronize()
        b1.close()                                           # destroy, then another list in its place
        b2 = ContextBias(C_SMALL, other)
        got2 = dec(e, cs, lm, b2, 1.5, batch)
    side.synchronize()
    assert got == want
    want2 = dec(fresh, cs, lm, b2, 1.5, batch)
    assert got2 == want2


def att_eng_new(models):
    e = MasrEngine(TINY, C_SMALL)
    e.load_state_dict(models["sd_att"])
    return e


def test_refusals(models, lm):
    l = lib()
    e = joint_engine(TINY, models["sd"])                     # a fresh workspace
    plain = att_eng_new(models)
    xs, il, _, _ = synth_batch(11, [40], [3])
    xs_d = xs.cuda().contiguous()
    buf = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731
    bias = ContextBias(C_SMALL, [[3, 4], [5]])
    bias13 = ContextBias(13, [[3, 4]])

    def att(eng, lmh, bh, K, lw, bw, nb=buf, ilv=il):
        return l.masr_recog_beam_bias(eng.h, lmh, bh, p(xs_d), p(ilv), 1, 40, K, 0.0, 1.0, lw, bw, p(buf), p(buf), p(buf), p(nb) if nb is not None else None, None)

    def joint(eng, lmh, bh, K, N, aw, cw, lw, bo, bw, nb=buf, ilv=il):
        return l.masr_recog_beam_ctc_bias(eng.h, lmh, bh, p(xs_d), p(ilv), 1, 40, K, N, 0.0, 1.0, aw, cw, lw, bo, bw, p(buf), p(buf), p(buf),
                                          p(nb) if nb is not None else None, None)

    e.recog_beam_ctc_bias(xs, il, 1, bias, 1.0)              # binds workspaces sized for K = 1
    plain.recog_beam_bias(xs, il, 1, bias, 1.0)
    buf.fill_(77)
    nan, inf = float("nan"), float("inf")
    for args, msg in (((lm.h, None, 4, 0.3, 1.0), b"null phrase list"), ((lm.h, bias13.h, 4, 0.3, 1.0), b"phrase list's classes differ"),
                      ((lm.h, bias.h, 4, 0.3, -0.5), b"bias_w"), ((None, bias.h, 4, 0.3, nan), b"bias_w"), ((lm.h, bias.h, 4, 0.3, inf), b"bias_w"),
                      ((lm.h, bias.h, 4, -0.3, 1.0), b"lm_w"), ((lm.h, bias.h, 4, nan, 1.0), b"lm_w"),
                      ((lm.h, bias.h, 0, 0.3, 1.0), b"beam size K must be in [1, 64]"), ((None, bias.h, 65, 0.3, 1.0), b"beam size K must be in [1, 64]")):
        assert att(plain, *args) == -1 and msg in l.masr_last_error(), (args, l.masr_last_error())
    assert att(plain, lm.h, bias.h, 4, 0.3, 1.0, nb=None) == -1 and b"null pointer" in l.masr_last_error()
    il_bad = torch.tensor([3], dtype=torch.int64)
    assert att(plain, lm.h, bias.h, 4, 0.3, 1.0, ilv=il_bad) != 0 and b"ilens must be in [4, T]" in l.masr_last_error()
    for args, msg in (((lm.h, None, 4, 1, 0.5, 0.5, 0.3, 0.0, 1.0), b"null phrase list"), ((None, bias13.h, 4, 1, 0.5, 0.5, 0.3, 0.0, 1.0), b"phrase list's classes differ"),
                      ((lm.h, bias.h, 4, 1, 0.5, 0.5, 0.3, 0.0, -1.0), b"bias_w"), ((lm.h, bias.h, 4, 1, 0.5, 0.5, 0.3, 0.0, nan), b"bias_w"),
                      ((lm.h, bias.h, 4, 1, 0.5, 0.0, 0.3, 0.0, 1.0), b"ctc_w"), ((None, bias.h, 4, 1, -0.1, 0.5, 0.3, 0.0, 1.0), b"att_w"),
                      ((lm.h, bias.h, 4, 1, 0.5, 0.5, -0.3, 0.0, 1.0), b"lm_w"), ((lm.h, bias.h, 4, 1, 0.5, 0.5, 0.3, nan, 1.0), b"len_bonus"),
                      ((None, bias.h, 4, 1, 0.5, 0.5, 0.3, inf, 1.0), b"len_bonus"),
                      ((lm.h, bias.h, 4, 0, 0.5, 0.5, 0.3, 0.0, 1.0), b"N must be in [1, K]"), ((None, bias.h, 4, 5, 0.5, 0.5, 0.3, 0.0, 1.0), b"N must be in [1, K]"),
                      ((lm.h, bias.h, 65, 1, 0.5, 0.5, 0.3, 0.0, 1.0), b"beam size K must be in [1, 64]")):
        assert joint(e, *args) == -1 and msg in l.masr_last_error(), (args, l.masr_last_error())
    assert joint(plain, None, bias.h, 4, 1, 0.5, 0.5, 0.3, 0.0, 1.0) == -1 and b"no CTC head" in l.masr_last_error()
    assert joint(e, lm.h, bias.h, 4, 1, 0.5, 0.5, 0.3, 0.0, 1.0, nb=None) == -1 and b"null pointer" in l.masr_last_error()
    xl = torch.zeros(1, 4000, 83, device="cuda:0")               # K = 64 over 1000 frames: far beyond the K = 1 workspaces
    il_l = torch.tensor([4000], dtype=torch.int64)
    assert l.masr_recog_beam_bias(plain.h, None, bias.h, p(xl), p(il_l), 1, 4000, 64, 0.0, 1.0, 0.0, 1.0, p(buf), p(buf), p(buf), p(buf), None) == -2
    assert b"masr_beam_bias_workspace_bytes" in l.masr_last_error()
    assert l.masr_recog_beam_ctc_bias(e.h, lm.h, bias.h, p(xl), p(il_l), 1, 4000, 64, 4, 0.0, 1.0, 0.5, 0.5, 0.3, 0.0, 1.0, p(buf), p(buf), p(buf), p(buf),
                                      None) == -2
    assert b"masr_beam_ctc_bias_workspace_bytes" in l.masr_last_error()
    torch.cuda.synchronize()
    assert (buf == 77).all()                                 # nothing was launched: no output was written
    # the workspaces: the LM variants' plus the states [2][R] and, joint, the bias terms [R][P], each rounded up to 256 bytes
    up = lambda n: (n + 255) // 256 * 256                     # noqa: E731
    B, T, K, N, Lmax = 16, 1000, 20, 20, 250
    R, Pw = B * K, 3 * K // 2
    assert l.masr_beam_bias_workspace_bytes(plain.h, B, T, K, Lmax) == l.masr_beam_lm_workspace_bytes(plain.h, B, T, K, Lmax) + up(2 * R * 8)
    assert l.masr_beam_ctc_bias_workspace_bytes(e.h, B, T, K, N, Lmax) == \
        l.masr_beam_ctc_lm_workspace_bytes(e.h, B, T, K, N, Lmax) + up(2 * R * 8) + up(R * Pw * 4)
    assert l.masr_beam_ctc_bias_workspace_bytes(plain.h, B, T, K, N, Lmax) < 0 and b"no CTC head" in l.masr_last_error()
    for bad in ((0, 40, 4, 10), (1, 3, 4, 10), (1, 40, 65, 10), (1, 40, 4, 0)):
        assert l.masr_beam_bias_workspace_bytes(plain.h, *bad) < 0
    with pytest.raises(ValueError, match="bias_w"):
        plain.recog_beam_bias(xs, il, 4, bias, -1.0)
    with pytest.raises(ValueError, match="live ContextBias"):
        e.recog_beam_ctc_bias(xs, il, 4, None, 1.0)
    with pytest.raises(MasrError, match="no CTC head"):
        plain.recog_beam_ctc_bias(xs, il, 4, bias, 1.0)


PHRASES = bias_ref.toy_phrases(ODIM, 40, 2, 4)


def _hyp_lines(log_dir, mode):
    lines = (log_dir / f"{mode}_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6 and all("\t" in ln for ln in lines)
    return lines


@pytest.mark.parametrize("with_lm", [False, True])
def test_tester_bias_beam_modes(tmp_path, monkeypatch, with_lm):
    arpa = str(_arpa(tmp_path)) if with_lm else None
    ctx = _phrase_file(tmp_path, PHRASES)

    def tester(mode, block, hybrid, path=ctx, **kw):
        t, log_dir, sd, cfg = make_tester(tmp_path, monkeypatch, mode, block, hybrid=hybrid, bs=4, **kw)
        t.paras.lm_model_path, t.paras.context_path = arpa, path
        return t, log_dir

    bias = ContextBias(ODIM, PHRASES)
    # bias_beam on a plain model; ctc_w is logged as ignored there
    bd = {"beam_size": 4, "lm_w": 0.6, "bias_w": 2.5, "ctc_w": 0.4}
    t, log_dir = tester("bias_beam", bd, False)
    _run(t)
    lm = NGramLM.from_arpa(arpa, t.id2ch) if with_lm else None
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        toks = t.asr_model.engine.recog_beam_bias(xs, il, 4, bias, 2.5, lm, 0.6)[0]
        want += [_fmt(y, h) for h, y in zip(toks, ys)]
    assert _hyp_lines(log_dir, "bias_beam") == want
    assert t.bias_weight == 2.5 and (t.lm is None) == (not with_lm)
    # bias_joint_beam on a hybrid model
    bd = {"beam_size": 4, "nbest": 2, "lm_w": 0.6, "len_bonus": 0.5, "ctc_w": 0.4, "bias_w": 2.5}
    t, log_dir = tester("bias_joint_beam", bd, True)
    _run(t)
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, _ = t.eval_set.materialize(idxs)
        lists = t.asr_model.engine.recog_beam_ctc_bias(xs, il, 4, bias, 2.5, lm, 0.6, 0.5, 2, 0.0, 1.0, 0.6, 0.4)
        want += [_fmt(y, n[0][0] if n else []) for n, y in zip(lists, ys)]
    assert _hyp_lines(log_dir, "bias_joint_beam") == want
    assert t.nbest == 2 and t.ctc_weight == 0.4 and abs(t.att_weight - 0.6) < 1e-12 and t.len_bonus == 0.5
    if with_lm:
        return
    # what the modes refuse, before anything is decoded
    for mode, block, hybrid, path, exc, pat in (
            ("bias_beam", {"beam_size": 4, "ctc_w": 0.4}, True, ctx, ValueError, "bias_joint_beam"),
            ("bias_joint_beam", {"beam_size": 4, "ctc_w": 0.4}, False, ctx, ValueError, "needs a CTC output layer"),
            ("bias_joint_beam", {"beam_size": 4}, True, ctx, ValueError, "ctc_w must be > 0"),
            ("bias_beam", {"beam_size": 4}, False, None, NotImplementedError, "no phrase list given; pass --context_path"),
            ("bias_joint_beam", {"beam_size": 4, "ctc_w": 0.4}, True, None, NotImplementedError, "no phrase list given; pass --context_path"),
            ("bias_beam", {"beam_size": 4, "bias_w": -0.5}, False, ctx, ValueError, "bias_w"),
            ("bias_joint_beam", {"beam_size": 4, "ctc_w": 0.4, "nbest": 5}, True, ctx, ValueError, "nbest")):
        t, log_dir = tester(mode, block, hybrid, path)
        t.load_data(); t.set_model()
        with pytest.raises(exc, match=pat):
            t.exec()
        assert not (log_dir / f"{mode}_decode" / "best-hyp").exists()
