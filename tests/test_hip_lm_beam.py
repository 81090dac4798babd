"""n-gram LM shallow fusion through the model (masr_recog_beam_lm, MasrEngine.recog_beam_lm, Tester --decode_mode lm_beam)
against the CPU restatement of tests/lm_ref.py and against the plain beam.

The toy model is decode_util.peaked_state_dict(TINY, 7) (12 classes, projection x 10) with char_trans.bias[0] = -30 as in joint_state_dict:
without the lowered bias it emits class 0 at log-prob ~ 0 up to maxlen and no LM changes anything.  The comparison rule is
test_hip_beam.py's, unchanged: utterances whose every decision gap exceeds DELTA = 0.02 nats are compared, tokens equal, score within
0.02 + 2e-3 |score|, and enough utterances must qualify.

The LM is lm_ref's toy trigram model; its seed is picked on the CPU restatement alone, by three criteria.
(a) At lm_w <= 1 the decoded hypotheses do not end in eos.  The random decoder never prefers eos (log-prob -7 .. -9.5 at the first step) and
there is no length bonus, so an LM that charges the decoder's own tokens ~4.6 nats each (most seeds: they are unseen n-grams) makes the
empty hypothesis win everywhere, and the compared score is then lp(eos | sos) + one LM term.  The rule's tolerance was set for scores made
of probable classes' log-probs; an improbable class's log-prob is a different quantity: with the projection scaled by 10, bf16 operand
rounding alone moves lp(eos | sos) by 0.001 .. 0.126 nats between the restatement with and without ref_cpu.bf16_emulation(), the top class's
by <= 2e-3 (measured with seed 3, where the engine and the restatement agreed on all tokens and differed by 0.002 .. 0.090 nats in those
scores).  Of the seeds 0 .. 399, 276 is the second cheapest for the decoder's preferred sequence (7.8 nats for 16 tokens); the hypotheses keep
their 8 .. 16 tokens and each score carries that many full-context trigram terms instead of one.
(b) At least 6 of the 9 utterances have every decision gap > DELTA at each (K, lm_w): 9, 8, 8 and 7 at (4, 0.5), (20, 0.5), (4, 1.0), (20, 1.0)
(the cheapest seed, 172, has 3 at (20, 0.5)).
(c) The LM changes the decoded tokens of at least half of the utterances at some weight: 6 of 9 at lm_w = 4 (the per-token cost then ends
them early)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import beam_ref  # noqa: E402
import lm_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from masr_amd.lm import NGramLM  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, make_tester, peaked_state_dict  # noqa: E402

DELTA = 0.02
LM_SEED = 276
BATCHES = ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60]))      # those of test_beam_vs_cpu_restatement_tiny


def toy_state_dict():
    sd = peaked_state_dict(TINY, 7)
    sd["char_trans.bias"] = sd["char_trans.bias"].clone()
    sd["char_trans.bias"][0] = -30.0
    return sd


@pytest.fixture(scope="module")
def sd():
    return toy_state_dict()


@pytest.fixture(scope="module")
def eng(sd):
    e = MasrEngine(TINY, C_SMALL)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def lm_dict():
    return lm_ref.toy_lm(C_SMALL, 3, LM_SEED)


@pytest.fixture(scope="module")
def lm(lm_dict):
    return NGramLM(3, C_SMALL, *lm_ref.to_arrays(lm_dict))


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in BATCHES]


_REF = {}


def reference(sd, lm_dict, batches, K, lm_w, minr=0.0):
    """the restatement's results for all nine utterances under the engine's bf16 operand rounding; computed once per setting"""
    key = (K, lm_w, minr)
    if key not in _REF:
        p = ref_cpu.leafify(sd, TINY)
        with ref_cpu.bf16_emulation():
            _REF[key] = [r for xs, il in batches for r in lm_ref.beam_search_lm(p, TINY, xs, il, K, lm_dict, lm_w, min_step_ratio=minr)]
    return _REF[key]


def decode(eng, lm, batches, K, lm_w, minr=0.0):
    toks, scores = [], []
    for xs, il in batches:
        t, s = eng.recog_beam_lm(xs, il, K, lm, lm_w, min_step_ratio=minr)
        toks += t; scores += s.tolist()
    return toks, scores


@pytest.mark.parametrize("K, lm_w, minr", [(4, 0.5, 0.0), (20, 0.5, 0.0), (4, 1.0, 0.0), (20, 1.0, 0.0), (4, 0.5, 0.5), (4, 1.0, 0.5)])
def test_lm_beam_vs_cpu_restatement(eng, sd, lm, lm_dict, batches, K, lm_w, minr):
    ref = reference(sd, lm_dict, batches, K, lm_w, minr)
    toks, scores = decode(eng, lm, batches, K, lm_w, minr)
    ok, worst = 0, 0.0
    for b, r in enumerate(ref):                             # every figure first, then the assertions
        print(f"  utt {b}: gap {beam_ref.min_gap(r):.3f}, tokens {toks[b]} / {r['tokens']}, score {scores[b]:.4f} / {r['score']:.4f}, "
              f"diff {abs(scores[b] - r['score']):.4f}, bound {0.02 + 2e-3 * abs(r['score']):.4f}")
    for b, r in enumerate(ref):
        if beam_ref.min_gap(r) <= DELTA:
            continue
        ok += 1
        assert toks[b] == r["tokens"], (K, lm_w, b, toks[b], r["tokens"], beam_ref.min_gap(r))
        worst = max(worst, abs(scores[b] - r["score"]))
        assert abs(scores[b] - r["score"]) <= 0.02 + 2e-3 * abs(r["score"]), (K, lm_w, b, scores[b], r["score"])
    print(f"K = {K}, lm_w = {lm_w}, min ratio {minr}: {ok} of {len(ref)} utterances have every decision gap > {DELTA} nats; tokens identical, "
          f"worst score diff {worst:.2e}; lengths {[len(t) for t in toks]}")
    assert ok >= 6, (ok, len(ref))                          # 9, 8, 8, 7 (and 9, 9) on the CPU restatement: >= 6 of 9, more than half
    if minr > 0:
        assert all(len(t) >= 4 for t in toks)


def test_lm_changes_the_result(eng, lm, batches):
    """a no-op cannot pass: the fused search decodes other tokens than the plain beam in at least half of the utterances, and where
    min_step_ratio keeps the hypotheses long their scores carry the LM terms"""
    plain = [t for xs, il in batches for t in eng.recog_beam(xs, il, 4)[0]]
    fused, _ = decode(eng, lm, batches, 4, 4.0)              # (at lm_w <= 1 this LM agrees with the decoder: the module's docstring)
    n = sum(a != b for a, b in zip(plain, fused))
    print(f"the LM changes {n} of {len(plain)} hypotheses")
    assert n >= 5
    ps = [float(s) for xs, il in batches for s in eng.recog_beam(xs, il, 4, min_step_ratio=0.5)[1]]
    _, fs = decode(eng, lm, batches, 4, 1.0, 0.5)
    assert all(f < p - 1.0 for f, p in zip(fs, ps)), (fs, ps)   # >= 4 tokens at an LM cost of more than 0.25 nats each


def test_lm_weight_zero_is_the_plain_beam(eng, lm, batches):
    # (a rounding tie that made one f of two logits could change tokens here; none does on these seeds, and lm_ref shows it on the CPU:
    # tests/test_lm_ref_cpu.py test_search_at_weight_zero_is_the_plain_beam)
    for K in (1, 4, 20):
        for xs, il in batches:
            t0, s0 = eng.recog_beam(xs, il, K)
            t1, s1 = eng.recog_beam_lm(xs, il, K, lm, 0.0)
            assert t1 == t0, (K, t0, t1)
            assert torch.equal(s1.view(torch.int32), s0.view(torch.int32)), (K, s0, s1)


def test_lm_beam_k1_is_fused_greedy(eng, sd, lm, lm_dict, batches):
    p = ref_cpu.leafify(sd, TINY)
    n = 0
    for lm_w, minr in ((0.5, 0.0), (2.0, 0.5)):
        gaps = reference(sd, lm_dict, batches, 1, lm_w, minr)
        with ref_cpu.bf16_emulation():
            greedy = [g for xs, il in batches for g in lm_ref.greedy_lm(p, TINY, xs, il, lm_dict, lm_w, min_step_ratio=minr)]
        toks, scores = decode(eng, lm, batches, 1, lm_w, minr)
        for b, (r, (gt, gs)) in enumerate(zip(gaps, greedy)):
            assert r["tokens"] == gt                        # the restatement at K = 1 is the arg-max chain
            if beam_ref.min_gap(r) <= DELTA:
                continue
            n += 1
            assert toks[b] == gt, (lm_w, b, toks[b], gt)
            assert abs(scores[b] - gs) <= 0.02 + 2e-3 * abs(gs)
    print(f"K = 1 vs fused arg-max: {n} of 18 utterances compared")
    assert n >= 9


def test_lm_beam_batch_independence(eng, lm):
    xs, il, _, _ = synth_batch(31, [64, 40, 52, 33, 60], [3] * 5)
    t1, s1 = eng.recog_beam_lm(xs, il, 6, lm, 0.7, min_step_ratio=0.3)
    t2, s2 = eng.recog_beam_lm(xs, il, 6, lm, 0.7, min_step_ratio=0.3)
    assert t1 == t2 and torch.equal(s1, s2)
    perm = [3, 0, 4, 2, 1]
    tp, sp = eng.recog_beam_lm(xs[perm], il[perm], 6, lm, 0.7, min_step_ratio=0.3)
    assert tp == [t1[i] for i in perm]
    assert torch.equal(sp, s1[perm])                         # bit for bit
    assert any(len(t) > 0 for t in t1)


def test_changing_lm_or_weight_never_replays_the_old_graph(eng, lm, lm_dict, monkeypatch):
    """calls that share B, T, K and Lmax and differ in lm_w or in the LM: on a side stream each is a step graph, and each must give what
    its direct launches give; a plain beam behind them is untouched"""
    monkeypatch.delenv("MASR_RECOG_NO_GRAPH", raising=False)
    other = lm_ref.toy_lm(C_SMALL, 2, LM_SEED + 1)
    lm2 = NGramLM(2, C_SMALL, *lm_ref.to_arrays(other))
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    xs = xs.cuda()
    calls = [(lm, 0.5), (lm, 1.5), (lm, 0.5), (lm2, 1.5), (lm, 1.5), (None, 0.0), (lm2, 0.5), (None, 0.0)]

    def run():
        out = []
        for m, w in calls:
            out.append(eng.recog_beam(xs, il, 4, min_step_ratio=0.5) if m is None else eng.recog_beam_lm(xs, il, 4, m, w, min_step_ratio=0.5))
        return out

    assert torch.cuda.current_stream().cuda_stream == 0       # the NULL stream: direct launches
    direct = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphs = run()
    side.synchronize()
    for c, (t0, s0), (t1, s1) in zip(calls, direct, graphs):
        assert t1 == t0 and torch.equal(s1, s0), (c[1], t0, t1, s0, s1)
    # the settings differ in their results, so a replay of the wrong graph would have shown
    distinct = {(id(m), w): repr(s.tolist()) for (m, w), (_, s) in zip(calls, direct)}
    assert len(set(distinct.values())) == len(distinct) == 5, distinct
    assert direct[5][0] == direct[7][0] and torch.equal(direct[5][1], direct[7][1])
    lm2.close()
    assert lm2.h is None


def test_lm_beam_errors(eng, lm):
    xs, il, _, _ = synth_batch(11, [40], [3])
    for K in (0, 65):
        with pytest.raises(ValueError):
            eng.recog_beam_lm(xs, il, K, lm, 0.5)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_w"):
            eng.recog_beam_lm(xs, il, 4, lm, w)
    wide = lm_ref.toy_lm(C_SMALL + 1, 2, 1)
    lm13 = NGramLM(2, C_SMALL + 1, *lm_ref.to_arrays(wide))
    with pytest.raises(MasrError, match="odim"):
        eng.recog_beam_lm(xs, il, 4, lm13, 0.5)
    import ctypes as C
    l = lib()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    xs_d = xs.cuda().contiguous()
    args = (C.c_void_p(xs_d.data_ptr()), C.c_void_p(il.data_ptr()), 1, 40)
    out = (C.c_void_p(buf.data_ptr()),) * 3 + (None,)
    assert l.masr_recog_beam_lm(eng.h, lm.h, *args, 0, 0.0, 1.0, 0.5, *out) != 0 and b"beam size K must be in [1, 64]" in l.masr_last_error()
    assert l.masr_recog_beam_lm(eng.h, lm.h, *args, 4, 0.0, 1.0, -1.0, *out) != 0 and b"lm_w must be finite and >= 0" in l.masr_last_error()
    assert l.masr_recog_beam_lm(eng.h, lm.h, *args, 4, 0.0, 1.0, float("nan"), *out) != 0 and b"lm_w" in l.masr_last_error()
    assert l.masr_recog_beam_lm(eng.h, None, *args, 4, 0.0, 1.0, 0.5, *out) != 0 and b"null language model" in l.masr_last_error()
    assert l.masr_beam_lm_workspace_bytes(eng.h, 1, 40, 65, 10) < 0 and b"1 <= K <= 64" in l.masr_last_error()
    # the workspace: the beam's plus the fp32 fused rows [B*K][Cp] (each plan entry is rounded up to 256 bytes)
    for B, K in ((1, 1), (3, 20)):
        extra = l.masr_beam_lm_workspace_bytes(eng.h, B, 40, K, 10) - l.masr_beam_workspace_bytes(eng.h, B, 40, K, 10)
        assert extra == (B * K * 128 * 4 + 255) // 256 * 256, (B, K, extra)


# ---------------------------------------------------------------- Tester
def _arpa(tmp_path, seed=5):
    m10 = lm_ref.toy_lm_log10(ODIM, 3, seed, n_sent=120, max_len=10, active=40)
    path = tmp_path / "toy.arpa"
    path.write_text(lm_ref.arpa_text(m10, lm_ref.units(ODIM)))
    return path


def test_tester_lm_beam_end_to_end(tmp_path, monkeypatch):
    bd = {"beam_size": 4, "lm_w": 0.6, "min_step_ratio": 0.3}
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", bd, bs=4)
    t.paras.lm_model_path = str(_arpa(tmp_path))
    t.load_data(); t.set_model(); t.exec()
    lines = (log_dir / "lm_beam_decode" / "best-hyp").read_text().splitlines()
    assert len(lines) == 6 and all("\t" in l for l in lines)
    for l in lines:
        assert ODIM - 1 not in [int(x) for x in l.split("\t")[1].split()]
    assert t.lm.order == 3 and t.lm_weight == 0.6
    want = []
    lm = NGramLM.from_arpa(t.paras.lm_model_path, t.id2ch)
    for idxs in t.eval_set.iter_indices():
        xs, ilens, ys, _ = t.eval_set.materialize(idxs)
        hyps, _ = t.asr_model.engine.recog_beam_lm(xs, ilens, 4, lm, 0.6, min_step_ratio=0.3)
        want += ["{}\t{}".format(" ".join(str(i) for i in y.tolist()), " ".join(str(i) for i in h)) for y, h in zip(ys, hyps)]
    assert lines == want
    assert any(l.split("\t")[1] for l in lines)


def test_tester_lm_beam_refusals(tmp_path, monkeypatch):
    arpa = str(_arpa(tmp_path))
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4, "ctc_w": 0.5}, hybrid=True)
    t.paras.lm_model_path = arpa
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="ctc_w: 0"):
        t.exec()
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4}, hybrid=True)     # ctc_w absent: the attention beam
    t.paras.lm_model_path = arpa
    t.load_data(); t.set_model(); t.exec()
    assert len((log_dir / "lm_beam_decode" / "best-hyp").read_text().splitlines()) == 6
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4}, model_name="blstm")
    t.model_name = "blstm"
    t.paras.lm_model_path = arpa
    with pytest.raises(NotImplementedError, match="transformer"):
        t.exec()
    broken = tmp_path / "broken.arpa"
    broken.write_text((tmp_path / "toy.arpa").read_text().replace("\\2-grams:", "\\4-grams:"))
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4})
    t.paras.lm_model_path = str(broken)
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="line"):
        t.exec()
    t, _, _, _ = make_tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4, "lm_w": -1})
    t.paras.lm_model_path = arpa
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="lm_w"):
        t.exec()
