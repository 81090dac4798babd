"""GPU beam search (masr_recog_beam, MasrEngine.recog_beam, Tester --decode_mode beam) against the greedy decode and the CPU
restatement of tests/beam_ref.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import beam_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, make_tester, peaked_state_dict  # noqa: E402
from test_hip_engine import HKUST  # noqa: E402

EOS = ODIM - 1
# Against the CPU restatement: a random-init model with 367 classes has near-flat log-probabilities, so the K-th and (K+1)-th
# candidate of a step are typically 1e-3 nats apart and no utterance has a well-defined beam.  The comparison therefore uses a
# 12-class model whose output projection is scaled by 10 (log-probabilities spread like a trained model's), and the restatement
# runs with the engine's bf16 operand rounding emulated (ref_cpu.bf16_emulation), which leaves summation order as the only
# difference: of the order of 1e-4 nats per log-probability.  DELTA = 0.02 nats keeps a margin of two orders of magnitude over
# that and still leaves most utterances qualified (the test prints how many; the worst score difference is printed too).
DELTA = 0.02


@pytest.fixture(scope="module")
def sd():
    return ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)


@pytest.fixture(scope="module")
def eng(sd):
    e = MasrEngine(TINY, ODIM)
    e.load_state_dict(sd)
    return e


def trimmed_greedy(eng, xs, il):
    g = eng.recog(xs, il).cpu()
    out = []
    for b in range(g.shape[1]):
        t = g[:, b].tolist()
        cut = t.index(EOS, 1) if EOS in t[1:] else len(t)
        out.append(None if t[0] == EOS else t[:cut])        # greedy keeps a leading eos; beam ends empty there
    return out


def test_beam_k1_is_greedy(eng):
    n = 0
    for seed, T in ((11, 64), (12, 48), (13, 37), (14, 52), (15, 61)):
        xs, il, _, _ = synth_batch(seed, [T], [3])
        want = trimmed_greedy(eng, xs, il)[0]
        toks, sc = eng.recog_beam(xs, il, 1)
        if want is None:
            continue
        assert toks[0] == want, (seed, toks[0], want)
        n += 1
    xs, il, _, _ = synth_batch(17, [48] * 6, [3] * 6)      # equal lengths: the greedy batch decodes enc_len steps for everyone
    want = trimmed_greedy(eng, xs, il)
    toks, _ = eng.recog_beam(xs, il, 1)
    for b, w in enumerate(want):
        if w is not None:
            assert toks[b] == w, (b, toks[b], w)
            n += 1
    print(f"K = 1 vs greedy: {n} utterances identical")
    assert n >= 6


def _vs_cpu(eng, sd, cfg, xs, il, K, quant):
    toks, sc = eng.recog_beam(xs, il, K)
    p = ref_cpu.leafify(sd, cfg)
    if quant:
        with ref_cpu.bf16_emulation():
            ref = beam_ref.beam_search(p, cfg, xs, il, K)
    else:
        ref = beam_ref.beam_search(p, cfg, xs, il, K)
    ok = 0
    worst = 0.0
    for b, r in enumerate(ref):
        if beam_ref.min_gap(r) <= DELTA:
            continue
        ok += 1
        assert toks[b] == r["tokens"], (K, b, toks[b], r["tokens"], beam_ref.min_gap(r))
        worst = max(worst, abs(float(sc[b]) - r["score"]))
        assert abs(float(sc[b]) - r["score"]) <= 0.02 + 2e-3 * abs(r["score"]), (K, b, float(sc[b]), r["score"])
    print(f"K = {K}: {ok} of {len(ref)} utterances have every decision gap > {DELTA} nats; tokens identical, worst score diff {worst:.2e}")
    return ok, len(ref)


@pytest.mark.parametrize("K", [4, 20])
def test_beam_vs_cpu_restatement_tiny(K):
    sdp = peaked_state_dict(TINY, 7)
    e = MasrEngine(TINY, C_SMALL)
    e.load_state_dict(sdp)
    ok = n = 0
    for seed, ilens in ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60])):
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        a, b = _vs_cpu(e, sdp, TINY, xs, il, K, quant=True)
        ok += a; n += b
    assert ok >= 0.5 * n, (ok, n)


def test_beam_vs_cpu_restatement_hkust_geometry():
    sdh = peaked_state_dict(HKUST, 3)
    e = MasrEngine(HKUST, C_SMALL)
    e.load_state_dict(sdh)
    torch.manual_seed(3)
    xs = torch.randn(4, 96, 83)
    il = torch.tensor([96, 88, 80, 72])
    ok, n = _vs_cpu(e, sdh, HKUST, xs, il, 4, quant=True)
    assert ok >= 0.5 * n, (ok, n)


def test_beam_batch_independence_and_graph_replay(eng):
    xs, il, _, _ = synth_batch(31, [64, 40, 52, 33, 60], [3] * 5)   # ragged: maxlen 16, 10, 13, 8, 15
    K = 6
    t1, s1 = eng.recog_beam(xs, il, K)
    t2, s2 = eng.recog_beam(xs, il, K)                      # again (direct launches on this stream; graphs: test_hip_decode_graphs.py)
    assert t1 == t2 and torch.equal(s1, s2)
    perm = [3, 0, 4, 2, 1]
    tp, sp = eng.recog_beam(xs[perm], il[perm], K)
    assert tp == [t1[i] for i in perm]
    assert torch.equal(sp, s1[perm])                         # bit for bit
    # each utterance alone (another B: a new capture).  Not bit for bit: the encoder's GEMMs choose their tiling by row count
    # (B * T/4), which moves the memory by bf16-level rounding; the beam itself never mixes utterances
    for b in range(5):
        ta, sa = eng.recog_beam(xs[b:b + 1], il[b:b + 1], K)
        assert ta[0] == t1[b], b
        assert abs(float(sa[0]) - float(s1[b])) <= 2e-4 * max(1.0, abs(float(s1[b])))
    # another K re-captures and still agrees with a fresh engine
    t3, s3 = eng.recog_beam(xs, il, 3)
    fresh = MasrEngine(TINY, ODIM)
    fresh.load_state_dict(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7))
    t4, s4 = fresh.recog_beam(xs, il, 3)
    assert t3 == t4 and torch.equal(s3, s4)
    assert all(len(t) <= int(n) // 4 for t, n in zip(t1, il))


def test_beam_min_max_ratio(eng):
    xs, il, _, _ = synth_batch(41, [64, 40], [3, 3])
    toks, _ = eng.recog_beam(xs, il, 5, min_step_ratio=0.5, max_step_ratio=0.5)
    for t, n in zip(toks, il.tolist()):
        enc = n // 4
        assert enc // 2 <= len(t) <= max(1, enc // 2)       # minlen = maxlen = floor(enc / 2)


def test_beam_errors(eng):
    xs, il, _, _ = synth_batch(11, [40], [3])
    for K in (0, 65):
        with pytest.raises(ValueError):
            eng.recog_beam(xs, il, K)
    import ctypes as C
    l = lib()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    xs_d = xs.cuda().contiguous()
    rc = l.masr_recog_beam(eng.h, C.c_void_p(xs_d.data_ptr()), C.c_void_p(il.data_ptr()), 1, 40, 0, 0.0, 1.0,
                           C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), None)
    assert rc != 0 and b"beam size K must be in [1, 64]" in l.masr_last_error()
    assert l.masr_beam_workspace_bytes(eng.h, 1, 40, 65, 10) < 0 and b"1 <= K <= 64" in l.masr_last_error()


def _tester(*args, **kw):
    return make_tester(*args, **kw)[:2]


def test_tester_beam_end_to_end(tmp_path, monkeypatch):
    t, log_dir = _tester(tmp_path, monkeypatch, "greedy", bs=1)   # alone, greedy decodes each utterance's own enc_len steps
    t.load_data(); t.set_model(); t.exec()
    greedy = (log_dir / "greedy_decode" / "best-hyp").read_text().splitlines()
    t, _ = _tester(tmp_path, monkeypatch, "beam", {"beam_size": 1, "min_step_ratio": 0.0, "max_step_ratio": 1.0, "att_w": 0.5}, bs=1)
    t.load_data(); t.set_model(); t.exec()
    hyp_file = log_dir / "beam_decode" / "best-hyp"
    beam1 = hyp_file.read_text().splitlines()
    assert len(beam1) == len(greedy) == 6
    for g, b in zip(greedy, beam1):
        gr, gh = g.split("\t"); br, bh = b.split("\t")
        assert gr == br
        if gh.split() and int(gh.split()[0]) == EOS:          # the eos-first exception
            assert bh == ""
        else:
            assert gh == bh, (g, b)
    t, _ = _tester(tmp_path, monkeypatch, "beam", {"beam_size": 8}, bs=4)
    t.paras.overwrite = True
    t.load_data(); t.set_model(); t.exec()
    full = hyp_file.read_text()
    lines = full.splitlines()
    assert len(lines) == 6 and all("\t" in l for l in lines)
    for l in lines:
        assert EOS not in [int(x) for x in l.split("\t")[1].split()]
    for keep in (5, 4, 1):
        hyp_file.write_text("".join(l + "\n" for l in lines[:keep]))
        t2, _ = _tester(tmp_path, monkeypatch, "beam", {"beam_size": 8}, resume=True, bs=4)
        assert t2.prev_decode_step == keep
        t2.load_data(); t2.set_model(); t2.exec()
        assert hyp_file.read_text() == full, f"resume after {keep} lines"


def test_tester_beam_errors(tmp_path, monkeypatch):
    t, _ = _tester(tmp_path, monkeypatch, "beam", None)
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="beam_decode"):
        t.exec()
    t, _ = _tester(tmp_path, monkeypatch, "lm_beam", {"beam_size": 4})
    t.load_data(); t.set_model()
    with pytest.raises(NotImplementedError, match="language model"):
        t.exec()
    t, _ = _tester(tmp_path, monkeypatch, "beam", {"beam_size": 0})
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        t.exec()
    t, _ = _tester(tmp_path, monkeypatch, "beam", {"beam_size": 4}, model_name="blstm")
    t.model_name = "blstm"
    with pytest.raises(NotImplementedError, match="transformer"):
        t.exec()
