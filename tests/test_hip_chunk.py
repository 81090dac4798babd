"""The chunk mask of the encoder's self-attention through the engine (asr_model.chunk, include/masr.h masr_set_chunk) on the GPU: training
and evaluation steps against the chunked oracle (tests/chunk_ref.py) with the bounds tests/test_hip_engine.py and tests/test_hip_hybrid_ctc.py
apply to the same comparison without a chunk, that no output frame in front of a chunk's end depends on later audio, decoding, the dynamic
policy's draw (direct launches and replayed step graphs) and switching the policy on and off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import beam_ref  # noqa: E402
import chunk_ref as R  # noqa: E402
import ctc_beam_ref as cr  # noqa: E402
import hybrid_ref  # noqa: E402
from masr_amd._cabi import MasrError  # noqa: E402
from masr_amd.engine import MasrEngine, chunk_draw  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402
from decode_util import C_SMALL, JOINT_DELTA, joint_state_dict, make_tester, peaked_state_dict  # noqa: E402
from test_chunk_ref_cpu import GPU_EPS, GPU_ILENS, GPU_OLENS, GPU_POLICIES, GPU_SEED, GPU_W  # noqa: E402

HEAD = hybrid_ref.HEAD


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cmp(a, b, n):
    a = a.cpu()
    if n.endswith("in_proj_bias"):
        E = TINY["d_model"]                                      # key-bias third has zero true gradient
        a = torch.cat([a[:E], a[2 * E:]]); b = torch.cat([b[:E], b[2 * E:]])
    return rel_l2(a, b)


@pytest.fixture(scope="module")
def sd():
    return ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7)


@pytest.fixture(scope="module")
def sdh(sd):
    return hybrid_ref.with_head(sd, ODIM, seed=3)


def engine(sd, policy, hybrid=False, dropout=0.0, seed=77, odim=ODIM, eps=GPU_EPS):
    cfg = dict(TINY, dropout=dropout, pos_dropout=dropout)
    if hybrid:
        cfg["ctc_weight"] = GPU_W
    if policy is not None:
        cfg["chunk"] = policy
    e = MasrEngine(cfg, odim, label_smoothing=eps)
    e.load_state_dict(sd); e.set_seed(seed)
    return e


def oracle(sd, hybrid, quant, pol, batch):
    """-> (info, grads, logits) of the chunked oracle, fp32 or with the engine's bf16 rounding points"""
    xs, il, ys, ol = batch
    import contextlib
    with R.chunked_oracle(pol["size"], pol["left"]), (ref_cpu.bf16_emulation() if quant else contextlib.nullcontext()):
        if hybrid:
            p = hybrid_ref.leafify(sd, TINY)
            info, grads = hybrid_ref.run_batch_train(p, TINY, (xs, il, ys, ol), GPU_EPS, GPU_W)
            with torch.no_grad():
                logit, _ = ref_cpu.model_forward(p, TINY, xs, il, ys, ol.clone())
        else:
            p = ref_cpu.leafify(sd, TINY)
            info, grads, logit, _ = ref_cpu.run_batch_train(p, TINY, (xs, il, ys, ol.clone()), GPU_EPS)
    return info, grads, logit.detach()


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("pi", range(len(GPU_POLICIES)))
def test_run_batch_vs_the_chunked_oracle(sd, sdh, hybrid, pi):
    """Bounds copied from test_hip_engine.py::test_run_batch_vs_oracle_and_golden and test_hip_hybrid_ctc.py::test_run_batch_vs_restatement:
    loss 1e-3 (fp32 oracle) and 2e-4 (bf16-emulating oracle), logits 4e-3, every gradient 8e-2 (0.15 against the fp32 oracle), cosine 0.999,
    norm 1e-2.  tests/test_chunk_ref_cpu.py shows that an encoder that ignored the policy would miss the loss (hybrid) / logit (plain) bound
    tenfold."""
    pol, weights = GPU_POLICIES[pi], sdh if hybrid else sd
    batch = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    xs, il, ys, ol = batch
    eng = engine(weights, pol, hybrid)
    eng.run_batch(xs, il, ys, ol, train=True)
    st = eng.read_stats()
    assert eng.chunk_last() == pol["size"] and eng.chunk == pol
    lg, _ = eng.last_logits()
    lg = lg.cpu().clone()
    g_all = {n: t.cpu() for n, t in eng.state_dict(flat=eng.grads).items()}
    info, grads, _ = oracle(weights, hybrid, False, pol, batch)
    infoq, gradsq, logitq = oracle(weights, hybrid, True, pol, batch)
    names = list(gradsq) if hybrid else ref_cpu.grad_param_names(ref_cpu.leafify(sd, TINY), TINY)
    r32 = abs(st["loss"] - info["loss"]) / info["loss"]
    r16 = abs(st["loss"] - infoq["loss"]) / infoq["loss"]
    rlg = rel_l2(lg[..., :ODIM].reshape(logitq.shape), logitq)
    worst32 = max(_cmp(g_all[n], grads[n], n) for n in names)
    per = {n: _cmp(g_all[n], gradsq[n], n) for n in names}
    worst_n = max(per, key=per.get)
    flat_a = torch.cat([g_all[n].reshape(-1) for n in names if not n.endswith("in_proj_bias")]).double()
    flat_b = torch.cat([gradsq[n].reshape(-1) for n in names if not n.endswith("in_proj_bias")]).double()
    cos = float((flat_a * flat_b).sum() / (flat_a.norm() * flat_b.norm()))
    rnorm = abs(float(flat_a.norm()) - float(flat_b.norm())) / float(flat_b.norm())
    # evaluation runs under the same chunk and leaves the gradients alone
    eng.grads.fill_(3.0)
    eng.run_batch(xs, il, ys, ol, train=False)
    se = eng.read_stats()
    le, _ = eng.last_logits()
    e16 = abs(se["loss"] - infoq["loss"]) / infoq["loss"]
    elg = rel_l2(le.cpu()[..., :ODIM].reshape(logitq.shape), logitq)
    print(f"hybrid {hybrid} {pol}: train loss rel {r32:.2e} (bound 1e-3) / bf16 oracle {r16:.2e} (2e-4), logits {rlg:.2e} (4e-3), worst gradient "
          f"{per[worst_n]:.4f} {worst_n} (8e-2), fp32 oracle {worst32:.4f} (0.15), cos {cos:.6f} (0.999), norm {rnorm:.2e} (1e-2); "
          f"eval loss {e16:.2e} (2e-4), logits {elg:.2e} (4e-3)")
    assert st["n_total"] == sum(GPU_OLENS) + len(GPU_OLENS)
    assert r32 <= 1e-3 and r16 <= 2e-4, (st["loss"], info["loss"], infoq["loss"])
    assert rlg < 4e-3
    assert per[worst_n] < 8e-2, (worst_n, per[worst_n])
    assert worst32 < 0.15 and cos > 0.999 and rnorm < 1e-2
    assert e16 <= 2e-4 and elg < 4e-3 and eng.chunk_last() == pol["size"] and bool((eng.grads == 3.0).all())


def test_no_frame_before_a_chunk_end_depends_on_later_audio(sdh):
    """T = 160 (40 encoder frames), chunk 8: the CTC head's logits of the frames < E keep their bits when the input changes from frame 4 E + 6
    on (encoder frame t reads the input frames <= 4 t + 9: tests/test_chunk_ref_cpu.py) -- and under full context frame E - 1 does change"""
    xs, il, _, _ = synth_batch(11, [160, 160], [3, 3])
    B, T, K = 2, 160, 4
    for pol, independent in ((dict(size=8), True), (dict(size=8, left=1), True), (None, False)):
        eng = engine(sdh, pol, hybrid=True)
        eng.recog_ctc_beam(xs, il, K, 1)
        base = eng.last_ctc_beam_logits(B, T, K)[0][..., :ODIM].clone()
        assert eng.chunk_last() == (8 if pol else 0)
        for E in (8, 24):
            x2 = xs.clone()
            x2[:, 4 * E + 6:] = torch.randn(B, T - 4 * E - 6, xs.shape[2], generator=torch.Generator().manual_seed(E))
            eng.recog_ctc_beam(x2, il, K, 1)
            got = eng.last_ctc_beam_logits(B, T, K)[0][..., :ODIM]
            assert not same_bits(got[:, E:], base[:, E:])
            if independent:
                assert same_bits(got[:, :E], base[:, :E]), (pol, E)
            else:
                assert not same_bits(got[:, E - 1], base[:, E - 1]), E


def test_greedy_decode_under_a_chunk_vs_the_restatement():
    """masr_recog under size 8 against beam_ref at K = 1 (the greedy decode: test_hip_beam.py::test_beam_k1_is_greedy) on the chunked oracle;
    the model, DELTA and the share of utterances are test_hip_beam.py's"""
    DELTA, EOS = 0.02, C_SMALL - 1
    sdp = peaked_state_dict(TINY, 7)
    eng = engine(sdp, dict(size=8), odim=C_SMALL, eps=0.0)
    ok = n = 0
    for seed, ilens in ((12, [128, 100, 72, 60]), (13, [96, 80, 64]), (14, [160, 96, 64, 40])):
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        hyp = eng.recog(xs, il).cpu()
        assert eng.chunk_last() == 8
        with R.chunked_oracle(8), ref_cpu.bf16_emulation(), torch.no_grad():
            ref = beam_ref.beam_search(ref_cpu.leafify(sdp, TINY), TINY, xs, il, 1)
        for b, r in enumerate(ref):
            n += 1
            if beam_ref.min_gap(r) <= DELTA:
                continue
            t = hyp[:ilens[b] // 4, b].tolist()
            cut = t.index(EOS, 1) if EOS in t[1:] else len(t)
            if t[0] == EOS:
                continue                                         # (greedy keeps a leading eos; the beam ends empty there)
            ok += 1
            assert t[:cut] == r["tokens"], (seed, b, t[:cut], r["tokens"], beam_ref.min_gap(r))
    print(f"greedy under a chunk of 8: {ok} of {n} utterances have every decision gap > {DELTA} nats; tokens identical")
    assert ok >= 0.5 * n, (ok, n)


def test_ctc_beam_under_a_chunk_vs_the_restatement():
    """masr_recog_ctc_beam under size 8 against ctc_beam_ref on the head logits of the chunked, bf16-emulating oracle: the peaked hybrid model,
    decision-gap filter, score tolerance and share of decode_util.py (JOINT_DELTA).  The batches were chosen on the CPU: the reference alone
    leaves 8 of 11 utterances above the gap at K = 4, and its best hypothesis differs from the full-context one in 8 of them."""
    sdj = joint_state_dict(TINY, 7)
    cfg = dict(TINY, ctc_weight=0.3, chunk=dict(size=8))
    eng = MasrEngine(cfg, C_SMALL)
    eng.load_state_dict(sdj)
    for K, nbest in ((4, 3), (1, 1)):
        ok = n = 0
        worst = 0.0
        for seed, ilens in ((12, [128, 100, 72, 60]), (13, [96, 80, 64]), (14, [160, 96, 64, 40])):
            xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
            got = eng.recog_ctc_beam(xs, il, K, nbest)
            assert eng.chunk_last() == 8
            with R.chunked_oracle(8), ref_cpu.bf16_emulation(), torch.no_grad():
                lp, lens = hybrid_ref.ctc_log_probs(hybrid_ref.leafify(sdj, TINY), TINY, xs, il)
            z = lp.transpose(0, 1).contiguous().numpy()[..., :C_SMALL]
            for b, r in enumerate(cr.ctc_beam_ref_batch(z, lens.tolist(), K, 0, C_SMALL - 1, nbest)):
                n += 1
                if not r["min_gap"] > JOINT_DELTA:
                    continue
                ok += 1
                hyp, s = got[b][0]
                pre, want = r["nbest"][0]
                worst = max(worst, abs(s - want))
                assert tuple(hyp) == pre and abs(s - want) <= 0.1 + 3e-3 * abs(want), (K, seed, b, hyp, pre, s, want)
        print(f"ctc_beam under a chunk of 8, K = {K}: {ok} of {n} utterances above the gap; best hypothesis identical, worst score diff {worst:.2e}")
        assert ok >= 0.5 * n, (K, ok, n)


def test_dynamic_policy_draws_per_step_and_replayed_graphs_follow(sd):
    xs, il, ys, ol = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    xd, Tp = xs.cuda(), max(GPU_ILENS) // 4
    pol = dict(size=8, left=2, dynamic=1)
    direct, graphs = engine(sd, pol, dropout=0.1), engine(sd, pol, dropout=0.1)
    graphs.set_step_graphs(True)
    drawn = []
    with torch.cuda.stream(torch.cuda.Stream()):                 # (steps on the legacy NULL stream are never captured)
        for k in range(16):
            state = direct.dropout_state()
            assert graphs.dropout_state() == state
            want = chunk_draw(*state, Tp)
            assert want == R.chunk_draw(*state, Tp)
            direct.run_batch(xd, il, ys, ol, train=True)
            graphs.run_batch(xd, il, ys, ol, train=True)
            assert direct.chunk_last() == want and graphs.chunk_last() == want, k
            assert direct.read_stats()["loss"] == graphs.read_stats()["loss"], (k, want)
            assert same_bits(direct.grads, graphs.grads), (k, want)
            drawn.append(want)
        torch.cuda.current_stream().synchronize()
    c = graphs.step_counters()
    assert c["captured"] == 1 and c["replayed"] >= 12 and direct.step_counters()["replayed"] == 0, c
    assert 0 in drawn and len(set(drawn)) >= 3, drawn            # full-context steps and several chunks, all through ONE captured graph
    # a pass that does not train runs under `size`, whatever the steps drew
    direct.run_batch(xd, il, ys, ol, train=False)
    assert direct.chunk_last() == 8
    fixed = engine(sd, dict(size=8, left=2), dropout=0.1)
    fixed.run_batch(xd, il, ys, ol, train=False)
    assert direct.read_stats()["loss"] == fixed.read_stats()["loss"]


def test_a_drawn_chunk_is_that_chunk_as_a_fixed_policy(sd):
    """the step a dynamic policy runs with chunk c has the bits of a fixed policy {c, left} at the same dropout position"""
    xs, il, ys, ol = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    xd, Tp = xs.cuda(), max(GPU_ILENS) // 4
    dyn = engine(sd, dict(size=0, left=1, dynamic=1), dropout=0.1)
    seen = set()
    for k in range(6):
        state = dyn.dropout_state()
        c = chunk_draw(*state, Tp)
        dyn.run_batch(xd, il, ys, ol, train=True)
        fixed = engine(sd, dict(size=c, left=1) if c else None, dropout=0.1)
        fixed.set_dropout_state(state)
        fixed.run_batch(xd, il, ys, ol, train=True)
        assert dyn.read_stats()["loss"] == fixed.read_stats()["loss"] and same_bits(dyn.grads, fixed.grads), (k, c)
        seen.add(c)
    assert len(seen) >= 2, seen


def test_policy_off_is_the_engine_without_one_bit_for_bit(sd):
    xs, il, ys, ol = synth_batch(GPU_SEED, GPU_ILENS, GPU_OLENS)
    xd = xs.cuda()
    e, plain = engine(sd, dict(size=4, left=1), dropout=0.1), engine(sd, None, dropout=0.1)
    assert plain.chunk is None
    e.run_batch(xd, il, ys, ol, train=True)
    plain.run_batch(xd, il, ys, ol, train=True)
    assert e.chunk_last() == 4 and plain.chunk_last() == 0
    assert e.read_stats()["loss"] != plain.read_stats()["loss"] and not same_bits(e.grads, plain.grads)
    e.set_chunk(None)
    assert e.chunk is None
    for train in (True, False):
        e.set_dropout_state(plain.dropout_state())
        e.run_batch(xd, il, ys, ol, train=train)
        plain.run_batch(xd, il, ys, ol, train=train)
        assert e.chunk_last() == 0
        assert e.read_stats()["loss"] == plain.read_stats()["loss"] and same_bits(e.grads, plain.grads)
        assert same_bits(e.last_logits()[0], plain.last_logits()[0])
    assert same_bits(e.recog(xd, il).float(), plain.recog(xd, il).float())
    # bad bounds: refused, the old policy stays
    e.set_chunk(dict(size=4))
    for bad in (dict(size=-1), dict(size=4, left=-2), dict(size=4, dynamic=2)):
        with pytest.raises(ValueError):
            e.set_chunk(bad)
    from masr_amd._cabi import MasrChunkPolicy, lib
    import ctypes as C
    assert lib().masr_set_chunk(e.h, C.byref(MasrChunkPolicy(4, -2, 0))) == -1 and b"left >= -1" in lib().masr_last_error()
    e.run_batch(xd, il, ys, ol, train=False)
    assert e.chunk == dict(size=4, left=-1, dynamic=0) and e.chunk_last() == 4
    fresh = MasrEngine(TINY, ODIM)
    with pytest.raises(MasrError, match="no encoder forward"):
        fresh.chunk_last()


@pytest.mark.parametrize("mode", ["greedy", "ctc_beam", "rescore"])
def test_tester_decodes_under_the_chunk_of_its_flags(tmp_path, monkeypatch, mode):
    beam = None if mode == "greedy" else {"beam_size": 4}
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, mode, beam, hybrid=True)
    t.load_data(); t.set_model(); t.exec()
    assert t.chunk_last == 0
    plain = (log_dir / f"{mode}_decode" / "best-hyp").read_text()
    t, log_dir, _, _ = make_tester(tmp_path, monkeypatch, mode, beam, hybrid=True)
    t.paras.decode_chunk, t.paras.decode_left = 8, 1
    from masr_amd.tester import Tester
    t = Tester(t.config, t.paras, {"af": "african", "au": "australia", "ca": "canada"})
    t.load_data(); t.set_model(); t.exec()
    assert t.chunk_last == 8 and t.asr_model.engine.chunk == dict(size=8, left=1, dynamic=0)
    assert len((log_dir / f"{mode}_decode" / "best-hyp").read_text().splitlines()) == len(plain.splitlines()) == 6


def test_blstm_trainer_refuses_the_key():
    from masr_amd.blstm_trainer import get_trainer
    with pytest.raises(ValueError, match="transformer only"):
        get_trainer(object, {"asr_model": {"chunk": dict(size=8)}}, None, None)
