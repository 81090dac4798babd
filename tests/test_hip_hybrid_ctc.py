"""Joint CTC/attention training of the transformer (asr_model.ctc_weight; include/masr.h masr_create_ctc) on the GPU, against the CPU
restatement tests/hybrid_ref.py with the bounds of tests/test_hip_engine.py::test_run_batch_vs_oracle_and_golden."""
import math
import random

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import hybrid_ref  # noqa: E402
from masr_amd import _cabi  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.make_goldens import TINY, ODIM, synth_batch  # noqa: E402

CASES = {"ragged": ([64, 52, 40, 33], [9, 7, 5, 3]), "same": ([48, 48, 48], [6, 6, 4]), "single": ([37], [5])}
HEAD = hybrid_ref.HEAD


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-20))


def hyb(w, **kw):
    return dict(TINY, ctc_weight=w, **kw)


@pytest.fixture(scope="module")
def sd():
    return hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7), ODIM, seed=3)


def _plain(sd):
    return {k: v for k, v in sd.items() if k not in HEAD}


def _cmp(a, b, n):
    a = a.cpu()
    if n.endswith("in_proj_bias"):
        E = TINY["d_model"]                                  # key-bias third has zero true gradient
        a = torch.cat([a[:E], a[2 * E:]]); b = torch.cat([b[:E], b[2 * E:]])
    return rel_l2(a, b)


def test_layout(sd):
    plain = MasrEngine(TINY, ODIM)
    eng = MasrEngine(hyb(0.3), ODIM)
    assert eng.ctc_weight == pytest.approx(0.3) and plain.ctc_weight == 0.0
    E = TINY["d_model"]
    assert list(eng.table)[:-2] == list(plain.table) and list(eng.table)[-2:] == list(HEAD)
    assert [eng.table[k] for k in plain.table] == [plain.table[k] for k in plain.table]          # every existing offset stays put
    assert eng.table[HEAD[0]][1] == (ODIM, E) and eng.table[HEAD[1]][1] == (ODIM,)
    assert eng.numel == plain.numel + ODIM * (E + 1)
    eng.load_state_dict(sd)
    out = eng.state_dict()
    assert list(out.keys()) == list(sd.keys())
    for k in sd:
        torch.testing.assert_close(out[k].cpu(), sd[k], rtol=0, atol=1e-6 if k == "pos_encoder.pe" else 0)


@pytest.mark.parametrize("cname", list(CASES))
@pytest.mark.parametrize("w", [0.3, 0.7])
def test_run_batch_vs_restatement(sd, cname, w):
    ilens, olens = CASES[cname]
    xs, il, ys, ol = synth_batch(11, ilens, olens)
    eng = MasrEngine(hyb(w), ODIM, label_smoothing=0.2)
    eng.load_state_dict(sd)
    eng.run_batch(xs, il, ys, ol, train=True)
    st = eng.read_stats()
    p = hybrid_ref.leafify(sd, TINY)
    info, grads = hybrid_ref.run_batch_train(p, TINY, (xs, il, ys, ol), 0.2, w)
    with ref_cpu.bf16_emulation():
        pq = hybrid_ref.leafify(sd, TINY)
        infoq, gradsq = hybrid_ref.run_batch_train(pq, TINY, (xs, il, ys, ol), 0.2, w)
    r32 = abs(st["loss"] - info["loss"]) / info["loss"]
    r16 = abs(st["loss"] - infoq["loss"]) / infoq["loss"]
    assert st["n_total"] == sum(olens) + len(olens)
    g_all = eng.state_dict(flat=eng.grads)
    names = list(gradsq)
    worst32 = max(_cmp(g_all[n], grads[n], n) for n in names)
    worst, worst_n = 0.0, None
    for n in names:
        r = _cmp(g_all[n], gradsq[n], n)
        if r > worst:
            worst, worst_n = r, n
    head = max(_cmp(g_all[n], gradsq[n], n) for n in HEAD)
    flat_a = torch.cat([g_all[n].cpu().reshape(-1) for n in names if not n.endswith("in_proj_bias")]).double()
    flat_b = torch.cat([gradsq[n].reshape(-1) for n in names if not n.endswith("in_proj_bias")]).double()
    cos = float((flat_a * flat_b).sum() / (flat_a.norm() * flat_b.norm()))
    print(f"{cname} w={w}: loss {st['loss']:.6f} (att {infoq['att']:.4f} ctc {infoq['ctc']:.4f}) rel fp32 {r32:.2e} rel bf16 {r16:.2e}; "
          f"worst grad rel-l2 {worst:.4f} ({worst_n}), head {head:.4f}, fp32 oracle {worst32:.4f}; cos {cos:.6f}")
    assert r32 <= 1e-3, (st["loss"], info["loss"])
    assert r16 <= 2e-4, (st["loss"], infoq["loss"])
    assert worst < 8e-2, (worst_n, worst)
    assert worst32 < 0.15, worst32
    assert cos > 0.999, cos


def test_two_inner_steps_vs_restatement(sd):
    """two inner steps (run_batch -> clip 5 -> SGD momentum .9 nesterov), lr x1000 as test_hip_engine's inner-step test, against the
    bf16-emulating restatement.  The first step is held to the single-batch bounds; at lr 0.79 that step turns the few-percent per-tensor
    gradient disagreement of two bf16 implementations into different weights, so the second is held to 2e-3 (a wrong weight, a missing head
    update or an unscaled branch shows up as >> 1e-2)"""
    w = 0.3
    ilens, olens = CASES["ragged"]
    eng = MasrEngine(hyb(w), ODIM, label_smoothing=0.2)
    eng.load_state_dict(sd)
    lr = ref_cpu.inner_lr(TINY) * 1000
    mom = torch.zeros_like(eng.params)
    p, bufs = hybrid_ref.leafify(sd, TINY), {}
    for i, seed in enumerate((11, 12)):
        batch = synth_batch(seed, ilens, olens)
        eng.run_batch(*batch, train=True)
        eng.clip_sgd_step(mom, 5.0, lr, 0.9, True, first_step=(i == 0))
        st = eng.read_stats()
        with ref_cpu.bf16_emulation():
            info = hybrid_ref.inner_step(p, TINY, batch, 0.2, w, bufs, lr)
        rl, rn = abs(st["loss"] - info["loss"]) / info["loss"], abs(st["grad_norm"] - info["grad_norm"]) / info["grad_norm"]
        print(f"step {i}: loss {st['loss']:.6f} vs {info['loss']:.6f} (rel {rl:.2e}), grad norm {st['grad_norm']:.4f} vs {info['grad_norm']:.4f}")
        assert rl <= (2e-4 if i == 0 else 2e-3)
        assert rn <= (2e-2 if i == 0 else 5e-2)
    for n in ("char_trans.weight", HEAD[0], HEAD[1], "encoder.norm.weight"):
        start = sd[n]
        r = rel_l2(eng.view(n).cpu() - start, p[n].detach() - start)
        print(f"update of {n}: rel-l2 {r:.4f}")
        assert r < 0.1, (n, r)


def test_weight_zero_is_the_plain_engine_bit_for_bit(sd):
    cfg = dict(TINY, dropout=0.1, pos_dropout=0.1)
    engs = [MasrEngine(cfg, ODIM, label_smoothing=0.2), MasrEngine(dict(cfg, ctc_weight=0.0), ODIM, label_smoothing=0.2)]
    assert engs[0].numel == engs[1].numel and list(engs[0].table) == list(engs[1].table)
    for e in engs:
        e.load_state_dict(_plain(sd)); e.set_seed(5)
    moms = [torch.zeros_like(e.params) for e in engs]
    for step, seed in enumerate((11, 12, 13)):
        out = []
        for e, mom in zip(engs, moms):
            e.run_batch(*synth_batch(seed, *CASES["ragged"]), train=True)
            g = e.grads.clone()
            e.clip_sgd_step(mom, 5.0, 0.01, 0.9, True, step == 0)
            out.append((e.read_stats(), g, e.params.clone()))
        (s0, g0, p0), (s1, g1, p1) = out
        assert s0 == s1 and torch.equal(g0, g1) and torch.equal(p0, p1), step


def test_infeasible_utterance_contributes_zero(sd):
    """the last utterance has 9 labels and 5 encoder frames: its CTC nll is infinite, zero_infinity drops it"""
    w = 0.5
    xs, il, ys, ol = synth_batch(11, [64, 52, 40, 20], [9, 7, 5, 9])
    eng = MasrEngine(hyb(w), ODIM, label_smoothing=0.2)
    eng.load_state_dict(sd)
    eng.run_batch(xs, il, ys, ol, train=True)
    st = eng.read_stats()
    assert math.isfinite(st["loss"]) and bool(torch.isfinite(eng.grads).all())
    with ref_cpu.bf16_emulation():
        info, grads = hybrid_ref.run_batch_train(hybrid_ref.leafify(sd, TINY), TINY, (xs, il, ys, ol), 0.2, w)
    # the same batch without that utterance's CTC term: its mean over the three others, divided by four
    with torch.no_grad(), ref_cpu.bf16_emulation():
        p = hybrid_ref.leafify(sd, TINY)
        three, _ = hybrid_ref.ctc_term(p, TINY, xs[:3], il[:3], ys[:3], ol[:3])
    assert abs(info["ctc"] - float(three) * 3 / 4) <= 1e-5 * info["ctc"]
    print(f"infeasible: loss {st['loss']:.6f} restatement {info['loss']:.6f}")
    assert abs(st["loss"] - info["loss"]) <= 2e-4 * info["loss"]
    g_all = eng.state_dict(flat=eng.grads)
    for n in HEAD:
        assert _cmp(g_all[n], grads[n], n) < 8e-2, n


def test_eval_mode_no_backward(sd):
    eng = MasrEngine(hyb(0.3), ODIM, label_smoothing=0.2)
    eng.load_state_dict(sd)
    eng.grads.fill_(3.0)
    xs, il, ys, ol = synth_batch(11, *CASES["same"])
    eng.run_batch(xs, il, ys, ol, train=False)
    st = eng.read_stats()
    with torch.no_grad(), ref_cpu.bf16_emulation():
        p = hybrid_ref.leafify(sd, TINY)
        logit, gold = ref_cpu.model_forward(p, TINY, xs, il, ys, ol.clone())
        att = float(ref_cpu.label_smoothed_ce(logit, gold, 0.2)[0])
        ctc = float(hybrid_ref.ctc_term(p, TINY, xs, il, ys, ol)[0])
    want = 0.7 * att + 0.3 * ctc
    assert abs(st["loss"] - want) <= 2e-4 * want and torch.all(eng.grads == 3.0)


@pytest.mark.parametrize("ksplit", [False, True])
def test_graph_replayed_steps_equal_direct_launches(sd, ksplit):
    cfg = hyb(0.3, dropout=0.1, pos_dropout=0.1)
    xs, il, ys, ol = synth_batch(11, *CASES["ragged"])
    ys2 = [(y + 1) % 365 + 1 for y in ys]
    xs_dev = xs.cuda()
    engs = []
    for direct in (False, True):
        e = MasrEngine(cfg, ODIM, label_smoothing=0.2)
        e.load_state_dict(sd); e.set_seed(99); e.set_ksplit(ksplit)
        if direct:
            e.profile(True)
        e.set_step_graphs(True)
        engs.append(e)
    moms = [torch.zeros_like(e.params) for e in engs]
    with torch.cuda.stream(torch.cuda.Stream()):
        for step in range(5):
            labels = ys if step % 3 else ys2
            out = []
            for e, mom in zip(engs, moms):
                e.run_batch(xs_dev, il, labels, ol, train=True)
                g = e.grads.clone()
                e.clip_sgd_step(mom, 5.0, 0.01, 0.9, True, step == 0)
                out.append((e.read_stats(), g, e.params.clone()))
            (s0, g0, p0), (s1, g1, p1) = out
            assert s0 == s1, (step, s0, s1)
            assert torch.equal(g0, g1) and torch.equal(p0, p1), f"step {step}: replayed and direct launches differ"
        for _ in range(3):
            r = [None, None]
            for i, e in enumerate(engs):
                e.run_batch(xs_dev, il, ys, ol, train=False)
                r[i] = e.read_stats()["loss"]
            assert r[0] == r[1]
        torch.cuda.current_stream().synchronize()
    c0 = engs[0].step_counters()
    assert c0["replayed"] > 0 and engs[1].step_counters()["replayed"] == 0, c0


def test_fomaml_task_slots_reproduce_sequential_run(tmp_path, monkeypatch):
    """--tasks_per_gpu 1 and 4 give bit-identical meta weights with the joint objective (test_hip_fomaml's invariant)"""
    from test_hip_fomaml import make_run
    from masr_amd.fo_meta_interface import FOMetaASRInterface
    from masr_amd.transformer_torch_trainer import get_trainer
    monkeypatch.chdir(tmp_path)
    finals = []
    for k in (1, 4):
        cfg, paras, id2accent = make_run(tmp_path, tasks_per_gpu=k, max_step=2)
        cfg["asr_model"]["ctc_weight"] = 0.3
        random.seed(531); np.random.seed(531); torch.manual_seed(531)
        solver = get_trainer(FOMetaASRInterface, cfg, paras, id2accent)
        solver.load_data(); solver.set_model()
        solver.asr_model.load_state_dict(hybrid_ref.with_head(ref_cpu.deterministic_state_dict(cfg["asr_model"], ODIM, seed=7), ODIM, 3))
        solver.load_model()
        solver.evaluate = lambda: None
        solver.exec()
        torch.cuda.synchronize()
        finals.append((solver._original.clone(), dict(solver.train_info)))
    assert finals[0][0].numel() == solver.asr_model.engine.numel
    assert torch.equal(finals[0][0], finals[1][0])
    assert finals[0][1] == finals[1][1]


def test_pretrain_from_plain_checkpoint_then_resume(golden_dir, tmp_path, monkeypatch, capsys):
    """train.py --pretrain of a hybrid model from a PLAIN model's snapshot (the head is initialised and the log says so), then --resume
    of a hybrid run continues it bit for bit (test_hip_chain / test_hip_resume fixtures)"""
    import train
    from oracle.make_goldens import chain_workspace
    monkeypatch.chdir(tmp_path)
    _, ft = chain_workspace(tmp_path, golden_dir)
    ft["solver"].update(eval_ival=20, log_ival=5)

    def cli(suffix, epochs, w, *extra):
        ft["solver"]["total_epochs"] = epochs
        ft["asr_model"].pop("ctc_weight", None)
        if w:
            ft["asr_model"]["ctc_weight"] = w
        yaml.safe_dump(ft, open(tmp_path / "ft.yaml", "w"))
        train.main(["--config", "ft.yaml", "--accent", "ca", "--algo", "no", "--eval_suffix", suffix, "--njobs", "1", *extra])
        torch.cuda.synchronize()
        return tmp_path / "testing-logs" / "evaluation" / "chain-ft" / "no" / suffix / suffix / "canada" / "0"
    plain = cli("plain", 1, 0.0, "--overwrite")
    assert HEAD[0] not in torch.load(plain / "snapshot.latest")
    capsys.readouterr()
    pre = cli("pre", 1, 0.3, "--overwrite", "--pretrain", "--pretrain_suffix", "pre", "--pretrain_model_path", str(plain / "snapshot.latest"))
    err = capsys.readouterr().err
    assert "no CTC head" in err and "ctc.ctc_lo.weight" in err, err[-2000:]
    sd = torch.load(pre / "snapshot.latest")
    assert HEAD[0] in sd and HEAD[1] in sd
    # resume of a hybrid run: 2 epochs straight == 1 epoch, stop, resume to 2
    full = cli("full", 2, 0.3, "--overwrite")
    cli("part", 1, 0.3, "--overwrite")
    part = cli("part", 2, 0.3, "--resume")
    a, b = torch.load(full / "snapshot.latest"), torch.load(part / "snapshot.latest")
    assert a.keys() == b.keys() and HEAD[0] in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a[HEAD[0]], sd[HEAD[0]])


def test_errors(sd):
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            MasrEngine(hyb(bad), ODIM)
    assert not _cabi.lib().masr_create_ctc(None, 1.0)
    plain = MasrEngine(TINY, ODIM)
    with pytest.raises(RuntimeError, match=r"ctc\.ctc_lo\.weight.*ctc\.ctc_lo\.bias"):
        plain.load_state_dict(sd)
