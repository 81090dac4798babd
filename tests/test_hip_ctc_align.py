"""CTC forced alignment through the models: MasrEngine.ctc_align / MyTransformer.ctc_align (masr_recog_ctc_align),
BlstmEngine.ctc_align / MonoBLSTM.ctc_align and the Tester's `ctc_align` mode.

Both models are checked on the fp32 logits the alignment itself read -- the BLSTM's last_logits(), the hybrid transformer's head logits in
the workspace (include/masr_test.h masr_test_ctc_align_logits) -- so no encoder noise enters: the path is a function of fp32 additions and
comparisons on those logits, and frames / start / end must equal the restatement of tests/ctc_align_ref.py bit for bit, whatever the logits
are.  The score is compared with masr_ctc_align's own on the same logits (bit for bit) and with the restatement's within the log-sum's
error and the roundings of fp32 sums of magnitude <= M on logits off any grid (ctc_align_ref.score_bound, on_grid=False)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import ctc_align_ref as ar  # noqa: E402
from masr_amd._cabi import MasrError, align_targets, lib  # noqa: E402
from masr_amd.blstm_engine import BlstmEngine  # noqa: E402
from masr_amd.engine import MasrEngine  # noqa: E402
from oracle import blstm_cpu  # noqa: E402
from oracle.make_goldens import BLSTM_TINY, ODIM, TINY, synth_batch  # noqa: E402
from decode_util import C_SMALL, joint_engine, joint_state_dict, make_tester  # noqa: E402

DEV = "cuda:0"


def p(t):
    return C.c_void_p(t.data_ptr())


def operator(logits, lens, ys, Cn, blank=0):
    """masr_ctc_align on device logits [B, Tp, ld] and enc_lens -> (frames, start, end, score) device tensors"""
    l = lib()
    B, Tp, ld = logits.shape
    tgt, off, tl, maxL = align_targets(ys, [len(y) for y in ys], logits.device)
    nb = int(l.masr_ctc_align_work_bytes(B, Tp, maxL))
    work = torch.empty(nb, dtype=torch.uint8, device=logits.device)
    i32 = dict(dtype=torch.int32, device=logits.device)
    out = (torch.empty(B, Tp, **i32), torch.empty(B, maxL, **i32), torch.empty(B, maxL, **i32), torch.empty(B, device=logits.device))
    rc = l.masr_ctc_align(p(logits), ld, p(lens), p(tgt), p(off), p(tl), B, Tp, Cn, blank, maxL, p(work), nb, *map(p, out),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, l.masr_last_error()
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def check_restatement(name, logits, lens, ys, Cn, out, blank=0):
    """device results against align_f32 on the same logits -> how many utterances were feasible"""
    fr, st, en, sc = (t.cpu().numpy() for t in out)
    z = logits[..., :Cn].cpu().numpy()
    Tp, maxL, feasible = fr.shape[1], st.shape[1], 0
    for b, y in enumerate(ys):
        n = int(lens[b])
        r = ar.align_f32(z[b], n, y, blank, Tp, maxL)
        assert np.array_equal(fr[b], r["frames"]) and np.array_equal(st[b], r["start"]) and np.array_equal(en[b], r["end"]), (name, b)
        if r["states"] is None:
            assert np.isneginf(sc[b]), (name, b)
            continue
        feasible += 1
        lp, M = ar.path_logprob_f64(z[b], n, y, blank, fr[b])
        bound = ar.score_bound(z[b], n, M, on_grid=False)
        print(f"{name} b={b}: score {float(sc[b]):.6f} fp64 {lp:.6f} bound {bound:.3g} segments {list(zip(st[b][:len(y)], en[b][:len(y)]))}")
        assert abs(float(sc[b]) - lp) <= bound, (name, b, float(sc[b]), lp, bound)
    return feasible


def targets(seed, lens, hi):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(1, hi, n)] for n in lens]


def test_hybrid_engine_ctc_align():
    eng = joint_engine(TINY, joint_state_dict(TINY, 7))
    ilens = [64, 52, 40, 33]                                     # enc_lens 16, 13, 10, 8
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    ys = targets(3, [5, 4, 12, 0], C_SMALL - 1)                 # the third transcript is longer than its 10 frames: infeasible
    ys[0][1] = ys[0][0]                                          # an adjacent repeat
    ol = [len(y) for y in ys]
    B, T = 4, 64
    got = [t.clone() for t in eng.ctc_align(xs, il, ys, ol, raw=True)]
    logits, lens = eng.last_ctc_align_logits(B, T, max(ol))
    assert lens.cpu().tolist() == [n // 4 for n in ilens] and logits.shape[1] == T // 4 and logits.shape[2] >= C_SMALL
    logits, lens = logits.clone(), lens.clone()
    assert same_bits(got, operator(logits, lens, ys, C_SMALL))
    assert check_restatement("hybrid", logits, lens.cpu().tolist(), ys, C_SMALL, got) == 3
    fr, st, en, sc = (t.cpu() for t in got)
    assert np.isneginf(float(sc[2])) and (fr[2] == -2).all() and (st[2] == -1).all() and (fr[3, :8] == -1).all() and (fr[3, 8:] == -2).all()
    # the lists
    lists = eng.ctc_align(xs, il, ys, ol)
    assert [len(s) for _, s, _ in lists] == [5, 4, 0, 0] and [len(f) for _, _, f in lists] == [16, 13, 0, 8]
    assert [tok for tok, _, _ in lists[0][1]] == ys[0] and all(e > s for _, s, e in lists[0][1]) and lists[2][0] == float("-inf")
    assert [float(sc[b]) for b in range(4)] == [s for s, _, _ in lists]
    # another decode mode uses the workspace in between: the same bits afterwards
    eng.recog_ctc_beam(xs, il, 4)
    eng.recog_beam(xs, il, 2)
    assert same_bits(got, eng.ctc_align(xs, il, ys, ol, raw=True))
    # tensors as run_batch takes them
    assert same_bits(got, eng.ctc_align(xs, il, [torch.tensor(y, dtype=torch.int64) for y in ys], torch.tensor(ol), raw=True))
    # a plain model has no CTC head
    plain = MasrEngine(TINY, C_SMALL)
    l = lib()
    assert l.masr_ctc_align_workspace_bytes(plain.h, 4, 64, 5) < 0 and b"no CTC head" in l.masr_last_error()
    with pytest.raises(MasrError, match="no CTC head"):
        plain.ctc_align(xs, il, ys, ol)
    assert l.masr_ctc_align_workspace_bytes(eng.h, 4, 64, 1024) < 0 and l.masr_ctc_align_workspace_bytes(eng.h, 4, 3, 5) < 0
    with pytest.raises(MasrError, match=r"ilens must be in \[4, T\]"):
        eng.ctc_align(xs, [64, 52, 40, 3], ys, ol)


def test_hybrid_engine_passes_refusals_on():
    eng = joint_engine(TINY, joint_state_dict(TINY, 7))
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    ys = [[1, 2, 3], [4, 0, 5], [2, C_SMALL, 2]]                 # a blank and a class past the last one
    lists = eng.ctc_align(xs, il, ys, [3, 3, 3])
    assert np.isfinite(lists[0][0]) and len(lists[0][1]) == 3
    assert all(np.isnan(s) and segs == [] and fr == [] for s, segs, fr in lists[1:])


def _blstm_sd(scale=30.0):
    sd = blstm_cpu.deterministic_state_dict(BLSTM_TINY, ODIM, seed=11)
    sd["head.weight"] = sd["head.weight"] * scale
    return sd


def test_blstm_engine_ctc_align():
    eng = BlstmEngine(BLSTM_TINY, ODIM)
    eng.load_state_dict(_blstm_sd())
    feasible = 0
    for seed, ilens, ol in ((22, [57, 57, 44, 12], [6, 0, 11, 4]), (24, [36, 28, 20, 13], [3, 7, 2, 1])):
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        ys = targets(seed, ol, ODIM - 1)
        got = eng.ctc_align(xs, il, ys, ol, raw=True)
        logits, lens = eng.last_logits()
        assert same_bits(got, operator(logits, lens, ys, ODIM))
        feasible += check_restatement(f"blstm {seed}", logits, lens.cpu().tolist(), ys, ODIM, got)
    assert feasible >= 6


def _all_blank(name, lists, enc_lens):
    """every utterance of an all-empty batch: the all-blank path over its frames, no segments, a finite log-probability"""
    assert len(lists) == len(enc_lens)
    for b, ((score, segs, frames), n) in enumerate(zip(lists, enc_lens)):
        assert segs == [] and frames == [-1] * n and np.isfinite(score) and score < 0, (name, b, score, segs, frames)


def test_all_empty_transcripts_through_the_facades():
    """maxL = 0: start and end have no element, and the calls must still hand the operator pointers it accepts"""
    from masr_amd.blstm_engine import MonoBLSTM
    from masr_amd.marcos import BLANK_SYMBOL
    ilens = [64, 52, 40, 33]
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    eng = joint_engine(TINY, joint_state_dict(TINY, 7))
    for ys in ([[]] * 4, [torch.zeros(0, dtype=torch.int64)] * 4):
        _all_blank("hybrid", eng.ctc_align(xs, il, ys, [0] * 4), [n // 4 for n in ilens])
    fr, st, en, sc = eng.ctc_align(xs, il, [[]] * 4, [0] * 4, raw=True)
    assert st.shape == (4, 0) and en.shape == (4, 0) and torch.isfinite(sc).all()
    logits, lens = eng.last_ctc_align_logits(4, 64, 0)
    z = logits[..., :C_SMALL].cpu().numpy()
    for b in range(4):
        r = ar.align_f32(z[b], int(lens[b]), [], 0, 16, 0)
        lp, M = ar.path_logprob_f64(z[b], int(lens[b]), [], 0, r["frames"])
        assert np.array_equal(fr[b].cpu().numpy(), r["frames"]) and abs(float(sc[b]) - lp) <= ar.score_bound(z[b], int(lens[b]), M, on_grid=False)
    # one empty transcript alone: what the Tester sends at decode_batch_size 1
    _all_blank("hybrid alone", eng.ctc_align(xs[1:2, :52], [52], [[]], [0]), [13])
    blstm = BlstmEngine(BLSTM_TINY, ODIM)
    blstm.load_state_dict(_blstm_sd())
    lists = blstm.ctc_align(xs, il, [[]] * 4, [0] * 4)
    _all_blank("blstm", lists, blstm.last_logits()[1].cpu().tolist())
    mono = MonoBLSTM([BLANK_SYMBOL] + [f"u{i}" for i in range(1, ODIM - 1)] + ["</s>"], BLSTM_TINY, init=False)
    mono.load_state_dict(_blstm_sd())
    lists = mono.ctc_align(xs, il, [torch.zeros(0, dtype=torch.int64)] * 4, torch.zeros(4, dtype=torch.int64))
    _all_blank("mono", lists, [((n + 1) // 2 + 1) // 2 for n in ilens])      # each alone at its own length: two 2 x 2 pools, ceil mode


def test_transcripts_are_cut_to_olens_by_both_engines():
    """rows of a padded target tensor with their lengths give what the cut lists give; a length beyond its row is refused in Python"""
    ilens, ol = [64, 52, 40, 33], [5, 2, 3, 0]
    xs, il, _, _ = synth_batch(11, ilens, [3] * 4)
    ys = targets(5, ol, C_SMALL - 1)
    pad = torch.full((4, 6), C_SMALL - 2, dtype=torch.int64)
    for b, y in enumerate(ys):
        pad[b, :len(y)] = torch.tensor(y, dtype=torch.int64)
    eng = joint_engine(TINY, joint_state_dict(TINY, 7))
    assert eng.ctc_align(xs, il, list(pad), ol) == eng.ctc_align(xs, il, ys, ol)
    blstm = BlstmEngine(BLSTM_TINY, ODIM)
    blstm.load_state_dict(_blstm_sd())
    assert blstm.ctc_align(xs, il, list(pad), ol) == blstm.ctc_align(xs, il, ys, ol)
    for e in (eng, blstm):
        with pytest.raises(ValueError, match=r"olens\[1\] = 3 but ys\[1\] holds 2 tokens"):
            e.ctc_align(xs, il, ys, [5, 3, 3, 0])
        with pytest.raises(ValueError, match="one transcript per utterance"):
            e.ctc_align(xs, il, ys[:3], ol)


def _run(t):
    t.load_data(); t.set_model(); t.exec()


def _lines(t, align):
    """the ctc-ali lines `align(xs, ilens, ys, olens)` gives on the Tester's own batches"""
    want = []
    for idxs in t.eval_set.iter_indices():
        xs, il, ys, ol = t.eval_set.materialize(idxs)
        ys = [y[:int(n)] for y, n in zip(ys, ol)]
        for y, (score, segs, _) in zip(ys, align(xs, il, ys, ol)):
            want.append("{}\t{}\t{}".format(" ".join(str(v) for v in y.tolist()), " ".join(f"{s}:{e}" for _, s, e in segs), repr(score)))
    return want


def _check_file(t, log_dir, lines):
    assert len(lines) == 6 and not (log_dir / "ctc_align_decode" / "best-hyp").exists()
    some = 0
    for l in lines:
        ref, segs, score = l.split("\t")
        if segs:
            some += 1
            se = [tuple(int(v) for v in s.split(":")) for s in segs.split()]
            assert len(se) == len(ref.split()) and all(e > s for s, e in se) and all(a[1] <= b[0] for a, b in zip(se, se[1:]))
            assert np.isfinite(float(score)) and float(score) < 0
        else:
            assert score == "-inf"
    assert some >= 2


def _resume(make, ali, lines):
    full = ali.read_text()
    for keep in (5, 1):
        ali.write_text("".join(l + "\n" for l in lines[:keep]))
        t2 = make(resume=True)
        assert t2.prev_decode_step == keep
        _run(t2)
        assert ali.read_text() == full, f"resume after {keep} lines"


def test_tester_transformer_ctc_align(tmp_path, monkeypatch):
    def make(resume=False, hybrid=True, bs=4):
        return make_tester(tmp_path, monkeypatch, "ctc_align", None, hybrid=hybrid, bs=bs, resume=resume)
    t, log_dir, sd, cfg = make()
    assert "beam_decode" not in cfg["solver"]
    _run(t)
    ali = log_dir / "ctc_align_decode" / "ctc-ali"
    lines = ali.read_text().splitlines()
    _check_file(t, log_dir, lines)
    eng = MasrEngine(cfg["asr_model"], ODIM)
    eng.load_state_dict(sd)
    assert lines == _lines(t, eng.ctc_align)
    _resume(lambda **kw: make(**kw)[0], ali, lines)
    assert not (log_dir / "ctc_align_decode" / "best-hyp").exists()
    t = make(hybrid=False)[0]
    t.load_data(); t.set_model()
    with pytest.raises(ValueError, match="asr_model.ctc_weight"):
        t.exec()


def test_tester_blstm_ctc_align_lines_do_not_depend_on_the_batch(tmp_path, monkeypatch):
    def make(resume=False, bs=4):
        return make_tester(tmp_path, monkeypatch, "ctc_align", None, blstm_sd=_blstm_sd(), bs=bs, resume=resume)[:2]
    t, log_dir = make()
    _run(t)
    ali = log_dir / "ctc_align_decode" / "ctc-ali"
    lines4 = ali.read_text().splitlines()
    _check_file(t, log_dir, lines4)
    assert lines4 == _lines(t, t.asr_model.ctc_align)
    _resume(lambda **kw: make(**kw)[0], ali, lines4)
    # MonoBLSTM.ctc_align runs every utterance alone at its own length: batch size 1 writes the same lines (in the loader's other order)
    t1, _ = make(bs=1)
    _run(t1)
    assert sorted(ali.read_text().splitlines()) == sorted(lines4)
    # and a padded batch gives each utterance what it gets alone
    xs, il, _, _ = synth_batch(21, [61, 50, 38, 30], [3] * 4)
    ys = targets(21, [4, 3, 5, 2], ODIM - 1)
    got = t1.asr_model.ctc_align(xs, il, ys, [4, 3, 5, 2])
    for b in range(4):
        n = int(il[b])
        assert got[b] == t1.asr_model.engine.ctc_align(xs[b:b + 1, :n], [n], [ys[b]], [len(ys[b])], blank=t1.asr_model.blank_id)[0]
