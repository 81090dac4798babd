"""The CPU side of LSTM LM shallow fusion: the restatement of tests/nlm_ref.py is torch.nn.Embedding / LSTM / Linear /
log_softmax when its bf16 emulation is off, its rows normalise, the restated search is the plain beam at lm_w = 0, the arg-max chain at K = 1
and an exhaustive search when nothing that matters is pruned, each mutated restatement changes results (so the comparison with the engine can
see such a bug), and the checkpoint reader (masr_amd.nlm.parse_state_dict) accepts both key layouts and names what is missing.  CPU only."""
import numpy as np
import pytest
import torch

import beam_ref
import nlm_ref
import masr_amd  # noqa: F401
from masr_amd.nlm import parse_state_dict
from oracle import ref_cpu
from oracle.make_goldens import TINY, synth_batch
from decode_util import C_SMALL, peaked_state_dict

NLM_SEED = 7                                                    # tests/test_hip_nlm_beam.py has the criteria
BATCHES = ((11, [64, 52, 40, 33]), (12, [48, 48, 44]), (13, [37, 60]))      # the nine utterances of test_hip_lm_beam.py


@pytest.mark.parametrize("L", [1, 2])
def test_restatement_without_emulation_is_torch(L):
    C, E, H = 11, 20, 24
    m = nlm_ref.toy_nlm(C, E, H, L, seed=7 + L, start_id=0)
    emb, rnn, lo = nlm_ref.torch_modules(m)
    rng = np.random.RandomState(L)
    for n in (0, 1, 5, 13):
        h = [int(t) for t in rng.randint(0, C, size=n)]
        with torch.no_grad():
            y, _ = rnn(emb(torch.tensor([m["start_id"]] + h)).unsqueeze(1))
            want = torch.log_softmax(lo(y[:, 0]), dim=-1).numpy()
        for i in range(n + 1):
            got = nlm_ref.lm_row(m, h[:i], emulate=False)
            assert np.abs(got - want[i]).max() <= 1e-5, (L, n, i, np.abs(got - want[i]).max())
        assert abs(nlm_ref.score(m, h, emulate=False) - float(sum(want[i][t] for i, t in enumerate(h + [C - 1])))) <= 1e-4


@pytest.mark.parametrize("emulate", [False, True])
def test_rows_normalise(emulate):
    m = nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED)
    rng = np.random.RandomState(3)
    for n in (0, 2, 9):
        row = nlm_ref.lm_row(m, [int(t) for t in rng.randint(1, C_SMALL - 1, size=n)], emulate)
        assert row.dtype == np.float32 and (row <= 0).all()
        assert abs(float(np.exp(row.astype(np.float64)).sum()) - 1.0) <= 1e-5


def test_start_token_matters():
    a, b = nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED, start_id=0), nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED, start_id=C_SMALL - 1)
    assert np.abs(nlm_ref.lm_row(a, [3, 4]) - nlm_ref.lm_row(b, [3, 4])).max() > 1e-3


@pytest.fixture(scope="module")
def peaked():
    sd = peaked_state_dict(TINY, 7)
    sd["char_trans.bias"] = sd["char_trans.bias"].clone()
    sd["char_trans.bias"][0] = -30.0
    return ref_cpu.leafify(sd, TINY)


@pytest.fixture(scope="module")
def batches():
    return [synth_batch(seed, ilens, [3] * len(ilens))[:2] for seed, ilens in BATCHES]


def test_search_at_weight_zero_is_the_plain_beam(peaked):
    m = nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED)
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    got = nlm_ref.beam_search_nlm(peaked, TINY, xs, il, 4, m, 0.0)
    want = beam_ref.beam_search(peaked, TINY, xs, il, 4)
    for g, w in zip(got, want):
        assert g["tokens"] == w["tokens"] and g["score"] == w["score"]              # (float == float: the same bits)
        assert g["sel_gaps"] == w["sel_gaps"] and g["stop_gaps"] == w["stop_gaps"]


@pytest.mark.parametrize("lm_w", [0.5, 2.0])
def test_search_is_exhaustive_when_the_beam_holds_everything_that_matters(lm_w):
    C = 5                                                    # tokens 0 .. 4, eos = 4
    p = ref_cpu.leafify(ref_cpu.deterministic_state_dict(TINY, C, seed=5), TINY)
    m = nlm_ref.toy_nlm(C, 8, 12, 2, seed=4)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3: at most 25 running hypotheses < K
    for minr in (0.0, 0.5):
        got = nlm_ref.beam_search_nlm(p, TINY, xs, il, 64, m, lm_w, min_step_ratio=minr)
        want = nlm_ref.exhaustive_nlm(p, TINY, xs, il, m, lm_w, min_step_ratio=minr)
        for g, (tok, sc) in zip(got, want):
            assert g["tokens"] == tok, (g, tok, sc)
            assert abs(g["score"] - sc) <= 1e-5 * max(1.0, abs(sc))
    # K = 1 of the search is the step-by-step arg-max of the fused increment
    for g, (tok, sc) in zip(nlm_ref.beam_search_nlm(p, TINY, xs, il, 1, m, lm_w), nlm_ref.greedy_nlm(p, TINY, xs, il, m, lm_w)):
        assert g["tokens"] == tok and abs(g["score"] - sc) <= 1e-6 * max(1.0, abs(sc))


def test_k1_is_the_fused_argmax_chain_on_the_toy_model(peaked, batches):
    m = nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED)
    for xs, il in batches[1:2]:
        for g, (tok, sc) in zip(nlm_ref.beam_search_nlm(peaked, TINY, xs, il, 1, m, 0.5, min_step_ratio=0.5),
                                nlm_ref.greedy_nlm(peaked, TINY, xs, il, m, 0.5, min_step_ratio=0.5)):
            assert g["tokens"] == tok and abs(g["score"] - sc) <= 1e-6 * max(1.0, abs(sc))


SETTINGS = ((4, 0.5, 0.5), (4, 1.0, 0.5))


@pytest.fixture(scope="module")
def honest(peaked, batches):
    return {s: _search(peaked, batches, s, None) for s in SETTINGS}


def _search(p, batches, setting, mut):
    K, lm_w, minr = setting
    m = nlm_ref.toy_nlm(C_SMALL, 16, 24, 2, NLM_SEED)
    slots = [nlm_ref.zero_state(m) for _ in range(K)] if mut == "no_reset" else None
    return [(r["tokens"], r["score"]) for xs, il in batches for r in nlm_ref.beam_search_nlm(p, TINY, xs, il, K, m, lm_w, min_step_ratio=minr, mut=mut,
                                                                                             slots=slots)]


@pytest.mark.parametrize("mut", nlm_ref.MUTATIONS)
def test_mutated_restatements_change_results(peaked, batches, honest, mut):
    """each wrong variant changes at least one of the nine utterances' results (tokens or score) at some tested setting"""
    changed = {s: sum(a != b for a, b in zip(_search(peaked, batches, s, mut), honest[s])) for s in SETTINGS}
    print(f"{mut}: utterances whose result changes, per (K, lm_w, min ratio): {changed}")
    assert max(changed.values()) >= 1, changed


# ---------------------------------------------------------------- the checkpoint reader
def test_loader_accepts_both_key_layouts():
    m = nlm_ref.toy_nlm(9, 6, 10, 2, 1)
    want = None
    for sd in (nlm_ref.to_state_dict(m), {"model": nlm_ref.to_state_dict(m), "epoch": 3}, nlm_ref.to_state_dict(m, "predictor")):
        got = parse_state_dict(sd)
        assert got["embed"].shape == (9, 6) and got["lo_w"].shape == (9, 10) and len(got["w_ih"]) == 2
        assert got["w_ih"][0].shape == (40, 6) and got["w_ih"][1].shape == (40, 10) and got["embed"].dtype == np.float32
        flat = np.concatenate([got["embed"].ravel(), got["lo_w"].ravel(), got["lo_b"]] + [a.ravel() for k in ("w_ih", "w_hh", "b_ih", "b_hh") for a in got[k]])
        assert want is None or np.array_equal(flat, want)
        want = flat


def test_loader_names_missing_keys():
    sd = nlm_ref.to_state_dict(nlm_ref.toy_nlm(9, 6, 10, 2, 1))
    for gone in (["lo.bias"], ["rnn.weight_hh_l1"], ["embed.weight", "rnn.bias_ih_l0"]):
        bad = {k: v for k, v in sd.items() if k not in gone}
        with pytest.raises(ValueError) as e:
            parse_state_dict(bad)
        assert all(k in str(e.value) for k in gone), (gone, str(e.value))
    with pytest.raises(ValueError, match="embed.weight"):
        parse_state_dict({"encoder.weight": torch.zeros(2, 2)})
    pred = nlm_ref.to_state_dict(nlm_ref.toy_nlm(9, 6, 10, 1, 1), "predictor")
    del pred["predictor.rnn.0.bias_hh"]
    with pytest.raises(ValueError, match="predictor.rnn.0.bias_hh"):
        parse_state_dict(pred)
    wrong = dict(sd); wrong["lo.weight"] = torch.zeros(9, 11)
    with pytest.raises(ValueError, match="lo_w"):
        parse_state_dict(wrong)
    with pytest.raises(ValueError, match="dict"):
        parse_state_dict([1, 2])
