"""The CPU side of n-gram LM shallow fusion: the toy LM of tests/lm_ref.py is a normalised backoff model, the ARPA reader
(masr_amd.lm.read_arpa) returns its numbers and refuses what it must, and the restated search (lm_ref.beam_search_lm) is the plain beam
at lm_w = 0 and an exhaustive search when nothing that matters is pruned.  CPU only."""
import math

import numpy as np
import pytest

import beam_ref
import lm_ref
import masr_amd  # noqa: F401
from masr_amd.lm import read_arpa
from oracle import ref_cpu
from oracle.make_goldens import TINY, synth_batch
from decode_util import C_SMALL, peaked_state_dict


def _read(path, C):
    u = lm_ref.units(C)
    return read_arpa(path, {w: i for i, w in enumerate(u)}, 0, C - 1)


def _write(tmp_path, text, name="lm.arpa"):
    p = tmp_path / name
    p.write_text(text)
    return p


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_toy_lm_is_normalised(order):
    C = 9
    lm = lm_ref.toy_lm(C, order, seed=3)
    rng = np.random.RandomState(order)
    ctxs = {()} if order == 1 else set()
    for k in range(1, order):                               # contexts of every length the rule can meet: <s> first (short), or k units
        seen = [g for g in lm["grams"][k - 1] if C - 1 not in g]
        ctxs.update(seen[:40])                              # seen as n-grams (with and without the extension)
        for _ in range(40):                                 # random ones, mostly unseen from length 2 on
            ctxs.add(tuple(int(t) for t in rng.randint(1, C - 1, size=k)))
        ctxs.add((0,) + tuple(int(t) for t in rng.randint(1, C - 1, size=k - 1)))
    n_unseen = 0
    for ctx in sorted(ctxs):
        if len(ctx) < order - 1 and (not ctx or ctx[0] != 0):
            continue                                        # a context shorter than N - 1 starts with <s>
        n_unseen += bool(ctx) and ctx not in lm["grams"][len(ctx) - 1]
        s = sum(math.exp(lm_ref.lm_logprob64(lm, None, c, ctx=ctx)) for c in range(C))
        assert abs(s - 1.0) <= 1e-5, (order, ctx, s)
        for c in range(C):                                  # the fp32-ordered rule is the fp64 one within rounding
            assert abs(float(lm_ref.lm_logprob_ctx32(lm, ctx, c)) - lm_ref.lm_logprob64(lm, None, c, ctx=ctx)) <= 1e-5
    if order >= 3:
        assert n_unseen >= 10
    for d in lm["grams"]:
        for lp, bo in d.values():
            assert np.isfinite(lp) and np.isfinite(bo) and lp <= 0 and bo <= 0


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_arpa_round_trip(tmp_path, order):
    C = C_SMALL
    m10 = lm_ref.toy_lm_log10(C, order, seed=11)
    a = _read(_write(tmp_path, lm_ref.arpa_text(m10, lm_ref.units(C))), C)
    assert a.order == order and a.C == C and a.dropped == 0
    assert a.counts == [len(d) for d in m10]
    got, want = lm_ref.from_arrays(a), lm_ref.toy_lm(C, order, seed=11)
    for n in range(order):
        assert list(got["grams"][n].keys()) == list(want["grams"][n].keys())         # input order kept
        for g, (lp, bo) in want["grams"][n].items():
            assert got["grams"][n][g][0] == lp and got["grams"][n][g][1] == bo, (g, got["grams"][n][g], lp, bo)
        assert a.logp[n].dtype == np.float32 and a.backoff[n].dtype == np.float32 and a.grams[n].dtype == np.int32
    assert all(bo == 0 for bo in a.backoff[order - 1])
    lp10, bo10 = m10[0][(3,)]
    assert got["grams"][0][(3,)][0] == np.float32(np.float64(lp10) * math.log(10.0))


UNI = "".join(f"-1.0\t{w}\t-0.5\n" for w in ["<s>", "u1", "u2", "</s>"])
GOOD = "\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n" + UNI + "\n\\2-grams:\n-0.3\t<s> u1\n-0.4\tu1 u2\n\n\\end\\\n"


def test_reader_accepts_the_base_case(tmp_path):
    a = _read(_write(tmp_path, GOOD), 4)
    assert a.order == 2 and a.counts == [4, 2] and a.grams[1].tolist() == [[0, 1], [1, 2]]
    assert a.logp[1][0] == np.float32(np.float64(-0.3) * math.log(10.0)) and a.backoff[0][1] == np.float32(np.float64(-0.5) * math.log(10.0))


@pytest.mark.parametrize("name, text, line", [
    ("no data", GOOD.replace("\\data\\", "\\dat\\"), 1),
    ("bad header", GOOD.replace("ngram 2=2", "ngram two=2"), 3),
    ("count mismatch", GOOD.replace("ngram 2=2", "ngram 2=3"), 15),
    ("too few fields", GOOD.replace("-0.4\tu1 u2", "-0.4\tu1"), 13),
    ("bad number", GOOD.replace("-0.4\tu1 u2", "-0.x\tu1 u2"), 13),
    ("positive logp", GOOD.replace("-0.4\tu1 u2", "0.4\tu1 u2"), 13),
    ("positive backoff", GOOD.replace("-1.0\tu2\t-0.5", "-1.0\tu2\t0.5"), 8),
    ("order 5", "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 6)) + "\n\\end\\\n", 6),
    ("duplicate", GOOD.replace("-0.4\tu1 u2", "-0.4\t<s> u1"), 13),
    ("eos inside", GOOD.replace("-0.4\tu1 u2", "-0.4\t</s> u2"), 13),
    ("sos inside", GOOD.replace("-0.4\tu1 u2", "-0.4\tu1 <s>"), 13),
    ("section out of order", GOOD.replace("\\2-grams:", "\\3-grams:"), 11),
    ("no end", GOOD.replace("\\end\\\n", ""), 14),
    ("non-finite", GOOD.replace("-0.4\tu1 u2", "-inf\tu1 u2"), 13),
])
def test_reader_errors_name_the_line(tmp_path, name, text, line):
    with pytest.raises(ValueError, match=rf"line {line}\b"):
        _read(_write(tmp_path, text), 4)


def test_unk_fills_missing_unigrams(tmp_path):
    text = GOOD.replace("-1.0\tu2\t-0.5\n", "-2.5\t<unk>\n")
    a = _read(_write(tmp_path, text.replace("-0.4\tu1 u2", "-0.4\tu1 </s>")), 4)
    lm = lm_ref.from_arrays(a)
    assert a.counts[0] == 4 and lm["grams"][0][(2,)] == (np.float32(np.float64(-2.5) * math.log(10.0)), np.float32(0.0))
    with pytest.raises(ValueError, match="<unk>"):            # no <unk> to stand in
        _read(_write(tmp_path, GOOD.replace("ngram 1=4", "ngram 1=3").replace("-1.0\tu2\t-0.5\n", "").replace("-0.4\tu1 u2", "-0.4\tu1 </s>")), 4)


def test_dropped_ngrams_are_counted(tmp_path, capsys):
    text = GOOD.replace("ngram 2=2", "ngram 2=4").replace("-0.4\tu1 u2\n", "-0.4\tu1 u2\n-0.7\tu1 zz\n-0.8\t<unk> u2\n")
    a = _read(_write(tmp_path, text), 4)
    assert a.dropped == 2 and a.counts == [4, 2]
    out = capsys.readouterr()
    assert "dropped 2 n-grams" in out.out + out.err


@pytest.fixture(scope="module")
def peaked():
    return ref_cpu.leafify(peaked_state_dict(TINY, 7), TINY)


def test_search_at_weight_zero_is_the_plain_beam(peaked):
    lm = lm_ref.toy_lm(C_SMALL, 3, seed=2)
    xs, il, _, _ = synth_batch(12, [48, 48, 44], [3] * 3)
    got = lm_ref.beam_search_lm(peaked, TINY, xs, il, 4, lm, 0.0)
    want = beam_ref.beam_search(peaked, TINY, xs, il, 4)
    for g, w in zip(got, want):
        assert g["tokens"] == w["tokens"] and g["score"] == w["score"]
        assert g["sel_gaps"] == w["sel_gaps"] and g["stop_gaps"] == w["stop_gaps"]


@pytest.mark.parametrize("lm_w", [0.5, 2.0])
def test_search_is_exhaustive_when_the_beam_holds_everything_that_matters(lm_w):
    C = 5                                                    # tokens 0 .. 4, eos = 4
    p = ref_cpu.leafify(ref_cpu.deterministic_state_dict(TINY, C, seed=5), TINY)
    lm = lm_ref.toy_lm(C, 3, seed=4)
    xs, il, _, _ = synth_batch(21, [12, 13, 14, 15], [1, 1, 1, 1])          # enc_len 3 -> maxlen 3: at most 25 running hypotheses < K
    for minr in (0.0, 0.5):
        got = lm_ref.beam_search_lm(p, TINY, xs, il, 64, lm, lm_w, min_step_ratio=minr)
        want = lm_ref.exhaustive_lm(p, TINY, xs, il, lm, lm_w, min_step_ratio=minr)
        for g, (tok, sc) in zip(got, want):
            assert g["tokens"] == tok, (g, tok, sc)
            assert abs(g["score"] - sc) <= 1e-5 * max(1.0, abs(sc))
    # K = 1 of the search is the step-by-step arg-max
    for g, (tok, sc) in zip(lm_ref.beam_search_lm(p, TINY, xs, il, 1, lm, lm_w), lm_ref.greedy_lm(p, TINY, xs, il, lm, lm_w)):
        assert g["tokens"] == tok and abs(g["score"] - sc) <= 1e-6 * max(1.0, abs(sc))
