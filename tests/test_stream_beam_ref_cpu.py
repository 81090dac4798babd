"""The resumable CTC prefix beam without a GPU: stable_prefix on the restatement of tests/ctc_beam_ref.py run on logits truncated
at every frame -- what a partial result is --, the Tester's argument errors for stream_sync_ctc_beam, Tester.MODES against the CLI's choices,
and the new symbols of include/masr.h in the ctypes table."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import masr_amd  # noqa: F401
import ctc_beam_ref as cr
import lm_ref
from masr_amd import _cabi
from masr_amd import tester as tester_mod
from masr_amd._cabi import stable_prefix
from masr_amd.tester import stream_decode_args
from oracle.make_goldens import TINY

REPO = Path(__file__).resolve().parents[1]


def test_stable_prefix_of_lists():
    assert stable_prefix([]) == []
    assert stable_prefix([([], 0.0)]) == []
    assert stable_prefix([([3, 4, 5], -1.0)]) == [3, 4, 5]
    assert stable_prefix([([3, 4, 5], -1.0), ([3, 4], -2.0), ([3, 4, 7, 1], -2.5)]) == [3, 4]
    assert stable_prefix([([3, 4], -1.0, -0.5, 2), ([2, 4], -2.0, -1.0, 0)]) == []      # entries with more fields (an LM, a phrase list)
    assert stable_prefix([([3], -1.0), ([], -2.0)]) == []


@pytest.mark.parametrize("name", ["basic", "few_classes", "peaky_merge", "no_eos", "neg_inf", "wide_367"])
def test_stable_prefix_only_grows_and_ends_in_the_best_hypothesis(name):
    """the partial result after t frames is the search on the logits truncated at t (the search is causal).  Every entry of a later beam
    extends an entry of the current one, so the common prefix of the whole K-best never shrinks and is a prefix of the final top-1."""
    cs, z, lens = cr.make_case(name)
    K = max(cs["Ks"])
    points = non_empty = 0
    for b, n in enumerate(lens.tolist()):
        zb = np.ascontiguousarray(z[b, :n, :cs["C"]])
        before = []
        for t in range(n + 1):
            full = cr.ctc_beam_ref(zb[:t], K, 0, cs["eos"], K)["nbest"]
            now = stable_prefix(full)
            assert list(now[:len(before)]) == list(before), (name, b, t, before, now)
            before = now
            points += 1
            non_empty += len(now) > 0
        assert list(full[0][0][:len(before)]) == list(before), (name, b)
    print(f"{name}: K = {K}, a non-empty stable prefix at {non_empty} of {points} truncation points")
    assert points == sum(int(n) + 1 for n in lens) and non_empty >= 1


def test_tester_argument_errors():
    hybrid = dict(TINY, ctc_weight=0.3)
    paras = lambda **kw: SimpleNamespace(**kw)  # noqa: E731
    pol = dict(size=8, left=-1, dynamic=0)
    mode = "stream_sync_ctc_beam"
    assert mode in tester_mod.STREAM_MODES
    assert stream_decode_args(hybrid, paras(), mode, pol) == 32
    assert stream_decode_args(hybrid, paras(stream_piece=7), mode, pol) == 7
    with pytest.raises(ValueError, match="stream_sync_ctc_beam: no chunk size; pass --decode_chunk"):
        stream_decode_args(hybrid, paras(), mode, None)
    with pytest.raises(ValueError, match="--decode_chunk"):
        stream_decode_args(hybrid, paras(), mode, dict(size=0, left=-1, dynamic=1))
    with pytest.raises(ValueError, match="'stream_sync_ctc_beam' needs a CTC output layer"):
        stream_decode_args(TINY, paras(), mode, pol)
    with pytest.raises(ValueError, match="--stream_piece"):
        stream_decode_args(hybrid, paras(stream_piece=0), mode, pol)
    with pytest.raises(NotImplementedError, match="BLSTM"):
        stream_decode_args(hybrid, paras(), mode, None, model_name="blstm")


def test_mode_table_and_cli():
    import train
    T = tester_mod.Tester
    act = next(a for a in train.build_parser()._actions if a.dest == "decode_mode")
    assert set(act.choices) == set(T.MODES) and "stream_sync_ctc_beam" in T.MODES
    settings, best, what = T.MODES["stream_sync_ctc_beam"]
    assert settings is T._stream_settings and callable(best)
    assert "resumable" in what(SimpleNamespace(chunk_policy=dict(size=8), beam_size=7)) and "beam 7" in what(SimpleNamespace(chunk_policy=dict(size=8), beam_size=7))
    a = train.build_parser().parse_args(["--config", "x", "--accent", "af", "--algo", "no", "--test", "--decode_mode", "stream_sync_ctc_beam",
                                         "--decode_chunk", "8", "--lm_model_path", "lm.arpa", "--context_path", "ctx.txt"])
    assert a.decode_mode == "stream_sync_ctc_beam" and a.lm_model_path == "lm.arpa" and a.context_path == "ctx.txt"
    # the mode hands the engine the final lists of a beam that followed the feeds, with the Tester's LM, phrase list and weights
    calls = []

    def recog_stream(xs, il, piece, beam_size, **kw):
        calls.append((xs, il, piece, beam_size, kw))
        return [[([5, 6], -1.0)], [([], -2.0)]], [[[5], []]]

    stub = SimpleNamespace(asr_model=SimpleNamespace(engine=SimpleNamespace(recog_stream=recog_stream)), stream_piece=32, beam_size=7, lm="LM", lm_weight=0.4,
                           len_bonus=0.1, bias="BIAS", bias_weight=2.5, model_name="transformer", _ctc_best=lambda lists: [n[0][0] for n in lists])
    assert best(stub, "xs", "il") == [[5, 6], []]
    assert calls == [("xs", "il", 32, 7, dict(sync_beam=True, lm="LM", lm_w=0.4, len_bonus=0.1, bias="BIAS", bias_w=2.5))]


def settings_tester(block, lm_path=None, ctx_path=None, head=True):
    """a Tester made with Tester.__new__ that carries only what _stream_settings reads (test_tester_bias_settings_cpu.py's form)"""
    t = tester_mod.Tester.__new__(tester_mod.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=lm_path, context_path=ctx_path)
    t.decode_mode, t.model_name = "stream_sync_ctc_beam", "transformer"
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = lm_ref.units(13), 0, 12, 0
    return t


@pytest.fixture
def lm_and_phrase_files(tmp_path, monkeypatch):
    """a small ARPA file and a phrase file over 13 units, read by the real readers; only the two device constructors are replaced (they
    allocate on the GPU), by ones that keep what the readers handed them"""
    from masr_amd import bias as bias_mod, lm as lm_mod
    arpa, ctx = tmp_path / "toy.arpa", tmp_path / "phrases.txt"
    arpa.write_text(lm_ref.arpa_text(lm_ref.toy_lm_log10(13, 3, 5, n_sent=40, max_len=6), lm_ref.units(13)))
    ctx.write_text("3 4 5\n\n7\n3 4\n")

    def lm_init(self, order, C_, grams, logp, backoff):
        self.h, self.order, self.C, self.counts = None, int(order), int(C_), [len(g) for g in grams]

    def bias_init(self, C_, phrases):
        self.h, self.C, self.phrases, self.lists = None, int(C_), len(phrases), [list(p) for p in phrases]

    monkeypatch.setattr(lm_mod.NGramLM, "__init__", lm_init)
    monkeypatch.setattr(bias_mod.ContextBias, "__init__", bias_init)
    return str(arpa), str(ctx)


def test_settings_read_the_lm_and_the_phrase_list(lm_and_phrase_files):
    arpa, ctx = lm_and_phrase_files
    t = settings_tester({"beam_size": 6, "lm_w": 0.6, "len_bonus": -0.2, "bias_w": 2.5}, arpa, ctx)
    t._stream_settings()
    assert t.beam_size == 6 and (t.lm_weight, t.len_bonus, t.bias_weight) == (0.6, -0.2, 2.5)
    assert t.lm.order == 3 and t.lm.C == 13 and len(t.lm.counts) == 3 and all(c > 0 for c in t.lm.counts)
    assert t.bias.C == 13 and t.bias.lists == [[3, 4, 5], [7], [3, 4]]
    # the defaults of lm_ctc_beam and bias_ctc_beam
    t = settings_tester({"beam_size": 6}, arpa, ctx)
    t._stream_settings()
    assert (t.lm_weight, t.len_bonus, t.bias_weight) == (0.3, 0.0, 3.0)
    # each alone; what belongs to the absent one is not read
    t = settings_tester({"beam_size": 6, "lm_w": 0.5, "bias_w": float("nan")}, arpa, None)
    t._stream_settings()
    assert t.lm.order == 3 and t.bias is None and (t.lm_weight, t.bias_weight) == (0.5, 0.0)
    t = settings_tester({"beam_size": 6, "lm_w": -1.0, "len_bonus": float("nan"), "bias_w": 1.5}, None, ctx)
    t._stream_settings()
    assert t.lm is None and t.bias.phrases == 3 and (t.lm_weight, t.len_bonus, t.bias_weight) == (0.0, 0.0, 1.5)
    t = settings_tester({"beam_size": 6, "lm_w": -1.0, "bias_w": -1.0})
    t._stream_settings()
    assert t.lm is None and t.bias is None and (t.lm_weight, t.len_bonus, t.bias_weight) == (0.0, 0.0, 0.0)


def test_settings_refusals(lm_and_phrase_files, tmp_path):
    arpa, ctx = lm_and_phrase_files

    def refused(exc, block, lm_path=None, ctx_path=None, **kw):
        with pytest.raises(exc) as e:
            settings_tester(block, lm_path, ctx_path, **kw)._stream_settings()
        return str(e.value)
    assert refused(ValueError, None) == "decode_mode 'stream_sync_ctc_beam' needs a solver.beam_decode block with at least beam_size in the config"
    assert refused(ValueError, {"beam_size": 65}) == "solver.beam_decode.beam_size must be in [1, 64], got 65"
    assert refused(ValueError, {"beam_size": 4}, head=False).startswith("decode_mode 'stream_sync_ctc_beam' needs a CTC output layer")
    assert refused(ValueError, {"beam_size": 4, "lm_w": -1.0}, arpa) == "solver.beam_decode.lm_w must be finite and >= 0, got -1.0"
    assert refused(ValueError, {"beam_size": 4, "len_bonus": float("nan")}, arpa) == "solver.beam_decode.len_bonus must be finite, got nan"
    assert refused(ValueError, {"beam_size": 4, "bias_w": float("inf")}, None, ctx) == "solver.beam_decode.bias_w must be finite and >= 0, got inf"
    bad = tmp_path / "bad.txt"
    bad.write_text("3 4\n5 x 6\n")
    assert refused(ValueError, {"beam_size": 4}, None, str(bad)).endswith(":2: a phrase is a list of unit ids, got '5 x 6'")
    with pytest.raises(FileNotFoundError):
        settings_tester({"beam_size": 4}, str(tmp_path / "none.arpa"))._stream_settings()


def test_new_symbols_are_bound():
    text = (REPO / "include" / "masr.h").read_text()
    declared = set(re.findall(r"\b(masr_ctc_beam_run_[a-z0-9_]+|masr_stream_beam_[a-z0-9_]+)\s*\(", text))
    assert declared == {"masr_ctc_beam_run_work_bytes", "masr_ctc_beam_run_open", "masr_ctc_beam_run_advance", "masr_ctc_beam_run_result",
                        "masr_ctc_beam_run_close", "masr_stream_beam_open", "masr_stream_beam_result"}
    assert declared <= set(_cabi.EXPORTS)
    sig = _cabi._SIGS
    assert len(sig["masr_ctc_beam_run_open"][1]) == 17 and len(sig["masr_ctc_beam_run_advance"][1]) == 3
    assert len(sig["masr_ctc_beam_run_result"][1]) == 8 and len(sig["masr_stream_beam_open"][1]) == 8 and len(sig["masr_stream_beam_result"][1]) == 8
