"""What MasrEngine's decode methods hand to the library, without a device: the real methods of an engine made with MasrEngine.__new__ run
against a stand-in for libmasr that records every call (the twin of test_decode_args_cpu.py, which pins the C side of the same calls).  Per
method: the recorded calls -- names, and every argument that is no pointer -- against literals; the pointers against the tensors they must
belong to; every argument's Python type against its slot in _cabi._SIGS (a float in an int's place shows here); the raw tensors' shapes and
dtypes; and the lists of raw=False for a fixed pattern that the stand-in writes through the output pointers.  Then the Python-side refusals:
the full text, and that the library was never called.  The literals were recorded from the engine before its decode methods were folded
into one runner: a change that moves a float into another float's slot, reorders two checks or converts a result differently shows here."""
import ctypes as C
import inspect
import math
from types import SimpleNamespace

import pytest
import torch

import masr_amd  # noqa: F401
from masr_amd import _cabi
from masr_amd.bias import ContextBias
from masr_amd.engine import MasrEngine

P, NAN, INF, I, F = "ptr", float("nan"), float("inf"), torch.int32, torch.float32
LM, NLM, DEAD_LM, DEAD_NLM = SimpleNamespace(h="LM"), SimpleNamespace(h="NLM", score=1), SimpleNamespace(h=None), SimpleNamespace(h=None, score=1)
BIAS = ContextBias.__new__(ContextBias)
BIAS.h = "BIAS"


@pytest.fixture(scope="module", autouse=True)
def _no_handle_left():
    yield
    BIAS.h = None                                               # (its __del__ would hand the stand-in handle to the real library)


def norm(args):
    return tuple(P if isinstance(a, C.c_void_p) else a for a in args)


class Lib:
    """every attribute is a library function that records (name, args) and returns 0.  Once the record equals `calls` -- so the shapes are
    the expected ones -- it writes a fixed pattern through the last len(outs) pointers of that call: the tokens 1..5, the lens 3, 1, -1, 2,
    other ints counting up, floats -0.5 * (i + 1) - the output's index"""
    def __init__(self, calls=(), outs=()):
        self.calls, self._want, self._outs = [], list(calls), outs

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if self._outs and [(n, norm(a)) for n, a in self.calls] == self._want:
                ptrs = [a.value for a in args if isinstance(a, C.c_void_p)][-len(self._outs):]
                for k, (p, (shape, dt)) in enumerate(zip(ptrs, self._outs)):
                    n = math.prod(shape)
                    vals = [-0.5 * (i + 1) - k for i in range(n)] if dt is F else [(1 + i % 5, (3, 1, -1, 2)[i % 4], i)[min(k, 2)] for i in range(n)]
                    ((C.c_float if dt is F else C.c_int32) * n).from_address(p)[:] = vals
            return 0
        return fn


def engine(calls=(), outs=()):
    e = MasrEngine.__new__(MasrEngine)
    e.device, e.h, e.ws, e._dirty, e.stream, e._l = torch.device("cpu"), "M", torch.zeros(1, dtype=torch.uint8), False, (lambda: "S"), Lib(calls, outs)
    return e


def call(e, name, **over):
    """the method with those of the fixed inputs that it takes, by keyword -> (its result, the inputs)"""
    kw = dict(xs=torch.zeros(2, 40, 80), ilens=torch.tensor([40, 36]), beam_size=4, nbest=2, min_step_ratio=0.125, max_step_ratio=0.75,
              att_weight=0.625, ctc_weight=0.375, att_w=0.625, ctc_w=0.375, lm=LM, nlm=NLM, lm_w=0.25, len_bonus=0.5, bias=BIAS, bias_w=2.5,
              ys=[[5, 6, 7], [8, 9]], olens=torch.tensor([3, 2]), tokens=torch.tensor([[[5, 6, 7], [5, 6, 0]], [[8, 9, 0], [0, 0, 0]]], dtype=I),
              lens=torch.tensor([[3, 2], [2, -1]], dtype=I), ctc=torch.tensor([[-1.0, -2.0], [-1.5, 0.0]]))
    kw.update(over)
    fn = getattr(e, name)
    return fn(**{k: kw[k] for k in inspect.signature(fn).parameters if k in kw}), kw


def plain(x):
    """a result with its tensors as lists"""
    return x.tolist() if isinstance(x, torch.Tensor) else type(x)(plain(v) for v in x) if isinstance(x, (list, tuple)) else x


# (method, what it is called with beside the fixed inputs, the recorded calls, the raw tensors, the result of raw=False under Lib's pattern)
STEP, STEP_L = [((2, 7), I), ((2,), I), ((2,), F)], ([[1, 2, 3], [3]], [-2.5, -3.0])                    # Lmax = 7; tokens, lens, scores
JOINT, JOINT_L = [((2, 2, 7), I), ((2, 2), I), ((2, 2), F)], [[([1, 2, 3], -2.5), ([3], -3.0)], [([2, 3], -4.0)]]
CTC = [((2, 2, 10), I), ((2, 2), I), ((2, 2), F)]                                                           # T // 4 = 10
CTC_LM, CTC_LM_L = CTC + [((2, 2), F)], [[([1, 2, 3], -2.5, -3.5), ([1], -3.0, -4.0)], [([1, 2], -4.0, -5.0)]]
CTC_BIAS, CTC_BIAS_L = CTC_LM + [((2, 2), I)], [[([1, 2, 3], -2.5, -3.5, 0), ([1], -3.0, -4.0, 1)], [([1, 2], -4.0, -5.0, 3)]]
RESC = CTC + [((2, 2), F), ((2, 2), F), ((2, 2), I)]
RESC_L = [[([1, 2, 3], -2.5, -3.5, -4.5, 0), ([1], -3.0, -4.0, -5.0, 1)], [([1, 2], -4.0, -5.0, -6.0, 3)]]
GREEDY_L = [[1, 2], [3, 4], [5, 1], [2, 3], [4, 5], [1, 2], [3, 4], [5, 1], [2, 3], [4, 5]]
CASES = [
    ('recog', {}, [('masr_workspace_bytes', ('M', 2, 40, 10)), ('masr_recog', ('M', P, P, 2, 40, P, 'S'))], [((10, 2), I)], GREEDY_L),
    ('recog', dict(full=True), [('masr_workspace_bytes', ('M', 2, 40, 10)), ('masr_recog_full', ('M', P, P, 2, 40, P, 'S'))], [((10, 2), I)], GREEDY_L),
    ('recog_beam', {}, [('masr_beam_ctc_workspace_bytes', ('M', 2, 40, 4, 7)),
                        ('masr_recog_beam_ctc', ('M', P, P, 2, 40, 4, 0.125, 0.75, 0.625, 0.375, P, P, P, 'S'))], STEP, STEP_L),
    ('recog_beam', dict(ctc_weight=0.0), [('masr_beam_workspace_bytes', ('M', 2, 40, 4, 7)),
                                          ('masr_recog_beam', ('M', P, P, 2, 40, 4, 0.125, 0.75, P, P, P, 'S'))], STEP, STEP_L),
    ('recog_beam_lm', {}, [('masr_beam_lm_workspace_bytes', ('M', 2, 40, 4, 7)),
                           ('masr_recog_beam_lm', ('M', 'LM', P, P, 2, 40, 4, 0.125, 0.75, 0.25, P, P, P, 'S'))], STEP, STEP_L),
    ('recog_beam_nlm', {}, [('masr_beam_nlm_workspace_bytes', ('M', 'NLM', 2, 40, 4, 7)),
                            ('masr_recog_beam_nlm', ('M', 'NLM', P, P, 2, 40, 4, 0.125, 0.75, 0.25, P, P, P, 'S'))], STEP, STEP_L),
    ('recog_beam_ctc_lm', {}, [('masr_beam_ctc_lm_workspace_bytes', ('M', 2, 40, 4, 2, 7)),
                               ('masr_recog_beam_ctc_lm', ('M', 'LM', P, P, 2, 40, 4, 2, 0.125, 0.75, 0.625, 0.375, 0.25, 0.5, P, P, P, 'S'))], JOINT, JOINT_L),
    ('recog_beam_ctc_nlm', {}, [('masr_beam_ctc_nlm_workspace_bytes', ('M', 'NLM', 2, 40, 4, 2, 7)),
                                ('masr_recog_beam_ctc_nlm', ('M', 'NLM', P, P, 2, 40, 4, 2, 0.125, 0.75, 0.625, 0.375, 0.25, 0.5, P, P, P, 'S'))], JOINT, JOINT_L),
    ('recog_ctc_beam', {}, [('masr_ctc_beam_workspace_bytes', ('M', 2, 40, 4)), ('masr_recog_ctc_beam', ('M', P, P, 2, 40, 4, 2, P, P, P, 'S'))],
     CTC, [[([1, 2, 3], -2.5), ([1], -3.0)], [([1, 2], -4.0)]]),
    ('recog_ctc_beam_lm', {}, [('masr_ctc_beam_workspace_bytes', ('M', 2, 40, 4)),
                               ('masr_recog_ctc_beam_lm', ('M', 'LM', P, P, 2, 40, 4, 2, 0.25, 0.5, P, P, P, P, 'S'))], CTC_LM, CTC_LM_L),
    ('recog_ctc_beam_nlm', {}, [('masr_ctc_beam_nlm_workspace_bytes', ('M', 'NLM', 2, 40, 4)),
                                ('masr_recog_ctc_beam_nlm', ('M', 'NLM', P, P, 2, 40, 4, 2, 0.25, 0.5, P, P, P, P, 'S'))], CTC_LM, CTC_LM_L),
    ('recog_ctc_beam_bias', {}, [('masr_ctc_beam_workspace_bytes', ('M', 2, 40, 4)),
                                 ('masr_recog_ctc_beam_bias', ('M', 'LM', 'BIAS', P, P, 2, 40, 4, 2, 0.25, 0.5, 2.5, P, P, P, P, P, 'S'))], CTC_BIAS, CTC_BIAS_L),
    ('recog_ctc_beam_bias', dict(lm=None), [('masr_ctc_beam_workspace_bytes', ('M', 2, 40, 4)),
                                            ('masr_recog_ctc_beam_bias', ('M', None, 'BIAS', P, P, 2, 40, 4, 2, 0.0, 0.0, 2.5, P, P, P, P, P, 'S'))],
     CTC_BIAS, CTC_BIAS_L),
    ('recog_beam_bias', {}, [('masr_beam_bias_workspace_bytes', ('M', 2, 40, 4, 7)),
                             ('masr_recog_beam_bias', ('M', 'LM', 'BIAS', P, P, 2, 40, 4, 0.125, 0.75, 0.25, 2.5, P, P, P, P, 'S'))],
     STEP + [((2,), I)], (*STEP_L, [0, 1])),
    ('recog_beam_bias', dict(lm=None), [('masr_beam_bias_workspace_bytes', ('M', 2, 40, 4, 7)),
                                        ('masr_recog_beam_bias', ('M', None, 'BIAS', P, P, 2, 40, 4, 0.125, 0.75, 0.0, 2.5, P, P, P, P, 'S'))],
     STEP + [((2,), I)], (*STEP_L, [0, 1])),
    ('recog_beam_ctc_bias', {}, [('masr_beam_ctc_bias_workspace_bytes', ('M', 2, 40, 4, 2, 7)),
                                 ('masr_recog_beam_ctc_bias', ('M', 'LM', 'BIAS', P, P, 2, 40, 4, 2, 0.125, 0.75, 0.625, 0.375, 0.25, 0.5, 2.5, P, P, P, P, 'S'))],
     JOINT + [((2, 2), I)], [[([1, 2, 3], -2.5, 0), ([3], -3.0, 1)], [([2, 3], -4.0, 3)]]),
    ('recog_beam_ctc_bias', dict(lm=None), [('masr_beam_ctc_bias_workspace_bytes', ('M', 2, 40, 4, 2, 7)),
                                            ('masr_recog_beam_ctc_bias', ('M', None, 'BIAS', P, P, 2, 40, 4, 2, 0.125, 0.75, 0.625, 0.375, 0.0, 0.5, 2.5, P, P, P, P, 'S'))],
     JOINT + [((2, 2), I)], [[([1, 2, 3], -2.5, 0), ([3], -3.0, 1)], [([2, 3], -4.0, 3)]]),
    ('recog_rescore', {}, [('masr_rescore_workspace_bytes', ('M', 2, 40, 4, 2, 10)),
                           ('masr_recog_rescore', ('M', P, P, 2, 40, 4, 2, 0.625, 0.375, P, P, P, P, P, P, 'S'))], RESC, RESC_L),
    ('recog_rescore_lm', {}, [('masr_rescore_workspace_bytes', ('M', 2, 40, 4, 2, 10)),
                              ('masr_recog_rescore_lm', ('M', 'LM', P, P, 2, 40, 4, 2, 0.25, 0.5, 0.625, 0.375, P, P, P, P, P, P, 'S'))], RESC, RESC_L),
    ('recog_rescore_nlm', {}, [('masr_rescore_nlm_workspace_bytes', ('M', 'NLM', 2, 40, 4, 2, 10)),
                               ('masr_recog_rescore_nlm', ('M', 'NLM', P, P, 2, 40, 4, 2, 0.25, 0.5, 0.625, 0.375, P, P, P, P, P, P, 'S'))], RESC, RESC_L),
    ('recog_rescore_bias', {}, [('masr_rescore_workspace_bytes', ('M', 2, 40, 4, 2, 10)),
                                ('masr_recog_rescore_bias', ('M', 'LM', 'BIAS', P, P, 2, 40, 4, 2, 0.25, 0.5, 2.5, 0.625, 0.375, P, P, P, P, P, P, 'S'))], RESC, RESC_L),
    ('recog_rescore_bias', dict(lm=None), [('masr_rescore_workspace_bytes', ('M', 2, 40, 4, 2, 10)),
                                           ('masr_recog_rescore_bias', ('M', None, 'BIAS', P, P, 2, 40, 4, 2, 0.0, 0.0, 2.5, 0.625, 0.375, P, P, P, P, P, P, 'S'))],
     RESC, RESC_L),
    ('ctc_align', {}, [('masr_ctc_align_workspace_bytes', ('M', 2, 40, 3)), ('masr_recog_ctc_align', ('M', P, P, 2, 40, P, P, 3, P, P, P, P, 'S'))],
     [((2, 10), I), ((2, 3), I), ((2, 3), I), ((2,), F)],
     [(-3.5, [(5, 3, 0), (6, 1, 1), (7, -1, 2)], [1, 2, 3, 4, 5, 1, 2, 3, 4, 5]), (-4.0, [(8, 2, 3), (9, 3, 4)], [1, 2, 3, 4, 5, 1, 2, 3, 4, 5])]),
    ('rescore_nbest', {}, [('masr_rescore_workspace_bytes', ('M', 2, 40, 2, 2, 3)),
                           ('masr_rescore_nbest', ('M', P, P, 2, 40, 2, P, 3, P, P, 0.625, 0.375, P, P, P, P, P, P, 'S'))],
     [((2, 2, 3), I), ((2, 2), I), ((2, 2), F), ((2, 2), F), ((2, 2), F), ((2, 2), I)],
     [[([1, 2, 3], -2.5, -3.5, -4.5, 0), ([4], -3.0, -4.0, -5.0, 1)], [([5, 1], -4.0, -5.0, -6.0, 3)]]),
]
MID ={"rescore_nbest": ("tokens", "lens", "ctc"), "ctc_align": (None, "olens")}   # the pointers between ilens and the outputs (None: a copy)


@pytest.mark.parametrize("name, over, calls, outs, lists", CASES, ids=[f"{c[0]}{sorted(c[1]) or ''}" for c in CASES])
def test_decode_call(name, over, calls, outs, lists):
    has_raw = "raw" in inspect.signature(getattr(MasrEngine, name)).parameters
    e = engine(calls, outs)
    res, kw = call(e, name, **over, **({"raw": True} if has_raw else {}))
    assert [(n, norm(a)) for n, a in e._l.calls] == calls
    for n, args in e._l.calls:
        sig = _cabi._SIGS[n][1]
        assert len(args) == len(sig), n
        for j, (a, s) in enumerate(zip(args, sig)):
            ok = type(a) is int if s in (_cabi.i32, _cabi.i64) else type(a) is float if s is _cabi.f32 else \
                s is _cabi.vp and (a is None or isinstance(a, (C.c_void_p, str)))
            assert ok, f"{n}: argument {j} is {a!r}"
    ptrs = [a.value for a in e._l.calls[-1][1] if isinstance(a, C.c_void_p)]
    want = [e._last_x, kw["ilens"], *[k and kw[k] for k in MID.get(name, ())], *(res if has_raw else [None] * len(outs))]
    assert e._last_x is kw["xs"] and len(ptrs) == len(want)
    assert [t is None or p == t.data_ptr() for p, t in zip(ptrs, want)] == [True] * len(want)
    if has_raw:
        assert [(tuple(t.shape), t.dtype) for t in res] == outs
        e = engine(calls, outs)
        res, _ = call(e, name, **over)
        assert [(n, norm(a)) for n, a in e._l.calls] == calls
    assert plain(res) == lists


METHODS = sorted({c[0] for c in CASES})
FAULTS = [                                                      # (argument, value, the ValueError's text), on every method that has the argument
    ("beam_size", 0, "beam_size must be in [1, 64], got 0"), ("beam_size", 65, "beam_size must be in [1, 64], got 65"),
    ("nbest", 0, "nbest must be in [1, beam_size], got 0"), ("nbest", 5, "nbest must be in [1, beam_size], got 5"),
    ("lm_w", -1.0, "lm_w must be finite and >= 0, got -1.0"), ("lm_w", NAN, "lm_w must be finite and >= 0, got nan"),
    ("len_bonus", INF, "len_bonus must be finite, got inf"), ("bias_w", -1.0, "bias_w must be finite and >= 0, got -1.0"),
    ("att_w", 0.0, "att_w must be finite and > 0, got 0.0"), ("ctc_w", -1.0, "ctc_w must be finite and >= 0, got -1.0"),
    ("lm", DEAD_LM, "lm must be a live NGramLM"), ("nlm", DEAD_NLM, "lm must be a live LstmLM"), ("bias", "BIAS", "bias must be a live ContextBias")]
TWO_FAULTS = [                                                  # (method, arguments, the text): the check that answers first
    ("recog_beam_ctc_lm", dict(beam_size=65, lm_w=-1.0), "beam_size must be in [1, 64], got 65"),
    ("recog_beam_ctc_nlm", dict(nbest=0, len_bonus=INF), "nbest must be in [1, beam_size], got 0"),
    ("recog_rescore_bias", dict(nbest=5, att_w=0.0), "nbest must be in [1, beam_size], got 5"),
    ("recog_rescore_bias", dict(ctc_w=-1.0, bias_w=-1.0), "ctc_w must be finite and >= 0, got -1.0"),
    ("recog_rescore_bias", dict(bias="BIAS", lm_w=-1.0), "bias must be a live ContextBias"),
    ("recog_rescore_lm", dict(att_w=0.0, lm=DEAD_LM), "att_w must be finite and > 0, got 0.0"),
    ("recog_rescore_nlm", dict(ctc_w=-1.0, lm_w=NAN), "ctc_w must be finite and >= 0, got -1.0"),
    ("recog_ctc_beam_bias", dict(bias_w=-1.0, len_bonus=INF), "bias_w must be finite and >= 0, got -1.0"),
    ("recog_beam_bias", dict(bias="BIAS", lm_w=-1.0), "bias must be a live ContextBias"),
    ("recog_beam_ctc_bias", dict(lm=None, bias="BIAS", len_bonus=INF), "bias must be a live ContextBias"),
    ("recog_ctc_beam_lm", dict(lm_w=-1.0, lm=DEAD_LM), "lm_w must be finite and >= 0, got -1.0")]
IGNORED = ("recog_beam_bias", "recog_ctc_beam_bias", "recog_rescore_bias")     # without an LM these read neither lm_w nor len_bonus


def refused(name, **over):
    e = engine()
    with pytest.raises(ValueError) as err:
        call(e, name, **over)
    assert e._l.calls == []
    return str(err.value)


@pytest.mark.parametrize("arg, value, text", FAULTS, ids=[f"{f[0]}={getattr(f[1], 'h', f[1])}" for f in FAULTS])
def test_refusals(arg, value, text):
    hit = [m for m in METHODS if arg in inspect.signature(getattr(MasrEngine, m)).parameters]
    assert hit and [refused(m, **{arg: value}) for m in hit] == [text] * len(hit)


def test_refusals_order_and_no_lm():
    for name, over, text in TWO_FAULTS:
        assert refused(name, **over) == text, (name, over)
    assert refused("recog_beam_ctc_bias", lm=None, len_bonus=INF) == "len_bonus must be finite, got inf"
    for name in IGNORED:                                        # not vetted there: the call is the one of the fixed inputs without an LM
        e = engine()
        call(e, name, lm=None, lm_w=NAN, len_bonus=INF, raw=True)
        assert [(n, norm(a)) for n, a in e._l.calls] == next(c[2] for c in CASES if c[0] == name and c[1] == dict(lm=None))
