"""What the decoders' C entry points answer on the host, without a device: every `*_workspace_bytes` query and every argument check
of csrc/recog.hip, on the hkust geometry once plain (masr_create) and once with a CTC head (masr_create_ctc).  A model handle that was
never bound answers all of them; a valid call ends at `masr_recog: not bound`.  The expected values are literals recorded from the
library before its host code was refactored: byte counts, return codes and the full masr_last_error() texts, so that a change of the
host code that moves a check, rewords a message or plans another byte shows here.

Not reachable without a device, and left to the GPU tests (test_hip_*beam*.py, test_hip_rescore.py):
  - everything behind the language-model check of the four *_lm entry points (lm_w, len_bonus; in masr_recog_beam_ctc_lm and
    masr_recog_beam_lm also K, N, the pointers, B and ilens): an LM object cannot be created without a device, and a null LM is refused
    first;
  - B = 0 and ilens out of range in masr_recog_ctc_beam: they are vetted behind `not bound` (the shared front half);
  - ilens out of range and the valid call in masr_rescore_nbest: it copies the caller's lists from the device before it gets there;
  - everything behind `null language model` in the *_nlm entry points and queries (an LSTM LM cannot be created without a device either) and
    behind `null phrase list` in the *_bias entry points (nor can a phrase list);
  - ilens out of range in masr_recog_ctc_align (behind `not bound`), and a bound model in the two masr_test_*_logits."""
import ctypes as C

import pytest

import masr_amd  # noqa: F401
from masr_amd import _cabi

NAN, INF = float("nan"), float("inf")
SHAPES = ((1, 8), (2, 40), (16, 1000))
KS = (1, 4, 20)
MAXLS = (0, 5, 1023)
# name -> which of (B, T, K, N, Lmax, M = maxL) it takes; 0: an LSTM LM, always null here (only the refusal is recorded)
WS_FNS = {"masr_workspace_bytes": "BTL", "masr_beam_workspace_bytes": "BTKL", "masr_beam_lm_workspace_bytes": "BTKL",
          "masr_beam_ctc_workspace_bytes": "BTKL", "masr_beam_ctc_lm_workspace_bytes": "BTKNL", "masr_ctc_beam_workspace_bytes": "BTK",
          "masr_rescore_workspace_bytes": "BTKNL", "masr_beam_bias_workspace_bytes": "BTKL", "masr_beam_ctc_bias_workspace_bytes": "BTKNL",
          "masr_ctc_align_workspace_bytes": "BTM", "masr_beam_nlm_workspace_bytes": "0BTKL", "masr_beam_ctc_nlm_workspace_bytes": "0BTKNL",
          "masr_ctc_beam_nlm_workspace_bytes": "0BTK", "masr_rescore_nlm_workspace_bytes": "0BTKNL"}


@pytest.fixture(scope="module")
def models():
    l = _cabi.lib()
    cfg = _cabi.MasrConfig(80, 367, 512, 8, 2048, 2, 4, 1, 0.1, 0.1, 0.0)
    m = {"plain": l.masr_create(C.byref(cfg)), "hybrid": l.masr_create_ctc(C.byref(cfg), 0.3)}
    assert m["plain"] and m["hybrid"]
    yield m
    for h in m.values():
        l.masr_destroy(h)


def _ws(models, tag, fn, **v):
    """the query `fn` with the arguments it takes out of B, T, K, N, L, M -> (bytes, None) or (-1, the recorded error)"""
    l = _cabi.lib()
    n = int(getattr(l, fn)(models[tag], *[None if c == "0" else v[c] for c in WS_FNS[fn]]))
    return (n, None) if n >= 0 else (n, l.masr_last_error().decode())


def ws_cases():
    for fn, sig in WS_FNS.items():
        if "0" in sig:
            continue
        for B, T in SHAPES:
            for K in KS if "K" in sig else (0,):
                for N in sorted({1, K}) if "N" in sig else (0,):
                    for M in MAXLS if "M" in sig else (0,):
                        yield fn, dict(B=B, T=T, K=K, N=N, L=T // 4, M=M)


def refusal_cases():
    ok = dict(B=2, T=40, K=4, N=1, L=10, M=5)
    for fn, sig in WS_FNS.items():
        if "0" in sig:                                         # (the null LM is refused in front of everything else)
            yield fn, "null LM", ok
            yield fn, "null LM + K=65", dict(ok, K=65)
            continue
        if "K" in sig:
            yield fn, "K=65", dict(ok, K=65)
        if "N" in sig:
            yield fn, "N>K", dict(ok, N=5)
        if "M" in sig:
            yield fn, "maxL=1024", dict(ok, M=1024)
            yield fn, "maxL=-1", dict(ok, M=-1)
        if fn != "masr_workspace_bytes":                       # (the training workspace query vets nothing: it is not a decoder's)
            yield fn, "T=3", dict(ok, T=3)
            yield fn, "B=0", dict(ok, B=0)


def _key(fn, v):
    return f"{fn}({', '.join(f'{c}={v[c]}' for c in WS_FNS[fn] if c != '0')})"


def measure_ws(models):
    return {tag: {_key(fn, v): _ws(models, tag, fn, **v)[0] for fn, v in ws_cases()} for tag in ("plain", "hybrid")}


def measure_refusals(models):
    return {f"{fn} {what}": _ws(models, "hybrid", fn, **v) for fn, what, v in refusal_cases()}


# ---------------------------------------------------------------- entry points
class Call:
    """one entry point with valid arguments; a case overrides some of them by name"""
    _buf = (C.c_int64 * 64)()                                   # stands in for every device pointer: never read on the host
    P = C.addressof(_buf)

    def __init__(self, fn, order, **defaults):
        self.fn, self.order = fn, order.split()
        self.defaults = dict(dict(m="hybrid", xs=self.P, il=(40, 36), B=2, T=40, K=4, N=2, r0=0.0, r1=1.0, att_w=0.5, ctc_w=0.5, lm_w=0.3, bonus=0.0,
                                  lm=None, tok=self.P, lens=self.P, sc=self.P, am=self.P, att=self.P, ctc=self.P, order=self.P, tok_in=self.P,
                                  ld=10, lens_in=self.P, ctc_in=self.P, stream=None,
                                  bias=None, bias_w=1.0, nbias=self.P,                                          # phrase biasing
                                  ys=self.P, ol=(3, 2), maxL=5, frames=self.P, start=self.P, end=self.P, score=self.P,   # alignment
                                  lg=self.P, ld64=384, enc=self.P, Tp=10, C=367, blank=0, eos=366, work=self.P, wb=1 << 20,   # the bare searches
                                  out0=C.byref(C.c_void_p()), out1=C.byref(C.c_int64()), out2=C.byref(C.c_void_p())), **defaults)

    def __call__(self, models, **over):
        v = dict(self.defaults, **over)
        v["m"] = models[v["m"]] if v["m"] else None
        keep = []                                               # ilens and olens are read on the host
        for k in ("il", "ol"):
            if v[k] is not None:
                keep.append((C.c_int64 * len(v[k]))(*v[k]))
                v[k] = C.addressof(keep[-1])
        l = _cabi.lib()
        rc = getattr(l, self.fn)(*[v[k] for k in self.order])
        return rc, l.masr_last_error().decode()


CALLS = {c.fn: c for c in (
    Call("masr_recog_beam", "m xs il B T K r0 r1 tok lens sc stream"),
    Call("masr_recog_beam_ctc", "m xs il B T K r0 r1 att_w ctc_w tok lens sc stream"),
    Call("masr_recog_beam_lm", "m lm xs il B T K r0 r1 lm_w tok lens sc stream"),
    Call("masr_recog_beam_ctc_lm", "m lm xs il B T K N r0 r1 att_w ctc_w lm_w bonus tok lens sc stream"),
    Call("masr_recog_ctc_beam", "m xs il B T K N tok lens sc stream"),
    Call("masr_recog_ctc_beam_lm", "m lm xs il B T K N lm_w bonus tok lens sc am stream"),
    Call("masr_recog_rescore", "m xs il B T K N att_w ctc_w tok lens sc att ctc order stream"),
    Call("masr_recog_rescore_lm", "m lm xs il B T K N lm_w bonus att_w ctc_w tok lens sc att ctc order stream"),
    Call("masr_rescore_nbest", "m xs il B T N tok_in ld lens_in ctc_in att_w ctc_w tok lens sc att ctc order stream"),
    # phrase biasing (lm may be null there: the list is what is vetted) and the LSTM LM (`lm` is the masr_nlm)
    Call("masr_recog_beam_bias", "m lm bias xs il B T K r0 r1 lm_w bias_w tok lens sc nbias stream"),
    Call("masr_recog_beam_ctc_bias", "m lm bias xs il B T K N r0 r1 att_w ctc_w lm_w bonus bias_w tok lens sc nbias stream"),
    Call("masr_recog_ctc_beam_bias", "m lm bias xs il B T K N lm_w bonus bias_w tok lens sc am nbias stream"),
    Call("masr_recog_rescore_bias", "m lm bias xs il B T K N lm_w bonus bias_w att_w ctc_w tok lens sc att ctc order stream"),
    Call("masr_recog_beam_nlm", "m lm xs il B T K r0 r1 lm_w tok lens sc stream"),
    Call("masr_recog_beam_ctc_nlm", "m lm xs il B T K N r0 r1 att_w ctc_w lm_w bonus tok lens sc stream"),
    Call("masr_recog_ctc_beam_nlm", "m lm xs il B T K N lm_w bonus tok lens sc am stream"),
    Call("masr_recog_rescore_nlm", "m lm xs il B T K N lm_w bonus att_w ctc_w tok lens sc att ctc order stream"),
    Call("masr_recog_ctc_align", "m xs il B T ys ol maxL frames start end score stream"),
    # listed cases only (BARE): the searches on caller-given logits, and where the last plan put the head's logits
    Call("masr_ctc_beam_search_bias", "lg ld64 enc B Tp C K N blank eos lm lm_w bonus bias bias_w work wb tok lens sc am nbias stream"),
    Call("masr_ctc_beam_search_nlm", "lg ld64 enc B Tp C K N blank eos lm lm_w bonus work wb tok lens sc am stream"),
    Call("masr_test_ctc_beam_logits", "m B T K out0 out1 out2"),
    Call("masr_test_ctc_align_logits", "m B T maxL out0 out1 out2"),
)}
WEIGHT_FAULTS = [(w, v) for w in ("att_w", "ctc_w") for v in (0.0, -0.5, NAN, INF)]
BARE = ("masr_ctc_beam_search_bias", "masr_ctc_beam_search_nlm", "masr_test_ctc_beam_logits", "masr_test_ctc_align_logits")
NEEDS_HEAD = [fn for fn in CALLS if fn not in BARE + ("masr_recog_beam", "masr_recog_beam_lm", "masr_recog_beam_bias", "masr_recog_beam_nlm")]


def fault_cases():
    """(entry point, label, overrides): every listed fault where the entry point has the argument, then the two-fault calls"""
    for fn, call in CALLS.items():
        if fn in BARE:
            continue
        has = set(call.order)
        yield fn, "null model", dict(m=None)
        if fn in NEEDS_HEAD:
            yield fn, "no CTC head", dict(m="plain")
        if "K" in has:
            yield fn, "K=0", dict(K=0)
            yield fn, "K=65", dict(K=65)
            yield fn, "N=0", dict(N=0) if "N" in has else None
            yield fn, "N>K", dict(N=5) if "N" in has else None
        elif "N" in has:                                           # masr_rescore_nbest: N in [1, 64], no K
            yield fn, "N=0", dict(N=0)
            yield fn, "N=65", dict(N=65)
        for w, v in WEIGHT_FAULTS:
            if w in has:
                yield fn, f"{w}={v}", {w: v}
        if "lm_w" in has:
            for v in (-0.5, NAN, INF):
                yield fn, f"lm_w={v}", dict(lm_w=v)
        if "bonus" in has:
            yield fn, "len_bonus=nan", dict(bonus=NAN)
        if "lm" in has:
            yield fn, "null LM", dict(lm=None)
        if "bias" in has:
            yield fn, "null list", dict(bias=None)
        if "maxL" in has:
            for v in (-1, 0, 1023, 1024):                          # 2 * maxL + 1 <= 2048
                yield fn, f"maxL={v}", dict(maxL=v)
        for p in ("xs", "il", "tok", "lens", "sc", "am", "att", "ctc", "order", "lens_in", "ctc_in", "tok_in", "nbias", "ys", "ol", "frames", "start",
                  "end", "score"):
            if p in has:
                yield fn, f"null {p}", {p: None}
        yield fn, "B=0", dict(B=0)
        yield fn, "T=3", dict(T=3)
        yield fn, "ilens<4", dict(il=(40, 3))
        yield fn, "ilens>T", dict(il=(41, 36))
        yield fn, "valid", {}
    # order of checks: two faults at once, the earlier check answers
    yield "masr_recog_beam", "K=0 + null xs", dict(K=0, xs=None)
    yield "masr_recog_beam", "null sc + B=0", dict(sc=None, B=0)
    yield "masr_recog_beam", "B=0 + ilens<4", dict(B=0, il=(3, 3))
    yield "masr_recog_beam_ctc", "no CTC head + ctc_w=0", dict(m="plain", ctc_w=0.0)
    yield "masr_recog_beam_ctc", "ctc_w=0 + att_w=-1", dict(ctc_w=0.0, att_w=-1.0)
    yield "masr_recog_beam_ctc", "att_w=nan + K=0", dict(att_w=NAN, K=0)
    yield "masr_recog_beam_lm", "null model + null LM", dict(m=None, lm=None)
    yield "masr_recog_beam_lm", "null LM + lm_w=-1 + K=0", dict(lm=None, lm_w=-1.0, K=0)
    yield "masr_recog_beam_ctc_lm", "ctc_w=0 + null LM", dict(ctc_w=0.0, lm=None)
    yield "masr_recog_beam_ctc_lm", "att_w=inf + null LM", dict(att_w=INF, lm=None)
    yield "masr_recog_beam_ctc_lm", "null LM + K=0 + N=0", dict(lm=None, K=0, N=0)
    yield "masr_recog_ctc_beam", "K=65 + N=0", dict(K=65, N=0)
    yield "masr_recog_ctc_beam", "N=5 + null tok", dict(N=5, tok=None)
    yield "masr_recog_ctc_beam_lm", "N=0 + null LM", dict(N=0, lm=None)
    yield "masr_recog_ctc_beam_lm", "null LM + null am", dict(lm=None, am=None)
    yield "masr_recog_rescore", "N=5 + att_w=0", dict(N=5, att_w=0.0)
    yield "masr_recog_rescore", "att_w=0 + ctc_w=-1", dict(att_w=0.0, ctc_w=-1.0)
    yield "masr_recog_rescore", "ctc_w=nan + null order", dict(ctc_w=NAN, order=None)
    yield "masr_recog_rescore", "null att + B=0", dict(att=None, B=0)
    yield "masr_recog_rescore", "T=3 + ilens<4", dict(T=3, il=(3, 3))
    yield "masr_recog_rescore_lm", "ctc_w=-1 + null LM", dict(ctc_w=-1.0, lm=None)
    yield "masr_recog_rescore_lm", "K=0 + null LM", dict(K=0, lm=None)
    yield "masr_rescore_nbest", "N=65 + att_w=0", dict(N=65, att_w=0.0)
    yield "masr_rescore_nbest", "ctc_w=inf + null lens_in", dict(ctc_w=INF, lens_in=None)
    yield "masr_rescore_nbest", "null ctc_in + ld=3000", dict(ctc_in=None, ld=3000)
    yield "masr_rescore_nbest", "ld=-1", dict(ld=-1)
    yield "masr_rescore_nbest", "ld=3000", dict(ld=3000)
    yield "masr_rescore_nbest", "ld=0 + null tok_in + B=0", dict(ld=0, tok_in=None, B=0)
    yield "masr_recog_beam_bias", "null model + null list", dict(m=None, bias=None)
    yield "masr_recog_beam_bias", "null list + bias_w=-1 + K=0", dict(bias=None, bias_w=-1.0, K=0)
    yield "masr_recog_beam_bias", "null list + null nbias", dict(bias=None, nbias=None)
    yield "masr_recog_beam_ctc_bias", "no CTC head + ctc_w=0", dict(m="plain", ctc_w=0.0)
    yield "masr_recog_beam_ctc_bias", "ctc_w=0 + att_w=-1", dict(ctc_w=0.0, att_w=-1.0)
    yield "masr_recog_beam_ctc_bias", "att_w=inf + len_bonus=nan", dict(att_w=INF, bonus=NAN)
    yield "masr_recog_beam_ctc_bias", "len_bonus=nan + null list", dict(bonus=NAN, bias=None)
    yield "masr_recog_beam_ctc_bias", "null list + K=0 + N=0", dict(bias=None, K=0, N=0)
    yield "masr_recog_ctc_beam_bias", "K=65 + N=0", dict(K=65, N=0)
    yield "masr_recog_ctc_beam_bias", "N=0 + null list", dict(N=0, bias=None)
    yield "masr_recog_ctc_beam_bias", "null list + len_bonus=nan + null am", dict(bias=None, bonus=NAN, am=None)
    yield "masr_recog_rescore_bias", "N=5 + att_w=0", dict(N=5, att_w=0.0)
    yield "masr_recog_rescore_bias", "ctc_w=-1 + null list", dict(ctc_w=-1.0, bias=None)
    yield "masr_recog_rescore_bias", "null list + null order", dict(bias=None, order=None)
    yield "masr_recog_beam_nlm", "null model + null LM", dict(m=None, lm=None)
    yield "masr_recog_beam_nlm", "null LM + lm_w=-1 + K=0", dict(lm=None, lm_w=-1.0, K=0)
    yield "masr_recog_beam_ctc_nlm", "ctc_w=0 + null LM", dict(ctc_w=0.0, lm=None)
    yield "masr_recog_beam_ctc_nlm", "att_w=inf + null LM", dict(att_w=INF, lm=None)
    yield "masr_recog_beam_ctc_nlm", "null LM + K=0 + N=0", dict(lm=None, K=0, N=0)
    yield "masr_recog_ctc_beam_nlm", "null LM + no CTC head", dict(lm=None, m="plain")
    yield "masr_recog_ctc_beam_nlm", "null LM + K=0", dict(lm=None, K=0)
    yield "masr_recog_rescore_nlm", "null LM + no CTC head", dict(lm=None, m="plain")
    yield "masr_recog_rescore_nlm", "null LM + att_w=0", dict(lm=None, att_w=0.0)
    yield "masr_recog_ctc_align", "no CTC head + null xs", dict(m="plain", xs=None)
    yield "masr_recog_ctc_align", "null score + maxL=1024", dict(score=None, maxL=1024)
    yield "masr_recog_ctc_align", "maxL=1024 + null ys", dict(maxL=1024, ys=None)
    yield "masr_recog_ctc_align", "B=0 + T=3", dict(B=0, T=3)
    yield "masr_recog_ctc_align", "null ys + no token in range", dict(ys=None, ol=(0, 9))
    yield "masr_recog_ctc_align", "null ys + ilens<4", dict(ys=None, il=(40, 3))
    yield "masr_ctc_beam_search_bias", "null list", dict(bias=None)
    yield "masr_ctc_beam_search_bias", "null list + K=0 + null lg", dict(bias=None, K=0, lg=None)
    yield "masr_ctc_beam_search_nlm", "null LM", dict(lm=None)
    yield "masr_ctc_beam_search_nlm", "null LM + K=0 + null lg", dict(lm=None, K=0, lg=None)
    for fn in ("masr_test_ctc_beam_logits", "masr_test_ctc_align_logits"):
        yield fn, "null model", dict(m=None)
        yield fn, "not bound", {}
        yield fn, "not bound + no CTC head", dict(m="plain")
        yield fn, "not bound + B=0", dict(B=0)
        yield fn, "null out + not bound", dict(out1=None)


# what a case of fault_cases() cannot reach on an unbound model without an LM (the docstring's list): left out, not asserted
def _unreachable(fn, label, over):
    if over is None:
        return True
    if fn.endswith(("_lm", "_nlm", "_bias")) and label != ("null list" if fn.endswith("_bias") else "null LM") and "+" not in label:
        # only what is vetted in front of the LM check (the list's, in *_bias) can answer; everything else would only repeat `null language
        # model` (`null phrase list`)
        front = {"masr_recog_beam_lm": ("null model",),
                 "masr_recog_beam_ctc_lm": ("null model", "no CTC head", "att_w", "ctc_w"),
                 "masr_recog_ctc_beam_lm": ("null model", "no CTC head", "K=", "N="),
                 "masr_recog_rescore_lm": ("null model", "no CTC head", "K=", "N=", "att_w", "ctc_w"),
                 "masr_recog_beam_nlm": ("null model",),
                 "masr_recog_beam_ctc_nlm": ("null model", "no CTC head", "att_w", "ctc_w"),
                 "masr_recog_ctc_beam_nlm": ("null model",),
                 "masr_recog_rescore_nlm": ("null model",),
                 "masr_recog_beam_bias": ("null model",),
                 "masr_recog_beam_ctc_bias": ("null model", "no CTC head", "att_w", "ctc_w", "len_bonus"),
                 "masr_recog_ctc_beam_bias": ("null model", "no CTC head", "K=", "N="),
                 "masr_recog_rescore_bias": ("null model", "no CTC head", "K=", "N=", "att_w", "ctc_w")}[fn]
        return not label.startswith(front)
    if fn in ("masr_recog_ctc_beam", "masr_recog_ctc_align") and label in ("ilens<4", "ilens>T"):
        return True
    if fn == "masr_recog_ctc_beam" and label in ("B=0", "T=3"):
        return True
    if fn == "masr_rescore_nbest" and label in ("ilens<4", "ilens>T", "valid", "ctc_w=0.0"):      # (ctc_w = 0 is valid there)
        return True
    return False


def measure_faults(models):
    return {f"{fn}: {label}": CALLS[fn](models, **over) for fn, label, over in fault_cases() if not _unreachable(fn, label, over)}


# ---------------------------------------------------------------- the recorded answers
WS_BYTES = {'hybrid': {'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': 100711168,
            'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': 105632256,
            'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': 105632256,
            'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': 101476608,
            'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': 101476608,
            'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': 1167079936,
            'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': 10769545728,
            'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': 10769548800,
            'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': 2677736960,
            'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': 2677736960,
            'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': 105518336,
            'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': 154026240,
            'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': 154026240,
            'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': 113148928,
            'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': 113148928,
            'masr_beam_ctc_workspace_bytes(B=1, T=8, K=1, L=2)': 100708352,
            'masr_beam_ctc_workspace_bytes(B=1, T=8, K=20, L=2)': 105597952,
            'masr_beam_ctc_workspace_bytes(B=1, T=8, K=4, L=2)': 101469184,
            'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=1, L=250)': 1167054080,
            'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=20, L=250)': 10769014784,
            'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=4, L=250)': 2677636096,
            'masr_beam_ctc_workspace_bytes(B=2, T=40, K=1, L=10)': 105513984,
            'masr_beam_ctc_workspace_bytes(B=2, T=40, K=20, L=10)': 153958912,
            'masr_beam_ctc_workspace_bytes(B=2, T=40, K=4, L=10)': 113135360,
            'masr_beam_lm_workspace_bytes(B=1, T=8, K=1, L=2)': 100701952,
            'masr_beam_lm_workspace_bytes(B=1, T=8, K=20, L=2)': 105591040,
            'masr_beam_lm_workspace_bytes(B=1, T=8, K=4, L=2)': 101466880,
            'masr_beam_lm_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154996992,
            'masr_beam_lm_workspace_bytes(B=16, T=1000, K=20, L=250)': 10718908416,
            'masr_beam_lm_workspace_bytes(B=16, T=1000, K=4, L=250)': 2664174592,
            'masr_beam_lm_workspace_bytes(B=2, T=40, K=1, L=10)': 105454848,
            'masr_beam_lm_workspace_bytes(B=2, T=40, K=20, L=10)': 153745152,
            'masr_beam_lm_workspace_bytes(B=2, T=40, K=4, L=10)': 113078272,
            'masr_beam_workspace_bytes(B=1, T=8, K=1, L=2)': 100700416,
            'masr_beam_workspace_bytes(B=1, T=8, K=20, L=2)': 105560320,
            'masr_beam_workspace_bytes(B=1, T=8, K=4, L=2)': 101460736,
            'masr_beam_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154972416,
            'masr_beam_workspace_bytes(B=16, T=1000, K=20, L=250)': 10718416896,
            'masr_beam_workspace_bytes(B=16, T=1000, K=4, L=250)': 2664076288,
            'masr_beam_workspace_bytes(B=2, T=40, K=1, L=10)': 105451776,
            'masr_beam_workspace_bytes(B=2, T=40, K=20, L=10)': 153683712,
            'masr_beam_workspace_bytes(B=2, T=40, K=4, L=10)': 113065984,
            'masr_ctc_beam_workspace_bytes(B=1, T=8, K=1)': 100573440,
            'masr_ctc_beam_workspace_bytes(B=1, T=8, K=20)': 100573440,
            'masr_ctc_beam_workspace_bytes(B=1, T=8, K=4)': 100573440,
            'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=1)': 660836352,
            'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=20)': 661747968,
            'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=4)': 660979968,
            'masr_ctc_beam_workspace_bytes(B=2, T=40, K=1)': 103217408,
            'masr_ctc_beam_workspace_bytes(B=2, T=40, K=20)': 103222016,
            'masr_ctc_beam_workspace_bytes(B=2, T=40, K=4)': 103218176,
            'masr_rescore_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': 100825344,
            'masr_rescore_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': 100825344,
            'masr_rescore_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': 108028928,
            'masr_rescore_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': 100825344,
            'masr_rescore_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': 101958144,
            'masr_rescore_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': 1163121664,
            'masr_rescore_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': 1164033280,
            'masr_rescore_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': 10764143872,
            'masr_rescore_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': 1163265280,
            'masr_rescore_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': 2678169856,
            'masr_rescore_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': 105730560,
            'masr_rescore_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': 105735168,
            'masr_rescore_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': 158645760,
            'masr_rescore_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': 105731328,
            'masr_rescore_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': 114084096,
            'masr_workspace_bytes(B=1, T=8, L=2)': 219722240,
            'masr_workspace_bytes(B=16, T=1000, L=250)': 1820787456,
            'masr_workspace_bytes(B=2, T=40, L=10)': 227050240,
            'masr_beam_bias_workspace_bytes(B=1, T=8, K=1, L=2)': 100702208,
            'masr_beam_bias_workspace_bytes(B=1, T=8, K=20, L=2)': 105591552,
            'masr_beam_bias_workspace_bytes(B=1, T=8, K=4, L=2)': 101467136,
            'masr_beam_bias_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154997248,
            'masr_beam_bias_workspace_bytes(B=16, T=1000, K=20, L=250)': 10718913536,
            'masr_beam_bias_workspace_bytes(B=16, T=1000, K=4, L=250)': 2664175616,
            'masr_beam_bias_workspace_bytes(B=2, T=40, K=1, L=10)': 105455104,
            'masr_beam_bias_workspace_bytes(B=2, T=40, K=20, L=10)': 153745920,
            'masr_beam_bias_workspace_bytes(B=2, T=40, K=4, L=10)': 113078528,
            'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': 100711680,
            'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': 105635328,
            'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': 105635328,
            'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': 101477120,
            'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': 101477120,
            'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': 1167080448,
            'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': 10769589248,
            'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': 10769592320,
            'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': 2677739520,
            'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': 2677739520,
            'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': 105518848,
            'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': 154031872,
            'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': 154031872,
            'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': 113149440,
            'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': 113149440,
            'masr_ctc_align_workspace_bytes(B=1, T=8, M=0)': 100573184,
            'masr_ctc_align_workspace_bytes(B=1, T=8, M=1023)': 100589056,
            'masr_ctc_align_workspace_bytes(B=1, T=8, M=5)': 100573184,
            'masr_ctc_align_workspace_bytes(B=16, T=1000, M=0)': 660792320,
            'masr_ctc_align_workspace_bytes(B=16, T=1000, M=1023)': 685409792,
            'masr_ctc_align_workspace_bytes(B=16, T=1000, M=5)': 660912384,
            'masr_ctc_align_workspace_bytes(B=2, T=40, M=0)': 103217152,
            'masr_ctc_align_workspace_bytes(B=2, T=40, M=1023)': 103347712,
            'masr_ctc_align_workspace_bytes(B=2, T=40, M=5)': 103217408},
 'plain': {'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': -1,
           'masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': -1,
           'masr_beam_ctc_workspace_bytes(B=1, T=8, K=1, L=2)': -1,
           'masr_beam_ctc_workspace_bytes(B=1, T=8, K=20, L=2)': -1,
           'masr_beam_ctc_workspace_bytes(B=1, T=8, K=4, L=2)': -1,
           'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=1, L=250)': -1,
           'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=20, L=250)': -1,
           'masr_beam_ctc_workspace_bytes(B=16, T=1000, K=4, L=250)': -1,
           'masr_beam_ctc_workspace_bytes(B=2, T=40, K=1, L=10)': -1,
           'masr_beam_ctc_workspace_bytes(B=2, T=40, K=20, L=10)': -1,
           'masr_beam_ctc_workspace_bytes(B=2, T=40, K=4, L=10)': -1,
           'masr_beam_lm_workspace_bytes(B=1, T=8, K=1, L=2)': 99915264,
           'masr_beam_lm_workspace_bytes(B=1, T=8, K=20, L=2)': 104804608,
           'masr_beam_lm_workspace_bytes(B=1, T=8, K=4, L=2)': 100680448,
           'masr_beam_lm_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154210304,
           'masr_beam_lm_workspace_bytes(B=16, T=1000, K=20, L=250)': 10718121984,
           'masr_beam_lm_workspace_bytes(B=16, T=1000, K=4, L=250)': 2663388160,
           'masr_beam_lm_workspace_bytes(B=2, T=40, K=1, L=10)': 104668416,
           'masr_beam_lm_workspace_bytes(B=2, T=40, K=20, L=10)': 152958720,
           'masr_beam_lm_workspace_bytes(B=2, T=40, K=4, L=10)': 112291840,
           'masr_beam_workspace_bytes(B=1, T=8, K=1, L=2)': 99913728,
           'masr_beam_workspace_bytes(B=1, T=8, K=20, L=2)': 104773888,
           'masr_beam_workspace_bytes(B=1, T=8, K=4, L=2)': 100674304,
           'masr_beam_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154185728,
           'masr_beam_workspace_bytes(B=16, T=1000, K=20, L=250)': 10717630464,
           'masr_beam_workspace_bytes(B=16, T=1000, K=4, L=250)': 2663289856,
           'masr_beam_workspace_bytes(B=2, T=40, K=1, L=10)': 104665344,
           'masr_beam_workspace_bytes(B=2, T=40, K=20, L=10)': 152897280,
           'masr_beam_workspace_bytes(B=2, T=40, K=4, L=10)': 112279552,
           'masr_ctc_beam_workspace_bytes(B=1, T=8, K=1)': -1,
           'masr_ctc_beam_workspace_bytes(B=1, T=8, K=20)': -1,
           'masr_ctc_beam_workspace_bytes(B=1, T=8, K=4)': -1,
           'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=1)': -1,
           'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=20)': -1,
           'masr_ctc_beam_workspace_bytes(B=16, T=1000, K=4)': -1,
           'masr_ctc_beam_workspace_bytes(B=2, T=40, K=1)': -1,
           'masr_ctc_beam_workspace_bytes(B=2, T=40, K=20)': -1,
           'masr_ctc_beam_workspace_bytes(B=2, T=40, K=4)': -1,
           'masr_rescore_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': -1,
           'masr_rescore_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': -1,
           'masr_rescore_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': -1,
           'masr_rescore_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': -1,
           'masr_rescore_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': -1,
           'masr_rescore_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': -1,
           'masr_rescore_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': -1,
           'masr_rescore_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': -1,
           'masr_rescore_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': -1,
           'masr_rescore_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': -1,
           'masr_rescore_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': -1,
           'masr_rescore_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': -1,
           'masr_rescore_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': -1,
           'masr_rescore_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': -1,
           'masr_rescore_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': -1,
           'masr_workspace_bytes(B=1, T=8, L=2)': 218930432,
           'masr_workspace_bytes(B=16, T=1000, L=250)': 1794752256,
           'masr_workspace_bytes(B=2, T=40, L=10)': 226213888,
           'masr_beam_bias_workspace_bytes(B=1, T=8, K=1, L=2)': 99915520,
           'masr_beam_bias_workspace_bytes(B=1, T=8, K=20, L=2)': 104805120,
           'masr_beam_bias_workspace_bytes(B=1, T=8, K=4, L=2)': 100680704,
           'masr_beam_bias_workspace_bytes(B=16, T=1000, K=1, L=250)': 1154210560,
           'masr_beam_bias_workspace_bytes(B=16, T=1000, K=20, L=250)': 10718127104,
           'masr_beam_bias_workspace_bytes(B=16, T=1000, K=4, L=250)': 2663389184,
           'masr_beam_bias_workspace_bytes(B=2, T=40, K=1, L=10)': 104668672,
           'masr_beam_bias_workspace_bytes(B=2, T=40, K=20, L=10)': 152959488,
           'masr_beam_bias_workspace_bytes(B=2, T=40, K=4, L=10)': 112292096,
           'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=1, N=1, L=2)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=20, N=1, L=2)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=20, N=20, L=2)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=4, N=1, L=2)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=1, T=8, K=4, N=4, L=2)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=1, N=1, L=250)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=20, N=1, L=250)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=20, N=20, L=250)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=4, N=1, L=250)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=16, T=1000, K=4, N=4, L=250)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=1, N=1, L=10)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=20, N=1, L=10)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=20, N=20, L=10)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=4, N=1, L=10)': -1,
           'masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=4, N=4, L=10)': -1,
           'masr_ctc_align_workspace_bytes(B=1, T=8, M=0)': -1,
           'masr_ctc_align_workspace_bytes(B=1, T=8, M=1023)': -1,
           'masr_ctc_align_workspace_bytes(B=1, T=8, M=5)': -1,
           'masr_ctc_align_workspace_bytes(B=16, T=1000, M=0)': -1,
           'masr_ctc_align_workspace_bytes(B=16, T=1000, M=1023)': -1,
           'masr_ctc_align_workspace_bytes(B=16, T=1000, M=5)': -1,
           'masr_ctc_align_workspace_bytes(B=2, T=40, M=0)': -1,
           'masr_ctc_align_workspace_bytes(B=2, T=40, M=1023)': -1,
           'masr_ctc_align_workspace_bytes(B=2, T=40, M=5)': -1}}
WS_REFUSALS = {'masr_beam_ctc_lm_workspace_bytes B=0': (-1, 'masr_beam_ctc_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_lm_workspace_bytes K=65': (-1, 'masr_beam_ctc_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_lm_workspace_bytes N>K': (-1, 'masr_beam_ctc_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_lm_workspace_bytes T=3': (-1, 'masr_beam_ctc_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_workspace_bytes B=0': (-1, 'masr_beam_ctc_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_workspace_bytes K=65': (-1, 'masr_beam_ctc_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_workspace_bytes T=3': (-1, 'masr_beam_ctc_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_lm_workspace_bytes B=0': (-1, 'masr_beam_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_lm_workspace_bytes K=65': (-1, 'masr_beam_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_lm_workspace_bytes T=3': (-1, 'masr_beam_lm_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_workspace_bytes B=0': (-1, 'masr_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_workspace_bytes K=65': (-1, 'masr_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_workspace_bytes T=3': (-1, 'masr_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_ctc_beam_workspace_bytes B=0': (-1, 'masr_ctc_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64'),
 'masr_ctc_beam_workspace_bytes K=65': (-1, 'masr_ctc_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64'),
 'masr_ctc_beam_workspace_bytes T=3': (-1, 'masr_ctc_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64'),
 'masr_rescore_workspace_bytes B=0': (-1, 'masr_rescore_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, 0 <= Lmax < 3000'),
 'masr_rescore_workspace_bytes K=65': (-1, 'masr_rescore_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, 0 <= Lmax < 3000'),
 'masr_rescore_workspace_bytes N>K': (-1, 'masr_rescore_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, 0 <= Lmax < 3000'),
 'masr_rescore_workspace_bytes T=3': (-1, 'masr_rescore_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, 0 <= Lmax < 3000'),
 'masr_beam_bias_workspace_bytes B=0': (-1, 'masr_beam_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_bias_workspace_bytes K=65': (-1, 'masr_beam_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_bias_workspace_bytes T=3': (-1, 'masr_beam_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_bias_workspace_bytes B=0': (-1, 'masr_beam_ctc_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_bias_workspace_bytes K=65': (-1, 'masr_beam_ctc_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_bias_workspace_bytes N>K': (-1, 'masr_beam_ctc_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_bias_workspace_bytes T=3': (-1, 'masr_beam_ctc_bias_workspace_bytes: need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1'),
 'masr_beam_ctc_nlm_workspace_bytes null LM': (-1, 'masr_beam_ctc_nlm_workspace_bytes: null language model'),
 'masr_beam_ctc_nlm_workspace_bytes null LM + K=65': (-1, 'masr_beam_ctc_nlm_workspace_bytes: null language model'),
 'masr_beam_nlm_workspace_bytes null LM': (-1, 'masr_beam_nlm_workspace_bytes: null language model'),
 'masr_beam_nlm_workspace_bytes null LM + K=65': (-1, 'masr_beam_nlm_workspace_bytes: null language model'),
 'masr_ctc_align_workspace_bytes B=0': (-1, 'masr_ctc_align_workspace_bytes: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_ctc_align_workspace_bytes T=3': (-1, 'masr_ctc_align_workspace_bytes: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_ctc_align_workspace_bytes maxL=-1': (-1, 'masr_ctc_align_workspace_bytes: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_ctc_align_workspace_bytes maxL=1024': (-1, 'masr_ctc_align_workspace_bytes: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_ctc_beam_nlm_workspace_bytes null LM': (-1, 'masr_ctc_beam_nlm_workspace_bytes: null language model'),
 'masr_ctc_beam_nlm_workspace_bytes null LM + K=65': (-1, 'masr_ctc_beam_nlm_workspace_bytes: null language model'),
 'masr_rescore_nlm_workspace_bytes null LM': (-1, 'masr_rescore_nlm_workspace_bytes: null language model'),
 'masr_rescore_nlm_workspace_bytes null LM + K=65': (-1, 'masr_rescore_nlm_workspace_bytes: null language model')}
FAULTS = {'masr_recog_beam: B=0': (-1, 'masr_recog_beam: need B >= 1'),
 'masr_recog_beam: B=0 + ilens<4': (-1, 'masr_recog_beam: need B >= 1'),
 'masr_recog_beam: K=0': (-1, 'masr_recog_beam: beam size K must be in [1, 64]'),
 'masr_recog_beam: K=0 + null xs': (-1, 'masr_recog_beam: beam size K must be in [1, 64]'),
 'masr_recog_beam: K=65': (-1, 'masr_recog_beam: beam size K must be in [1, 64]'),
 'masr_recog_beam: T=3': (-1, 'masr_recog_beam: ilens must be in [4, T]'),
 'masr_recog_beam: ilens<4': (-1, 'masr_recog_beam: ilens must be in [4, T]'),
 'masr_recog_beam: ilens>T': (-1, 'masr_recog_beam: ilens must be in [4, T]'),
 'masr_recog_beam: null il': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: null lens': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: null model': (-1, 'masr_recog_beam: null model'),
 'masr_recog_beam: null sc': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: null sc + B=0': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: null tok': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: null xs': (-1, 'masr_recog_beam: null pointer'),
 'masr_recog_beam: valid': (-1, 'masr_recog: not bound'),
 'masr_recog_beam_ctc: B=0': (-1, 'masr_recog_beam_ctc: need B >= 1'),
 'masr_recog_beam_ctc: K=0': (-1, 'masr_recog_beam_ctc: beam size K must be in [1, 64]'),
 'masr_recog_beam_ctc: K=65': (-1, 'masr_recog_beam_ctc: beam size K must be in [1, 64]'),
 'masr_recog_beam_ctc: T=3': (-1, 'masr_recog_beam_ctc: ilens must be in [4, T]'),
 'masr_recog_beam_ctc: att_w=-0.5': (-1, 'masr_recog_beam_ctc: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc: att_w=0.0': (-1, 'masr_recog: not bound'),
 'masr_recog_beam_ctc: att_w=inf': (-1, 'masr_recog_beam_ctc: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc: att_w=nan': (-1, 'masr_recog_beam_ctc: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc: att_w=nan + K=0': (-1, 'masr_recog_beam_ctc: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc: ctc_w=-0.5': (-1, 'masr_recog_beam_ctc: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc: ctc_w=0 + att_w=-1': (-1, 'masr_recog_beam_ctc: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc: ctc_w=0.0': (-1, 'masr_recog_beam_ctc: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc: ctc_w=inf': (-1, 'masr_recog_beam_ctc: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc: ctc_w=nan': (-1, 'masr_recog_beam_ctc: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc: ilens<4': (-1, 'masr_recog_beam_ctc: ilens must be in [4, T]'),
 'masr_recog_beam_ctc: ilens>T': (-1, 'masr_recog_beam_ctc: ilens must be in [4, T]'),
 'masr_recog_beam_ctc: no CTC head': (-1, 'masr_recog_beam_ctc: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc: no CTC head + ctc_w=0': (-1, 'masr_recog_beam_ctc: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc: null il': (-1, 'masr_recog_beam_ctc: null pointer'),
 'masr_recog_beam_ctc: null lens': (-1, 'masr_recog_beam_ctc: null pointer'),
 'masr_recog_beam_ctc: null model': (-1, 'masr_recog_beam_ctc: null model'),
 'masr_recog_beam_ctc: null sc': (-1, 'masr_recog_beam_ctc: null pointer'),
 'masr_recog_beam_ctc: null tok': (-1, 'masr_recog_beam_ctc: null pointer'),
 'masr_recog_beam_ctc: null xs': (-1, 'masr_recog_beam_ctc: null pointer'),
 'masr_recog_beam_ctc: valid': (-1, 'masr_recog: not bound'),
 'masr_recog_beam_ctc_lm: att_w=-0.5': (-1, 'masr_recog_beam_ctc_lm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_lm: att_w=0.0': (-1, 'masr_recog_beam_ctc_lm: null language model'),
 'masr_recog_beam_ctc_lm: att_w=inf': (-1, 'masr_recog_beam_ctc_lm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_lm: att_w=inf + null LM': (-1, 'masr_recog_beam_ctc_lm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_lm: att_w=nan': (-1, 'masr_recog_beam_ctc_lm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_lm: ctc_w=-0.5': (-1, 'masr_recog_beam_ctc_lm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_lm: ctc_w=0 + null LM': (-1, 'masr_recog_beam_ctc_lm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_lm: ctc_w=0.0': (-1, 'masr_recog_beam_ctc_lm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_lm: ctc_w=inf': (-1, 'masr_recog_beam_ctc_lm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_lm: ctc_w=nan': (-1, 'masr_recog_beam_ctc_lm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_lm: no CTC head': (-1, 'masr_recog_beam_ctc_lm: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc_lm: null LM': (-1, 'masr_recog_beam_ctc_lm: null language model'),
 'masr_recog_beam_ctc_lm: null LM + K=0 + N=0': (-1, 'masr_recog_beam_ctc_lm: null language model'),
 'masr_recog_beam_ctc_lm: null model': (-1, 'masr_recog_beam_ctc_lm: null model'),
 'masr_recog_beam_lm: null LM': (-1, 'masr_recog_beam_lm: null language model'),
 'masr_recog_beam_lm: null LM + lm_w=-1 + K=0': (-1, 'masr_recog_beam_lm: null language model'),
 'masr_recog_beam_lm: null model': (-1, 'masr_recog_beam_lm: null model'),
 'masr_recog_beam_lm: null model + null LM': (-1, 'masr_recog_beam_lm: null model'),
 'masr_recog_ctc_beam: K=0': (-1, 'masr_recog_ctc_beam: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam: K=65': (-1, 'masr_recog_ctc_beam: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam: K=65 + N=0': (-1, 'masr_recog_ctc_beam: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam: N=0': (-1, 'masr_recog_ctc_beam: nbest must be in [1, K]'),
 'masr_recog_ctc_beam: N=5 + null tok': (-1, 'masr_recog_ctc_beam: nbest must be in [1, K]'),
 'masr_recog_ctc_beam: N>K': (-1, 'masr_recog_ctc_beam: nbest must be in [1, K]'),
 'masr_recog_ctc_beam: no CTC head': (-1, 'masr_recog_ctc_beam: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_ctc_beam: null il': (-1, 'masr_recog_ctc_beam: null pointer'),
 'masr_recog_ctc_beam: null lens': (-1, 'masr_recog_ctc_beam: null pointer'),
 'masr_recog_ctc_beam: null model': (-1, 'masr_recog_ctc_beam: null model'),
 'masr_recog_ctc_beam: null sc': (-1, 'masr_recog_ctc_beam: null pointer'),
 'masr_recog_ctc_beam: null tok': (-1, 'masr_recog_ctc_beam: null pointer'),
 'masr_recog_ctc_beam: null xs': (-1, 'masr_recog_ctc_beam: null pointer'),
 'masr_recog_ctc_beam: valid': (-1, 'masr_recog: not bound'),
 'masr_recog_ctc_beam_lm: K=0': (-1, 'masr_recog_ctc_beam_lm: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam_lm: K=65': (-1, 'masr_recog_ctc_beam_lm: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam_lm: N=0': (-1, 'masr_recog_ctc_beam_lm: nbest must be in [1, K]'),
 'masr_recog_ctc_beam_lm: N=0 + null LM': (-1, 'masr_recog_ctc_beam_lm: nbest must be in [1, K]'),
 'masr_recog_ctc_beam_lm: no CTC head': (-1, 'masr_recog_ctc_beam_lm: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_ctc_beam_lm: null LM': (-1, 'masr_recog_ctc_beam_lm: null language model'),
 'masr_recog_ctc_beam_lm: null LM + null am': (-1, 'masr_recog_ctc_beam_lm: null language model'),
 'masr_recog_ctc_beam_lm: null model': (-1, 'masr_recog_ctc_beam_lm: null model'),
 'masr_recog_rescore: B=0': (-1, 'masr_recog_rescore: need B >= 1 and T >= 4'),
 'masr_recog_rescore: K=0': (-1, 'masr_recog_rescore: beam size K must be in [1, 64]'),
 'masr_recog_rescore: K=65': (-1, 'masr_recog_rescore: beam size K must be in [1, 64]'),
 'masr_recog_rescore: N=0': (-1, 'masr_recog_rescore: N must be in [1, K]'),
 'masr_recog_rescore: N=5 + att_w=0': (-1, 'masr_recog_rescore: N must be in [1, K]'),
 'masr_recog_rescore: N>K': (-1, 'masr_recog_rescore: N must be in [1, K]'),
 'masr_recog_rescore: T=3': (-1, 'masr_recog_rescore: need B >= 1 and T >= 4'),
 'masr_recog_rescore: T=3 + ilens<4': (-1, 'masr_recog_rescore: need B >= 1 and T >= 4'),
 'masr_recog_rescore: att_w=-0.5': (-1, 'masr_recog_rescore: att_w must be finite and > 0'),
 'masr_recog_rescore: att_w=0 + ctc_w=-1': (-1, 'masr_recog_rescore: att_w must be finite and > 0'),
 'masr_recog_rescore: att_w=0.0': (-1, 'masr_recog_rescore: att_w must be finite and > 0'),
 'masr_recog_rescore: att_w=inf': (-1, 'masr_recog_rescore: att_w must be finite and > 0'),
 'masr_recog_rescore: att_w=nan': (-1, 'masr_recog_rescore: att_w must be finite and > 0'),
 'masr_recog_rescore: ctc_w=-0.5': (-1, 'masr_recog_rescore: ctc_w must be finite and >= 0'),
 'masr_recog_rescore: ctc_w=0.0': (-1, 'masr_recog: not bound'),
 'masr_recog_rescore: ctc_w=inf': (-1, 'masr_recog_rescore: ctc_w must be finite and >= 0'),
 'masr_recog_rescore: ctc_w=nan': (-1, 'masr_recog_rescore: ctc_w must be finite and >= 0'),
 'masr_recog_rescore: ctc_w=nan + null order': (-1, 'masr_recog_rescore: ctc_w must be finite and >= 0'),
 'masr_recog_rescore: ilens<4': (-1, 'masr_recog_rescore: ilens must be in [4, T]'),
 'masr_recog_rescore: ilens>T': (-1, 'masr_recog_rescore: ilens must be in [4, T]'),
 'masr_recog_rescore: no CTC head': (-1, 'masr_recog_rescore: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_rescore: null att': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null att + B=0': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null ctc': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null il': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null lens': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null model': (-1, 'masr_recog_rescore: null model'),
 'masr_recog_rescore: null order': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null sc': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null tok': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: null xs': (-1, 'masr_recog_rescore: null pointer'),
 'masr_recog_rescore: valid': (-1, 'masr_recog: not bound'),
 'masr_recog_rescore_lm: K=0': (-1, 'masr_recog_rescore_lm: beam size K must be in [1, 64]'),
 'masr_recog_rescore_lm: K=0 + null LM': (-1, 'masr_recog_rescore_lm: beam size K must be in [1, 64]'),
 'masr_recog_rescore_lm: K=65': (-1, 'masr_recog_rescore_lm: beam size K must be in [1, 64]'),
 'masr_recog_rescore_lm: N=0': (-1, 'masr_recog_rescore_lm: N must be in [1, K]'),
 'masr_recog_rescore_lm: att_w=-0.5': (-1, 'masr_recog_rescore_lm: att_w must be finite and > 0'),
 'masr_recog_rescore_lm: att_w=0.0': (-1, 'masr_recog_rescore_lm: att_w must be finite and > 0'),
 'masr_recog_rescore_lm: att_w=inf': (-1, 'masr_recog_rescore_lm: att_w must be finite and > 0'),
 'masr_recog_rescore_lm: att_w=nan': (-1, 'masr_recog_rescore_lm: att_w must be finite and > 0'),
 'masr_recog_rescore_lm: ctc_w=-0.5': (-1, 'masr_recog_rescore_lm: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_lm: ctc_w=-1 + null LM': (-1, 'masr_recog_rescore_lm: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_lm: ctc_w=0.0': (-1, 'masr_recog_rescore_lm: null language model'),
 'masr_recog_rescore_lm: ctc_w=inf': (-1, 'masr_recog_rescore_lm: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_lm: ctc_w=nan': (-1, 'masr_recog_rescore_lm: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_lm: no CTC head': (-1, 'masr_recog_rescore_lm: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_rescore_lm: null LM': (-1, 'masr_recog_rescore_lm: null language model'),
 'masr_recog_rescore_lm: null model': (-1, 'masr_recog_rescore_lm: null model'),
 'masr_rescore_nbest: B=0': (-1, 'masr_rescore_nbest: need B >= 1, T >= 4 and 0 <= ld_tok < 3000'),
 'masr_rescore_nbest: N=0': (-1, 'masr_rescore_nbest: N must be in [1, 64]'),
 'masr_rescore_nbest: N=65': (-1, 'masr_rescore_nbest: N must be in [1, 64]'),
 'masr_rescore_nbest: N=65 + att_w=0': (-1, 'masr_rescore_nbest: N must be in [1, 64]'),
 'masr_rescore_nbest: T=3': (-1, 'masr_rescore_nbest: need B >= 1, T >= 4 and 0 <= ld_tok < 3000'),
 'masr_rescore_nbest: att_w=-0.5': (-1, 'masr_rescore_nbest: att_w must be finite and > 0'),
 'masr_rescore_nbest: att_w=0.0': (-1, 'masr_rescore_nbest: att_w must be finite and > 0'),
 'masr_rescore_nbest: att_w=inf': (-1, 'masr_rescore_nbest: att_w must be finite and > 0'),
 'masr_rescore_nbest: att_w=nan': (-1, 'masr_rescore_nbest: att_w must be finite and > 0'),
 'masr_rescore_nbest: ctc_w=-0.5': (-1, 'masr_rescore_nbest: ctc_w must be finite and >= 0'),
 'masr_rescore_nbest: ctc_w=inf': (-1, 'masr_rescore_nbest: ctc_w must be finite and >= 0'),
 'masr_rescore_nbest: ctc_w=inf + null lens_in': (-1, 'masr_rescore_nbest: ctc_w must be finite and >= 0'),
 'masr_rescore_nbest: ctc_w=nan': (-1, 'masr_rescore_nbest: ctc_w must be finite and >= 0'),
 'masr_rescore_nbest: ld=-1': (-1, 'masr_rescore_nbest: need B >= 1, T >= 4 and 0 <= ld_tok < 3000'),
 'masr_rescore_nbest: ld=0 + null tok_in + B=0': (-1, 'masr_rescore_nbest: need B >= 1, T >= 4 and 0 <= ld_tok < 3000'),
 'masr_rescore_nbest: ld=3000': (-1, 'masr_rescore_nbest: need B >= 1, T >= 4 and 0 <= ld_tok < 3000'),
 'masr_rescore_nbest: no CTC head': (-1, 'masr_rescore_nbest: the model has no CTC head (masr_create_ctc)'),
 'masr_rescore_nbest: null att': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null ctc': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null ctc_in': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null ctc_in + ld=3000': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null il': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null lens': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null lens_in': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null model': (-1, 'masr_rescore_nbest: null model'),
 'masr_rescore_nbest: null order': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null sc': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null tok': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null tok_in': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_rescore_nbest: null xs': (-1, 'masr_rescore_nbest: null pointer'),
 'masr_ctc_beam_search_bias: null list': (-1, 'mk_ctc_beam_search_bias: null phrase list'),
 'masr_ctc_beam_search_bias: null list + K=0 + null lg': (-1, 'mk_ctc_beam_search_bias: null phrase list'),
 'masr_ctc_beam_search_nlm: null LM': (-1, 'mk_ctc_beam_search_nlm: null language model'),
 'masr_ctc_beam_search_nlm: null LM + K=0 + null lg': (-1, 'mk_ctc_beam_search_nlm: null language model'),
 'masr_recog_beam_bias: null list': (-1, 'masr_recog_beam_bias: null phrase list'),
 'masr_recog_beam_bias: null list + bias_w=-1 + K=0': (-1, 'masr_recog_beam_bias: null phrase list'),
 'masr_recog_beam_bias: null list + null nbias': (-1, 'masr_recog_beam_bias: null phrase list'),
 'masr_recog_beam_bias: null model': (-1, 'masr_recog_beam_bias: null model'),
 'masr_recog_beam_bias: null model + null list': (-1, 'masr_recog_beam_bias: null model'),
 'masr_recog_beam_ctc_bias: att_w=-0.5': (-1, 'masr_recog_beam_ctc_bias: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_bias: att_w=0.0': (-1, 'masr_recog_beam_ctc_bias: null phrase list'),
 'masr_recog_beam_ctc_bias: att_w=inf': (-1, 'masr_recog_beam_ctc_bias: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_bias: att_w=inf + len_bonus=nan': (-1, 'masr_recog_beam_ctc_bias: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_bias: att_w=nan': (-1, 'masr_recog_beam_ctc_bias: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_bias: ctc_w=-0.5': (-1, 'masr_recog_beam_ctc_bias: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_bias: ctc_w=0 + att_w=-1': (-1, 'masr_recog_beam_ctc_bias: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_bias: ctc_w=0.0': (-1, 'masr_recog_beam_ctc_bias: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_bias: ctc_w=inf': (-1, 'masr_recog_beam_ctc_bias: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_bias: ctc_w=nan': (-1, 'masr_recog_beam_ctc_bias: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_bias: len_bonus=nan': (-1, 'masr_recog_beam_ctc_bias: len_bonus must be finite'),
 'masr_recog_beam_ctc_bias: len_bonus=nan + null list': (-1, 'masr_recog_beam_ctc_bias: len_bonus must be finite'),
 'masr_recog_beam_ctc_bias: no CTC head': (-1, 'masr_recog_beam_ctc_bias: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc_bias: no CTC head + ctc_w=0': (-1, 'masr_recog_beam_ctc_bias: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc_bias: null list': (-1, 'masr_recog_beam_ctc_bias: null phrase list'),
 'masr_recog_beam_ctc_bias: null list + K=0 + N=0': (-1, 'masr_recog_beam_ctc_bias: null phrase list'),
 'masr_recog_beam_ctc_bias: null model': (-1, 'masr_recog_beam_ctc_bias: null model'),
 'masr_recog_beam_ctc_nlm: att_w=-0.5': (-1, 'masr_recog_beam_ctc_nlm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_nlm: att_w=0.0': (-1, 'masr_recog_beam_ctc_nlm: null language model'),
 'masr_recog_beam_ctc_nlm: att_w=inf': (-1, 'masr_recog_beam_ctc_nlm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_nlm: att_w=inf + null LM': (-1, 'masr_recog_beam_ctc_nlm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_nlm: att_w=nan': (-1, 'masr_recog_beam_ctc_nlm: att_w must be finite and >= 0'),
 'masr_recog_beam_ctc_nlm: ctc_w=-0.5': (-1, 'masr_recog_beam_ctc_nlm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_nlm: ctc_w=0 + null LM': (-1, 'masr_recog_beam_ctc_nlm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_nlm: ctc_w=0.0': (-1, 'masr_recog_beam_ctc_nlm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_nlm: ctc_w=inf': (-1, 'masr_recog_beam_ctc_nlm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_nlm: ctc_w=nan': (-1, 'masr_recog_beam_ctc_nlm: ctc_w must be finite and > 0'),
 'masr_recog_beam_ctc_nlm: no CTC head': (-1, 'masr_recog_beam_ctc_nlm: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_beam_ctc_nlm: null LM': (-1, 'masr_recog_beam_ctc_nlm: null language model'),
 'masr_recog_beam_ctc_nlm: null LM + K=0 + N=0': (-1, 'masr_recog_beam_ctc_nlm: null language model'),
 'masr_recog_beam_ctc_nlm: null model': (-1, 'masr_recog_beam_ctc_nlm: null model'),
 'masr_recog_beam_nlm: null LM': (-1, 'masr_recog_beam_nlm: null language model'),
 'masr_recog_beam_nlm: null LM + lm_w=-1 + K=0': (-1, 'masr_recog_beam_nlm: null language model'),
 'masr_recog_beam_nlm: null model': (-1, 'masr_recog_beam_nlm: null model'),
 'masr_recog_beam_nlm: null model + null LM': (-1, 'masr_recog_beam_nlm: null model'),
 'masr_recog_ctc_align: B=0': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: B=0 + T=3': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: T=3': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: maxL=-1': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: maxL=0': (-1, 'masr_recog: not bound'),
 'masr_recog_ctc_align: maxL=1023': (-1, 'masr_recog: not bound'),
 'masr_recog_ctc_align: maxL=1024': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: maxL=1024 + null ys': (-1, 'masr_recog_ctc_align: need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048'),
 'masr_recog_ctc_align: no CTC head': (-1, 'masr_recog_ctc_align: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_ctc_align: no CTC head + null xs': (-1, 'masr_recog_ctc_align: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_ctc_align: null end': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null frames': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null il': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null model': (-1, 'masr_recog_ctc_align: null model'),
 'masr_recog_ctc_align: null ol': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null score': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null score + maxL=1024': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null start': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null xs': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null ys': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null ys + ilens<4': (-1, 'masr_recog_ctc_align: null pointer'),
 'masr_recog_ctc_align: null ys + no token in range': (-1, 'masr_recog: not bound'),
 'masr_recog_ctc_align: valid': (-1, 'masr_recog: not bound'),
 'masr_recog_ctc_beam_bias: K=0': (-1, 'masr_recog_ctc_beam_bias: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam_bias: K=65': (-1, 'masr_recog_ctc_beam_bias: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam_bias: K=65 + N=0': (-1, 'masr_recog_ctc_beam_bias: beam size K must be in [1, 64]'),
 'masr_recog_ctc_beam_bias: N=0': (-1, 'masr_recog_ctc_beam_bias: nbest must be in [1, K]'),
 'masr_recog_ctc_beam_bias: N=0 + null list': (-1, 'masr_recog_ctc_beam_bias: nbest must be in [1, K]'),
 'masr_recog_ctc_beam_bias: no CTC head': (-1, 'masr_recog_ctc_beam_bias: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_ctc_beam_bias: null list': (-1, 'masr_recog_ctc_beam_bias: null phrase list'),
 'masr_recog_ctc_beam_bias: null list + len_bonus=nan + null am': (-1, 'masr_recog_ctc_beam_bias: null phrase list'),
 'masr_recog_ctc_beam_bias: null model': (-1, 'masr_recog_ctc_beam_bias: null model'),
 'masr_recog_ctc_beam_nlm: null LM': (-1, 'masr_recog_ctc_beam_nlm: null language model'),
 'masr_recog_ctc_beam_nlm: null LM + K=0': (-1, 'masr_recog_ctc_beam_nlm: null language model'),
 'masr_recog_ctc_beam_nlm: null LM + no CTC head': (-1, 'masr_recog_ctc_beam_nlm: null language model'),
 'masr_recog_ctc_beam_nlm: null model': (-1, 'masr_recog_ctc_beam_nlm: null model'),
 'masr_recog_rescore_bias: K=0': (-1, 'masr_recog_rescore_bias: beam size K must be in [1, 64]'),
 'masr_recog_rescore_bias: K=65': (-1, 'masr_recog_rescore_bias: beam size K must be in [1, 64]'),
 'masr_recog_rescore_bias: N=0': (-1, 'masr_recog_rescore_bias: N must be in [1, K]'),
 'masr_recog_rescore_bias: N=5 + att_w=0': (-1, 'masr_recog_rescore_bias: N must be in [1, K]'),
 'masr_recog_rescore_bias: att_w=-0.5': (-1, 'masr_recog_rescore_bias: att_w must be finite and > 0'),
 'masr_recog_rescore_bias: att_w=0.0': (-1, 'masr_recog_rescore_bias: att_w must be finite and > 0'),
 'masr_recog_rescore_bias: att_w=inf': (-1, 'masr_recog_rescore_bias: att_w must be finite and > 0'),
 'masr_recog_rescore_bias: att_w=nan': (-1, 'masr_recog_rescore_bias: att_w must be finite and > 0'),
 'masr_recog_rescore_bias: ctc_w=-0.5': (-1, 'masr_recog_rescore_bias: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_bias: ctc_w=-1 + null list': (-1, 'masr_recog_rescore_bias: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_bias: ctc_w=0.0': (-1, 'masr_recog_rescore_bias: null phrase list'),
 'masr_recog_rescore_bias: ctc_w=inf': (-1, 'masr_recog_rescore_bias: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_bias: ctc_w=nan': (-1, 'masr_recog_rescore_bias: ctc_w must be finite and >= 0'),
 'masr_recog_rescore_bias: no CTC head': (-1, 'masr_recog_rescore_bias: the model has no CTC head (masr_create_ctc)'),
 'masr_recog_rescore_bias: null list': (-1, 'masr_recog_rescore_bias: null phrase list'),
 'masr_recog_rescore_bias: null list + null order': (-1, 'masr_recog_rescore_bias: null phrase list'),
 'masr_recog_rescore_bias: null model': (-1, 'masr_recog_rescore_bias: null model'),
 'masr_recog_rescore_nlm: null LM': (-1, 'masr_recog_rescore_nlm: null language model'),
 'masr_recog_rescore_nlm: null LM + att_w=0': (-1, 'masr_recog_rescore_nlm: null language model'),
 'masr_recog_rescore_nlm: null LM + no CTC head': (-1, 'masr_recog_rescore_nlm: null language model'),
 'masr_recog_rescore_nlm: null model': (-1, 'masr_recog_rescore_nlm: null model'),
 'masr_test_ctc_align_logits: not bound': (-1, 'masr_test_ctc_align_logits: null pointer or model not bound'),
 'masr_test_ctc_align_logits: not bound + B=0': (-1, 'masr_test_ctc_align_logits: null pointer or model not bound'),
 'masr_test_ctc_align_logits: not bound + no CTC head': (-1, 'masr_test_ctc_align_logits: null pointer or model not bound'),
 'masr_test_ctc_align_logits: null model': (-1, 'masr_test_ctc_align_logits: null pointer or model not bound'),
 'masr_test_ctc_align_logits: null out + not bound': (-1, 'masr_test_ctc_align_logits: null pointer or model not bound'),
 'masr_test_ctc_beam_logits: not bound': (-1, 'masr_test_ctc_beam_logits: null pointer or model not bound'),
 'masr_test_ctc_beam_logits: not bound + B=0': (-1, 'masr_test_ctc_beam_logits: null pointer or model not bound'),
 'masr_test_ctc_beam_logits: not bound + no CTC head': (-1, 'masr_test_ctc_beam_logits: null pointer or model not bound'),
 'masr_test_ctc_beam_logits: null model': (-1, 'masr_test_ctc_beam_logits: null pointer or model not bound'),
 'masr_test_ctc_beam_logits: null out + not bound': (-1, 'masr_test_ctc_beam_logits: null pointer or model not bound')}


def _compare(got, want):
    assert sorted(got) == sorted(want)                             # the same cases as recorded: none dropped, none new
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_workspace_bytes_are_unchanged(models):
    got = measure_ws(models)
    for tag in ("plain", "hybrid"):
        _compare(got[tag], WS_BYTES[tag])
    # a plain model is refused by the six queries whose decoder needs the head, and by no other
    for k, v in WS_BYTES["plain"].items():
        assert (v == -1) == k.startswith(("masr_beam_ctc_", "masr_ctc_beam_", "masr_rescore_", "masr_ctc_align_")), k
    assert all(v > 0 for v in WS_BYTES["hybrid"].values())
    assert WS_BYTES["hybrid"]["masr_beam_bias_workspace_bytes(B=2, T=40, K=4, L=10)"] == 113078528
    assert WS_BYTES["hybrid"]["masr_beam_ctc_bias_workspace_bytes(B=2, T=40, K=4, N=1, L=10)"] > WS_BYTES["hybrid"]["masr_beam_ctc_lm_workspace_bytes(B=2, T=40, K=4, N=1, L=10)"]
    assert WS_BYTES["hybrid"]["masr_ctc_align_workspace_bytes(B=2, T=40, M=5)"] == 103217408
    l = _cabi.lib()
    assert l.masr_beam_ctc_bias_workspace_bytes(models["hybrid"], 2, 40, 4, 2, 10) == 113149440
    assert l.masr_ctc_beam_workspace_bytes(models["plain"], 2, 40, 4) == -1
    assert l.masr_last_error().decode() == "masr_ctc_beam_workspace_bytes: the model has no CTC head (masr_create_ctc)"
    assert l.masr_beam_workspace_bytes(None, 2, 40, 4, 10) == -1
    assert l.masr_last_error().decode() == "masr_beam_workspace_bytes: need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1"


def test_workspace_refusals_are_unchanged(models):
    _compare(measure_refusals(models), WS_REFUSALS)
    for k, (rc, msg) in WS_REFUSALS.items():
        assert rc == -1 and msg.startswith(k.split()[0] + (": null language model" if "null LM" in k else ": need ")), k


def test_entry_point_faults_are_unchanged(models):
    _compare(measure_faults(models), FAULTS)
    for k, (rc, msg) in FAULTS.items():
        assert rc == -1, k
        if k.endswith(": valid"):
            assert msg == "masr_recog: not bound", k
        if k.endswith(": null list"):
            assert msg.endswith(": null phrase list"), k
