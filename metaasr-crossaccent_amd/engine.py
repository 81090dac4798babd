"""MasrEngine: owner of the flat HBM buffers and thin driver of the libmasr C ABI.

PyTorch is used only as plumbing here: device memory (`torch.empty`), the current HIP stream and
(in parallel.py) `torch.distributed`.  All arithmetic of the hot path runs in libmasr's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import math
import time
from collections import OrderedDict

import numpy as np
import torch

from . import _cabi
from ._cabi import MasrChunkPolicy, MasrConfig, MasrSpecaugPolicy, align_lists, align_outputs, check, check_target_lengths, check_beam_args, check_lm_args, check_nlm_args, lib, nbest_lists, nbest_lists_bias
from .bias import check_bias_args

MASR_TRAIN, MASR_EVAL = 1, 0
CTC_HEAD = ("ctc.ctc_lo.weight", "ctc.ctc_lo.bias")           # parameters of the joint objective's CTC head (asr_model.ctc_weight > 0)


def ctc_weight_of(model_para: dict) -> float:
    """asr_model.ctc_weight (absent = 0: the plain model), validated: 0 <= w < 1"""
    w = float(model_para.get('ctc_weight', 0.0) or 0.0)
    if not 0.0 <= w < 1.0:
        raise ValueError(f"asr_model.ctc_weight must lie in [0, 1), got {w}")
    return w


SPECAUG_KEYS = ("time_warp", "freq_masks", "freq_width", "freq_bins", "time_masks", "time_width", "time_ratio")


def _specaug_policy(policy, idim: int, what: str = "asr_model.specaug"):
    """a SpecAugment policy dict (None: off) -> the complete validated dict, or None when it augments nothing.  Absent keys are 0, freq_bins
    idim.  The bounds are include/masr.h masr_specaug_policy's; a ValueError names the key."""
    if policy is None:
        return None
    if not isinstance(policy, dict):
        raise ValueError(f"{what} must be a mapping of {', '.join(SPECAUG_KEYS)}, got {type(policy).__name__}")
    unknown = sorted(set(policy) - set(SPECAUG_KEYS))
    if unknown:
        raise ValueError(f"{what}: unknown key {unknown[0]} (known: {', '.join(SPECAUG_KEYS)})")
    out = {}
    for k in SPECAUG_KEYS[:-1]:
        v = policy.get(k, idim if k == "freq_bins" else 0)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}.{k} must be an integer, got {v!r}")
        out[k] = int(v)
    r = policy.get("time_ratio", 0.0)
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0.0 <= float(r) <= 1.0:
        raise ValueError(f"{what}.time_ratio must lie in [0, 1], got {r!r}")
    out["time_ratio"] = float(r)
    for k in ("time_warp", "freq_width", "time_width"):
        if out[k] < 0 or out[k] >= 2 ** 31:
            raise ValueError(f"{what}.{k} must be >= 0, got {out[k]}")
    for k in ("freq_masks", "time_masks"):
        if not 0 <= out[k] <= 8:
            raise ValueError(f"{what}.{k} must lie in [0, 8], got {out[k]}")
    if not 1 <= out["freq_bins"] <= idim:
        raise ValueError(f"{what}.freq_bins must lie in [1, idim = {idim}], got {out['freq_bins']}")
    if out["time_warp"] == 0 and out["freq_masks"] == 0 and out["time_masks"] == 0:
        return None
    return out


def specaug_of(model_para: dict):
    """asr_model.specaug (absent or null = off), validated: the policy dict that MasrEngine hands to masr_set_specaug, or None"""
    return _specaug_policy(model_para.get('specaug'), int(model_para["idim"]))


CHUNK_KEYS = ("size", "left", "dynamic")


def _chunk_policy(policy, what: str = "asr_model.chunk"):
    """a chunk policy dict (None: off) -> the complete validated dict {size, left, dynamic}, or None when it masks nothing.  Absent keys: size 0,
    left -1, dynamic 0.  The bounds are include/masr.h masr_chunk_policy's; a ValueError names the key."""
    if policy is None:
        return None
    if not isinstance(policy, dict):
        raise ValueError(f"{what} must be a mapping of {', '.join(CHUNK_KEYS)}, got {type(policy).__name__}")
    unknown = sorted(set(policy) - set(CHUNK_KEYS))
    if unknown:
        raise ValueError(f"{what}: unknown key {unknown[0]} (known: {', '.join(CHUNK_KEYS)})")
    out = {}
    for k, default in zip(CHUNK_KEYS, (0, -1, 0)):
        v = policy.get(k, default)
        if isinstance(v, bool) and k == "dynamic":
            v = int(v)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}.{k} must be an integer, got {v!r}")
        out[k] = int(v)
    if not 0 <= out["size"] < 2 ** 31:
        raise ValueError(f"{what}.size must be >= 0 (encoder frames; 0 = full context), got {out['size']}")
    if not -1 <= out["left"] < 2 ** 31:
        raise ValueError(f"{what}.left must be >= -1 (-1 = every earlier chunk), got {out['left']}")
    if out["dynamic"] not in (0, 1):
        raise ValueError(f"{what}.dynamic must be 0 or 1, got {out['dynamic']}")
    if out["size"] == 0 and out["dynamic"] == 0:
        return None
    return out


def chunk_of(model_para: dict):
    """asr_model.chunk (absent or null = off), validated: the policy dict that MasrEngine hands to masr_set_chunk, or None"""
    return _chunk_policy(model_para.get('chunk'))


def chunk_draw(seed: int, step: int, Tp: int) -> int:
    """the chunk a dynamic policy's training step draws at the dropout position (seed, step) for a batch of Tp encoder frames
    (include/masr.h masr_chunk_draw): 0 = full context, else 1..25"""
    return int(lib().masr_chunk_draw(C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint64(step & (2 ** 64 - 1)), int(Tp)))


def _policy_struct(policy):
    return MasrSpecaugPolicy(*[policy[k] for k in SPECAUG_KEYS])


def specaug(xs: torch.Tensor, ilens, policy, seed: int, step: int) -> torch.Tensor:
    """the stateless operator (include/masr.h masr_specaug): SpecAugment of the device batch xs fp32 [B, T, D] with raw frame lengths ilens
    under `policy` (a dict of SPECAUG_KEYS; absent keys 0, freq_bins D) at the dropout position (seed, step) -> a new tensor.  What an engine with
    this policy feeds its encoder in the training step it runs from dropout_state() == (seed, step)."""
    if not xs.is_cuda:
        raise RuntimeError("specaug needs a device tensor; there is no CPU path")
    xs = xs.contiguous().float()
    B, T, D = xs.shape
    pol = _specaug_policy(policy or {}, D, "policy") or {**dict.fromkeys(SPECAUG_KEYS, 0), "freq_bins": D}
    lens = torch.as_tensor(ilens, dtype=torch.int32).reshape(B).to(xs.device)
    out = torch.empty_like(xs)
    check(lib().masr_specaug(_ptr(xs), _ptr(lens), _ptr(out), B, T, D, C.byref(_policy_struct(pol)), C.c_uint64(seed & (2 ** 64 - 1)),
                             C.c_uint64(step & (2 ** 64 - 1)), C.c_void_p(torch.cuda.current_stream(xs.device).cuda_stream)), "masr_specaug")
    return out


def sinusoid_pe(max_len: int, E: int) -> torch.Tensor:
    """PositionalEncoding buffer, formula of mono_transformer_torch.py:21-28 -> [max_len, 1, E]."""
    pe = torch.zeros(max_len, E)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, E, 2).float() * (-math.log(10000.0) / E))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(1)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class PendingStats:
    """stats block of one batch on its way to the host (MasrEngine.read_stats_async): a ticket of the engine's ring of page-locked
    blocks (include/masr.h masr_stats_post).  The waiting thread first polls the block's words -- they hold MASR_STATS_PENDING until
    the copy lands -- WITHOUT entering the HIP runtime (the task threads are inside its launch path at that moment and the runtime
    serialises callers), then confirms through the event recorded behind the copy (masr_stats_wait: completion + host visibility).
    The block belongs to the engine and is only handed out again once that event has completed, so a dropped handle is harmless."""
    SENTINEL = 0x7FC0DEAD

    def __init__(self, engine, ticket, words):
        self.engine, self.ticket, self.words = engine, ticket, words
        self._result = None

    def ready(self):
        w = self.words
        return not (w[0] == self.SENTINEL or w[1] == self.SENTINEL or w[2] == self.SENTINEL or w[3] == self.SENTINEL)

    def get(self):
        if self._result is not None:                              # (already brought in, e.g. by the engine before its ring wrapped)
            return self._result
        n, t0 = 0, None
        while not self.ready():
            n += 1
            time.sleep(0 if n < 50 else 5e-5)                 # (releases the interpreter to the task threads either way)
            if n % 4096 == 0:
                t0 = t0 or time.monotonic()
                if time.monotonic() - t0 > 300.0:
                    raise RuntimeError("the stats of a queued batch never reached the host (stream wedged, or the batch failed to launch)")
        out = (C.c_float * 4)()
        check(self.engine._l.masr_stats_wait(self.engine.h, self.ticket, out), "masr_stats_wait")
        self._result = {"loss": float(out[0]), "n_correct": float(out[1]), "n_total": float(out[2]), "grad_norm": float(out[3])}
        return self._result


def _best_lists(tok, lens, scores, *nbias):
    """a step beam's best hypotheses -> (B token lists, scores on the host[, credited tokens on the host])"""
    tok, lens = tok.cpu(), lens.cpu()
    return ([tok[b, :int(lens[b])].tolist() for b in range(lens.size(0))], scores.cpu(), *[n.cpu() for n in nbias])


def _nbest_lists_nbias(tok, lens, scores, nbias):
    """the biased joint beam's lists -> per utterance [(token list, score, credited tokens), ...]"""
    return [[(t, sc, int(n)) for t, sc, n in u] for u in nbest_lists(tok, lens, scores, nbias)]


def _rescore_lists(*out):
    tok, lens, scores, att, ctc, order = (t.cpu() for t in out)
    return [[(tok[b, j, :int(lens[b, j])].tolist(), float(scores[b, j]), float(att[b, j]), float(ctc[b, j]), int(order[b, j]))
             for j in range(lens.size(1)) if int(lens[b, j]) >= 0] for b in range(lens.size(0))]


# What MasrEngine._decode runs, per entry point of include/masr.h: (its workspace query, that query's arguments behind the model; the entry
# point's own arguments between the model and the outputs, in its order; the outputs behind tokens, lens, scores as _outputs' `extra`; what
# turns the outputs into the lists of raw=False).  The names are _decode's: lm and bias are handles (lm an n-gram or an LSTM LM, as the entry
# point takes), xs and il the inputs' pointers, r0 / r1 the min / max step ratio, bonus the length bonus, L the token stride of the outputs.
# An entry point with r0 r1 is a step beam: L is the longest utterance's step limit, everywhere else T // 4.  One with N returns lists:
# the outputs are [B, N, ...], else [B, ...].  tests/test_engine_decode_calls_cpu.py pins every call this table leads to.
_DECODES = {
    "masr_recog_beam": ("masr_beam_workspace_bytes", "B T K L", "xs il B T K r0 r1", "", _best_lists),
    "masr_recog_beam_ctc": ("masr_beam_ctc_workspace_bytes", "B T K L", "xs il B T K r0 r1 att_w ctc_w", "", _best_lists),
    "masr_recog_beam_lm": ("masr_beam_lm_workspace_bytes", "B T K L", "lm xs il B T K r0 r1 lm_w", "", _best_lists),
    "masr_recog_beam_nlm": ("masr_beam_nlm_workspace_bytes", "lm B T K L", "lm xs il B T K r0 r1 lm_w", "", _best_lists),
    "masr_recog_beam_bias": ("masr_beam_bias_workspace_bytes", "B T K L", "lm bias xs il B T K r0 r1 lm_w bias_w", "i", _best_lists),
    "masr_recog_beam_ctc_lm": ("masr_beam_ctc_lm_workspace_bytes", "B T K N L", "lm xs il B T K N r0 r1 att_w ctc_w lm_w bonus", "", nbest_lists),
    "masr_recog_beam_ctc_nlm": ("masr_beam_ctc_nlm_workspace_bytes", "lm B T K N L", "lm xs il B T K N r0 r1 att_w ctc_w lm_w bonus", "", nbest_lists),
    "masr_recog_beam_ctc_bias": ("masr_beam_ctc_bias_workspace_bytes", "B T K N L", "lm bias xs il B T K N r0 r1 att_w ctc_w lm_w bonus bias_w", "i",
                                 _nbest_lists_nbias),
    "masr_recog_ctc_beam": ("masr_ctc_beam_workspace_bytes", "B T K", "xs il B T K N", "", nbest_lists),
    "masr_recog_ctc_beam_lm": ("masr_ctc_beam_workspace_bytes", "B T K", "lm xs il B T K N lm_w bonus", "f", nbest_lists),
    "masr_recog_ctc_beam_nlm": ("masr_ctc_beam_nlm_workspace_bytes", "lm B T K", "lm xs il B T K N lm_w bonus", "f", nbest_lists),
    "masr_recog_ctc_beam_bias": ("masr_ctc_beam_workspace_bytes", "B T K", "lm bias xs il B T K N lm_w bonus bias_w", "fi", nbest_lists_bias),
    "masr_recog_rescore": ("masr_rescore_workspace_bytes", "B T K N L", "xs il B T K N att_w ctc_w", "ffi", _rescore_lists),
    "masr_recog_rescore_lm": ("masr_rescore_workspace_bytes", "B T K N L", "lm xs il B T K N lm_w bonus att_w ctc_w", "ffi", _rescore_lists),
    "masr_recog_rescore_nlm": ("masr_rescore_nlm_workspace_bytes", "lm B T K N L", "lm xs il B T K N lm_w bonus att_w ctc_w", "ffi", _rescore_lists),
    "masr_recog_rescore_bias": ("masr_rescore_workspace_bytes", "B T K N L", "lm bias xs il B T K N lm_w bonus bias_w att_w ctc_w", "ffi", _rescore_lists),
}
_DECODE_FLOATS = frozenset("r0 r1 att_w ctc_w lm_w bonus bias_w".split())


class MasrEngine:
    """One model instance on one GPU: flat fp32 params / grads + activation workspace."""

    def __init__(self, model_para: dict, odim: int, label_smoothing: float = 0.0, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("MasrEngine needs a HIP device (MI355X); there is no CPU path")
        self.device = torch.device(device)
        self.model_para = model_para
        self.odim = odim
        self.ctc_weight = ctc_weight_of(model_para)      # joint CTC/attention objective: loss = (1 - w) CE + w CTC (include/masr.h masr_create_ctc)
        policy = specaug_of(model_para)                  # SpecAugment inside the training step (include/masr.h masr_set_specaug; None = off)
        chunk = chunk_of(model_para)                     # chunk mask of the encoder's self-attention (include/masr.h masr_set_chunk; None = off)
        self.cfg = MasrConfig(
            idim=model_para["idim"], odim=odim, d_model=model_para["d_model"], nheads=model_para["nheads"],
            d_inner=model_para["d_inner"], enc_layers=model_para["encoder"]["nlayers"],
            dec_layers=model_para["decoder"]["nlayers"], tie_weights=int(model_para.get("tgt_share_weight", 0) != 0),
            dropout=float(model_para.get("dropout", 0.0)), pos_dropout=float(model_para.get("pos_dropout", 0.0)),
            label_smoothing=float(label_smoothing))
        self._l = lib()
        self.h = self._l.masr_create_ctc(C.byref(self.cfg), self.ctc_weight)
        if not self.h:
            raise _cabi.MasrError("masr_create_ctc: " + self._l.masr_last_error().decode())
        self.numel = int(self._l.masr_param_numel(self.h))
        self.tied = bool(self.cfg.tie_weights)
        with torch.cuda.device(self.device):
            self.params = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
            self.grads = torch.zeros(self.numel, dtype=torch.float32, device=self.device)
            self.pe = sinusoid_pe(3000, self.cfg.d_model).to(self.device).contiguous()
        self.table = OrderedDict()           # name -> (offset, shape)
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        ndim, off = C.c_int(), C.c_int64()
        for i in range(self._l.masr_param_count(self.h)):
            check(self._l.masr_param_info(self.h, i, name, 256, shape, C.byref(ndim), C.byref(off)), "masr_param_info")
            self.table[name.value.decode()] = (int(off.value), tuple(int(shape[k]) for k in range(ndim.value)))
        self.ws = None
        self._ws_key = (0, 0, 0)
        self.specaug = None
        self.set_specaug(policy)                         # (before the first bind: the plan holds the augmented batch)
        self.chunk = None
        self.set_chunk(chunk)
        self._ensure_ws(1, 64, 8)
        self._dirty = True

    # ------------------------------------------------------------------ buffers
    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._l.masr_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ensure_ws(self, B, T, L):
        self._ensure_ws_bytes(int(self._l.masr_workspace_bytes(self.h, B, T, L)))

    def _ensure_ws_bytes(self, need):
        if self.ws is None or self.ws.numel() < need:
            torch.cuda.synchronize(self.device)
            self.ws = None
            self.ws = torch.empty(int(need * 1.05) + 4096, dtype=torch.uint8, device=self.device)
            check(self._l.masr_bind(self.h, _ptr(self.params), _ptr(self.grads), _ptr(self.pe), _ptr(self.ws), self.ws.numel()), "masr_bind")
            self._dirty = True

    def view(self, name, flat=None):
        off, shape = self.table[name]
        flat = self.params if flat is None else flat
        return flat[off:off + int(np.prod(shape))].view(shape)

    def state_dict(self, flat=None, clone=True) -> "OrderedDict[str, torch.Tensor]":
        """Reference key set and order, incl. pos_encoder.pe and the tied alias."""
        sd = OrderedDict()
        for n in self.table:
            v = self.view(n, flat)
            sd[n] = v.clone() if clone else v
            if n == "vgg2enc.bias":
                sd["pos_encoder.pe"] = self.pe.clone() if clone else self.pe
            if n == "char_trans.bias" and self.tied:
                sd["pre_embed.weight"] = sd["char_trans.weight"]
        return sd

    def load_state_dict(self, sd, flat=None):
        """strict, except that a checkpoint without the CTC head loads into a hybrid model (the head keeps what it holds, i.e. its
        fresh initialisation); a checkpoint WITH the head does not load into a plain model"""
        dst = self.params if flat is None else flat
        extra = [k for k in CTC_HEAD if k in sd and k not in self.table]
        if extra:
            raise RuntimeError(f"the checkpoint holds the CTC head {', '.join(extra)} but this model has none (asr_model.ctc_weight is 0): "
                               "set ctc_weight to load it")
        kept = [k for k in CTC_HEAD if k in self.table and k not in sd]
        if kept:
            from .monitor import logger
            logger.notice(f"the checkpoint has no CTC head: {', '.join(kept)} keep their fresh initialisation")
        for n, (off, shape) in self.table.items():
            if n in kept:
                continue
            t = sd[n]
            dst[off:off + t.numel()].copy_(t.detach().reshape(-1).to(torch.float32))
        if flat is None:
            self._dirty = True

    def mark_dirty(self):
        """call after writing self.params outside the C ABI (copy_, all-reduce, ...)"""
        self._dirty = True

    def refresh(self):
        if self._dirty:
            check(self._l.masr_refresh(self.h, self.stream()), "masr_refresh")
            self._dirty = False

    def set_seed(self, seed: int):
        self._l.masr_set_seed(self.h, C.c_uint64(seed & (2 ** 64 - 1)))

    def set_concurrency(self, slots: int):
        """this engine is one of `slots` task slots sharing the GPU (include/masr.h masr_set_concurrency)"""
        self._l.masr_set_concurrency(self.h, int(slots))

    def set_specaug(self, policy):
        """SpecAugment policy of the training steps (include/masr.h masr_set_specaug): a dict of SPECAUG_KEYS as asr_model.specaug, or None = off.
        Evaluation and every recog* never augment.  The next run_batch re-sizes the workspace for the augmented batch."""
        pol = _specaug_policy(policy, self.cfg.idim)
        check(self._l.masr_set_specaug(self.h, C.byref(_policy_struct(pol)) if pol else None), "masr_set_specaug")
        self.specaug = pol

    def specaug_last(self):
        """[B, T, idim] fp32 view (into the workspace) of the augmented batch the last training run_batch fed the encoder"""
        xp, B, T, D = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        check(self._l.masr_specaug_last(self.h, C.byref(xp), C.byref(B), C.byref(T), C.byref(D)), "masr_specaug_last")
        lo, n = xp.value - self.ws.data_ptr(), B.value * T.value * D.value
        return self.ws[lo:lo + n * 4].view(torch.float32).view(B.value, T.value, D.value)

    def set_chunk(self, policy):
        """chunk mask of the encoder's self-attention (include/masr.h masr_set_chunk): a dict of CHUNK_KEYS as asr_model.chunk, or None = off.
        Evaluation and every recog* run under `size`; training steps under `size`, or with dynamic = 1 under the step's draw."""
        pol = _chunk_policy(policy, "policy")
        st = MasrChunkPolicy(*[pol[k] for k in CHUNK_KEYS]) if pol else None
        check(self._l.masr_set_chunk(self.h, C.byref(st) if st else None), "masr_set_chunk")
        self.chunk = pol

    def chunk_last(self) -> int:
        """the chunk (encoder frames; 0 = full context) the last run_batch or recog* ran its encoder with"""
        c = C.c_int()
        check(self._l.masr_chunk_last(self.h, C.byref(c)), "masr_chunk_last")
        return int(c.value)

    def dropout_state(self):
        """(seed, batches run since set_seed): the position of the dropout mask stream (include/masr.h masr_dropout_state)"""
        st = (C.c_uint64 * 2)()
        self._l.masr_dropout_state(self.h, st, 0)
        return int(st[0]), int(st[1])

    def set_dropout_state(self, state):
        st = (C.c_uint64 * 2)(int(state[0]), int(state[1]))
        self._l.masr_dropout_state(self.h, st, 1)

    # ------------------------------------------------------------------ the operator
    def run_batch(self, xs: torch.Tensor, ilens, ys, olens, train: bool):
        """forward + loss (+ backward).  xs: device fp32 [B,T,idim] (host tensors are uploaded);
        ilens/olens: int64 host tensors; ys: list of int64 host tensors."""
        ready = getattr(xs, "_masr_ready", None)               # uploaded ahead on the loader's copy stream (io/dataset.py Loader._materialize_ahead)
        if ready is not None:
            torch.cuda.current_stream(self.device).wait_event(ready)
        if xs.device != self.device:
            xs = xs.to(self.device, non_blocking=True)
        elif xs.is_cuda:
            # made on another stream (HBM-resident shards are gathered on the main stream a meta-step ahead): tell the allocator it
            # is read on this one, or the block could be handed out again while this stream's backward still needs it
            xs.record_stream(torch.cuda.current_stream(self.device))
        xs = xs.contiguous().float()
        B, T, D = xs.shape
        assert D == self.cfg.idim, f"idim mismatch {D} vs {self.cfg.idim}"
        il = torch.as_tensor(ilens, dtype=torch.int64).cpu().contiguous()
        ol = torch.as_tensor(olens, dtype=torch.int64).cpu().contiguous()
        yf = torch.cat([torch.as_tensor(y, dtype=torch.int64).reshape(-1) for y in ys]).cpu().contiguous()
        L = int(ol.max()) + 1
        self._ensure_ws(B, T, L)
        self.refresh()
        check(self._l.masr_run_batch(self.h, _ptr(xs), C.c_void_p(il.data_ptr()), C.c_void_p(yf.data_ptr()),
                                     C.c_void_p(ol.data_ptr()), B, T, MASR_TRAIN if train else MASR_EVAL, self.stream()),
              "masr_run_batch")
        self._last_x = xs          # keep the input alive until the stream has consumed it

    # ------------------------------------------------------------------ decoding: every recog_* below vets its arguments and calls _decode
    def _decode_inputs(self, xs, ilens):
        """xs on this device as contiguous fp32 and ilens as a host int64 tensor -> (xs, il, B, T)"""
        if xs.device != self.device:
            xs = xs.to(self.device, non_blocking=True)
        xs = xs.contiguous().float()
        B, T, D = xs.shape
        return xs, torch.as_tensor(ilens, dtype=torch.int64).cpu().contiguous(), B, T

    def _decode_ws(self, ws_fn, *args):
        """a workspace of at least ws_fn(*args) bytes, bound, with the shadows fresh; a refusal raises under ws_fn's name"""
        need = int(getattr(self._l, ws_fn)(self.h, *args))
        check(need if need < 0 else 0, ws_fn)
        self._ensure_ws_bytes(need)
        self.refresh()

    def _outputs(self, *lead, ld, extra=""):
        """device outputs of a decode: tokens int32 [*lead, ld], lens int32 [*lead], scores fp32 [*lead], then one [*lead] tensor per letter
        of `extra` (f: fp32, i: int32)"""
        kinds = {"i": torch.int32, "f": torch.float32}
        return (torch.empty(*lead, ld, dtype=torch.int32, device=self.device),
                *[torch.empty(*lead, dtype=kinds[k], device=self.device) for k in "if" + extra])

    def _beam_lmax(self, il, min_step_ratio, max_step_ratio):
        return max(ml for ml, _ in self.beam_lengths(il.tolist(), min_step_ratio, max_step_ratio))

    def _decode(self, fn, xs, ilens, raw=False, **v):
        """one decode call: the entry point `fn` as its row of _DECODES describes it, on the arguments `v` that its method has vetted, under
        the row's names.  Inputs, token stride, workspace, outputs, the call, then the device outputs (raw) or the row's lists."""
        ws_fn, ws_args, order, extra, lists = _DECODES[fn]
        order = order.split()
        xs, il, B, T = self._decode_inputs(xs, ilens)
        v.update(xs=_ptr(xs), il=_ptr(il), B=B, T=T)
        v["L"] = self._beam_lmax(il, v["r0"], v["r1"]) if "r0" in order else T // 4
        self._decode_ws(ws_fn, *[v[k] for k in ws_args.split()])
        out = self._outputs(*[v[k] for k in ("B", "N") if k in order], ld=v["L"], extra=extra)
        check(getattr(self._l, fn)(self.h, *[float(v[k]) if k in _DECODE_FLOATS else v[k] for k in order], *map(_ptr, out), self.stream()), fn)
        self._last_x = xs
        return out if raw else lists(*out)

    def recog(self, xs: torch.Tensor, ilens, full: bool = False):
        """greedy decode (MyTransformer.recog): returns int64 [Ldec, B] on the device, Ldec = max(ilens // 4).
        Default = KV-cached incremental decode; full=True = the reference's literal whole-prefix re-decode per step."""
        xs, il, B, T = self._decode_inputs(xs, ilens)
        Ldec = int(il.max()) // 4
        self._decode_ws("masr_workspace_bytes", B, T, Ldec)
        out = torch.zeros(Ldec, B, dtype=torch.int32, device=self.device)
        fn = self._l.masr_recog_full if full else self._l.masr_recog
        check(fn(self.h, _ptr(xs), _ptr(il), B, T, _ptr(out), self.stream()), "masr_recog")
        self._last_x = xs
        return out.to(torch.int64)

    @staticmethod
    def beam_lengths(ilens, min_step_ratio=0.0, max_step_ratio=1.0):
        """per-utterance (maxlen, minlen) of masr_recog_beam, computed as the library does (the ratios as fp32)"""
        rmax, rmin = float(np.float32(max_step_ratio)), float(np.float32(min_step_ratio))
        out = []
        for n in ilens:
            enc = int(n) // 4
            ml = enc if rmax <= 0 else max(1, math.floor(rmax * enc))
            out.append((min(ml, 3000), max(0, math.floor(rmin * enc))))
        return out

    def recog_beam(self, xs: torch.Tensor, ilens, beam_size: int, min_step_ratio: float = 0.0, max_step_ratio: float = 1.0,
                   att_weight: float = 1.0, ctc_weight: float = 0.0):
        """beam search (masr_recog_beam): returns (list of B token lists without sos / eos, fp32 scores [B] on the host).
        K = beam_size in [1, 64]; an utterance's result does not depend on the rest of its batch.  ctc_weight != 0 runs the joint
        CTC/attention search (masr_recog_beam_ctc: needs a hybrid model, ctc_weight > 0, att_weight >= 0); with ctc_weight == 0 the
        attention decoder alone decides and att_weight is not used."""
        K, _ = check_beam_args(beam_size)
        return self._decode("masr_recog_beam_ctc" if float(ctc_weight) != 0.0 else "masr_recog_beam", xs, ilens, K=K, r0=min_step_ratio,
                            r1=max_step_ratio, att_w=att_weight, ctc_w=ctc_weight)

    def recog_beam_lm(self, xs: torch.Tensor, ilens, beam_size: int, lm, lm_w: float, min_step_ratio: float = 0.0, max_step_ratio: float = 1.0):
        """beam search with an n-gram LM fused in (masr_recog_beam_lm): recog_beam's attention-only search with the per-step
        increment log p_att(c | h) + lm_w * lm(c | h).  lm: an NGramLM (lm.py) over this model's odim classes; lm_w finite and >= 0.
        Returns what recog_beam returns: (B token lists without sos / eos, fp32 scores [B] on the host)."""
        K, _ = check_beam_args(beam_size)
        lm_w, _ = check_lm_args(lm, lm_w, 0.0)
        return self._decode("masr_recog_beam_lm", xs, ilens, K=K, lm=lm.h, lm_w=lm_w, r0=min_step_ratio, r1=max_step_ratio)

    def recog_beam_nlm(self, xs: torch.Tensor, ilens, beam_size: int, nlm, lm_w: float, min_step_ratio: float = 0.0, max_step_ratio: float = 1.0):
        """beam search with an LSTM LM fused in (masr_recog_beam_nlm): recog_beam's attention-only search with the per-step
        increment log p_att(c | h) + lm_w * lm(c | h), every hypothesis carrying the LM's recurrent state.  nlm: an LstmLM (nlm.py) over this
        model's odim classes; lm_w finite and >= 0.  Returns what recog_beam returns."""
        K, _ = check_beam_args(beam_size)
        lm_w = check_nlm_args(nlm, lm_w)
        return self._decode("masr_recog_beam_nlm", xs, ilens, K=K, lm=nlm.h, lm_w=lm_w, r0=min_step_ratio, r1=max_step_ratio)

    def recog_beam_ctc_lm(self, xs: torch.Tensor, ilens, beam_size: int, lm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest: int = 1,
                          min_step_ratio: float = 0.0, max_step_ratio: float = 1.0, att_weight: float = 0.7, ctc_weight: float = 0.3,
                          raw: bool = False):
        """one-pass joint CTC/attention beam search with the n-gram LM `lm`, a per-token bonus and an N-best list (masr_recog_beam_ctc_lm,
        DESIGN 5.7; needs a hybrid model): recog_beam's joint search with the LM in the pre-beam and in the score.  lm_w finite and >= 0,
        len_bonus finite of any sign, ctc_weight > 0, att_weight >= 0, nbest in [1, beam_size].  Returns per utterance a list of at most
        nbest (token list, score), best first (raw: the device tensors tokens [B, nbest, Lmax], lens, scores instead)."""
        K, N = check_beam_args(beam_size, nbest)
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus)
        return self._decode("masr_recog_beam_ctc_lm", xs, ilens, raw, K=K, N=N, lm=lm.h, lm_w=lm_w, bonus=len_bonus, r0=min_step_ratio,
                            r1=max_step_ratio, att_w=att_weight, ctc_w=ctc_weight)

    def recog_beam_ctc_nlm(self, xs: torch.Tensor, ilens, beam_size: int, nlm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest: int = 1,
                           min_step_ratio: float = 0.0, max_step_ratio: float = 1.0, att_weight: float = 0.7, ctc_weight: float = 0.3,
                           raw: bool = False):
        """recog_beam_ctc_lm with the LSTM LM `nlm` (an LstmLM over this model's odim classes) in the n-gram's place (masr_recog_beam_ctc_nlm,
        DESIGN 5.11; needs a hybrid model): the LM's term in the pre-beam and in the score, every hypothesis carrying the LM's recurrent
        state.  lm_w finite and >= 0, len_bonus finite of any sign, ctc_weight > 0, att_weight >= 0, nbest in [1, beam_size].  Returns what
        recog_beam_ctc_lm returns: per utterance a list of at most nbest (token list, score), best first (raw: the device tensors)."""
        K, N = check_beam_args(beam_size, nbest)
        lm_w, len_bonus = check_nlm_args(nlm, lm_w, len_bonus)
        return self._decode("masr_recog_beam_ctc_nlm", xs, ilens, raw, K=K, N=N, lm=nlm.h, lm_w=lm_w, bonus=len_bonus, r0=min_step_ratio,
                            r1=max_step_ratio, att_w=att_weight, ctc_w=ctc_weight)

    def recog_ctc_beam(self, xs: torch.Tensor, ilens, beam_size: int, nbest: int = 1, raw: bool = False):
        """CTC prefix beam search on the CTC head alone (masr_recog_ctc_beam; needs a hybrid model): one encoder pass, the
        head GEMM, one sweep over the T/4 frames.  Returns per utterance a list of at most nbest (token list, score), best first
        (raw: the device tensors tokens [B, nbest, T // 4], lens, scores instead)."""
        K, N = check_beam_args(beam_size, nbest)
        return self._decode("masr_recog_ctc_beam", xs, ilens, raw, K=K, N=N)

    def recog_ctc_beam_lm(self, xs: torch.Tensor, ilens, beam_size: int, lm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest: int = 1,
                          raw: bool = False):
        """recog_ctc_beam with the n-gram LM `lm` (an NGramLM over this model's odim classes) and a per-token bonus fused into the search
        (masr_recog_ctc_beam_lm).  lm_w finite and >= 0, len_bonus finite of any sign.  Returns per utterance a list of at most
        nbest (token list, fused score, acoustic score), best first (raw: the device tensors tokens, lens, scores, am instead)."""
        K, N = check_beam_args(beam_size, nbest)
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus)
        return self._decode("masr_recog_ctc_beam_lm", xs, ilens, raw, K=K, N=N, lm=lm.h, lm_w=lm_w, bonus=len_bonus)

    def recog_ctc_beam_bias(self, xs: torch.Tensor, ilens, beam_size: int, bias, bias_w: float = 3.0, lm=None, lm_w: float = 0.3,
                            len_bonus: float = 0.0, nbest: int = 1, raw: bool = False):
        """recog_ctc_beam with contextual phrase biasing (masr_recog_ctc_beam_bias): `bias` a ContextBias over this model's odim
        classes, bias_w finite and >= 0; with lm (an NGramLM) the n-gram LM and the bonus are fused in as recog_ctc_beam_lm does, without
        one lm_w and len_bonus are ignored.  Returns per utterance a list of at most nbest (token list, final score, acoustic score,
        credited tokens), best first (raw: the device tensors tokens, lens, scores, am, nbias instead)."""
        K, N = check_beam_args(beam_size, nbest)
        bias_w = check_bias_args(bias, bias_w)
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus) if lm is not None else (0.0, 0.0)
        return self._decode("masr_recog_ctc_beam_bias", xs, ilens, raw, K=K, N=N, lm=getattr(lm, "h", None), bias=bias.h, lm_w=lm_w, bonus=len_bonus,
                            bias_w=bias_w)

    def recog_beam_bias(self, xs: torch.Tensor, ilens, beam_size: int, bias, bias_w: float = 3.0, lm=None, lm_w: float = 0.3,
                        min_step_ratio: float = 0.0, max_step_ratio: float = 1.0, raw: bool = False):
        """the attention beam with contextual phrase biasing (masr_recog_beam_bias): recog_beam's search -- with lm (an NGramLM)
        recog_beam_lm's -- whose per-step increment also carries bias_w per token credited by the phrase automaton of `bias` (a ContextBias
        over this model's odim classes); bias_w finite and >= 0, without an LM lm_w is ignored.  Returns (B token lists without sos / eos,
        fp32 scores [B] on the host, credited tokens int32 [B] on the host); raw: the device tensors tokens, lens, scores, nbias instead."""
        K, _ = check_beam_args(beam_size)
        bias_w = check_bias_args(bias, bias_w)
        lm_w, _ = check_lm_args(lm, lm_w, 0.0) if lm is not None else (0.0, 0.0)
        return self._decode("masr_recog_beam_bias", xs, ilens, raw, K=K, lm=getattr(lm, "h", None), bias=bias.h, lm_w=lm_w, bias_w=bias_w,
                            r0=min_step_ratio, r1=max_step_ratio)

    def recog_beam_ctc_bias(self, xs: torch.Tensor, ilens, beam_size: int, bias, bias_w: float = 3.0, lm=None, lm_w: float = 0.3,
                            len_bonus: float = 0.0, nbest: int = 1, min_step_ratio: float = 0.0, max_step_ratio: float = 1.0,
                            att_weight: float = 0.7, ctc_weight: float = 0.3, raw: bool = False):
        """the one-pass joint CTC/attention beam with contextual phrase biasing (masr_recog_beam_ctc_bias; needs a hybrid model):
        recog_beam_ctc_lm's search with the automaton's term in the pre-beam and in the score; lm may be None (no LM term; lm_w is ignored, the
        bonus is kept).  Returns per utterance a list of at most nbest (token list, score, credited tokens), best first (raw: the device
        tensors tokens [B, nbest, Lmax], lens, scores, nbias instead)."""
        K, N = check_beam_args(beam_size, nbest)
        bias_w = check_bias_args(bias, bias_w)
        if lm is not None:
            lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus)
        else:
            lm_w, len_bonus = 0.0, float(len_bonus)
            if not math.isfinite(len_bonus):
                raise ValueError(f"len_bonus must be finite, got {len_bonus}")
        return self._decode("masr_recog_beam_ctc_bias", xs, ilens, raw, K=K, N=N, lm=getattr(lm, "h", None), bias=bias.h, lm_w=lm_w, bonus=len_bonus,
                            bias_w=bias_w, r0=min_step_ratio, r1=max_step_ratio, att_w=att_weight, ctc_w=ctc_weight)

    def recog_rescore_bias(self, xs: torch.Tensor, ilens, beam_size: int, bias, bias_w: float = 3.0, lm=None, lm_w: float = 0.3,
                           len_bonus: float = 0.0, nbest=None, att_w: float = 0.5, ctc_w: float = 0.5, raw: bool = False):
        """recog_rescore whose first pass is recog_ctc_beam_bias's search (masr_recog_rescore_bias): the `ctc` of an entry is
        that pass's final score; the attention pass is not biased.  Returns what recog_rescore returns."""
        K, N = check_beam_args(beam_size, nbest)
        att_w, ctc_w = self._rescore_weights(att_w, ctc_w)
        bias_w = check_bias_args(bias, bias_w)
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus) if lm is not None else (0.0, 0.0)
        return self._decode("masr_recog_rescore_bias", xs, ilens, raw, K=K, N=N, lm=getattr(lm, "h", None), bias=bias.h, lm_w=lm_w, bonus=len_bonus,
                            bias_w=bias_w, att_w=att_w, ctc_w=ctc_w)

    def recog_ctc_beam_nlm(self, xs: torch.Tensor, ilens, beam_size: int, nlm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest: int = 1,
                           raw: bool = False):
        """recog_ctc_beam_lm with the LSTM LM `nlm` (an LstmLM over this model's odim classes) in the n-gram's place
        (masr_recog_ctc_beam_nlm): the search runs frame by frame, every beam row carrying the LM's recurrent state.  lm_w
        finite and >= 0, len_bonus finite of any sign.  Returns what recog_ctc_beam_lm returns: per utterance a list of at most nbest
        (token list, fused score, acoustic score), best first (raw: the device tensors tokens, lens, scores, am instead)."""
        K, N = check_beam_args(beam_size, nbest)
        lm_w, len_bonus = check_nlm_args(nlm, lm_w, len_bonus)
        return self._decode("masr_recog_ctc_beam_nlm", xs, ilens, raw, K=K, N=N, lm=nlm.h, lm_w=lm_w, bonus=len_bonus)

    def ctc_align(self, xs: torch.Tensor, ilens, ys, olens, raw: bool = False):
        """CTC forced alignment of each utterance's transcript on the CTC head (masr_recog_ctc_align; needs a hybrid model): one
        encoder pass, the head GEMM, one Viterbi sweep over the T/4 frames.  ys: per-utterance token lists / tensors without sos / eos, olens
        their lengths.  Returns per utterance (score, [(token, start, end), ...], frames list), start / end / frames in ENCODER frames (4 input
        frames each); an infeasible utterance has score -inf and empty lists (raw: the device tensors frames [B, T // 4], start / end
        [B, maxL], score [B] instead)."""
        xs, il, B, T = self._decode_inputs(xs, ilens)
        ol = torch.as_tensor(olens, dtype=torch.int64).cpu().contiguous()
        ys = [torch.as_tensor(y, dtype=torch.int64).reshape(-1) for y in ys]
        check_target_lengths(ys, ol.tolist())
        # each transcript cut to its olens[b] (a row of a padded tensor may be longer): the library reads olens[b] tokens per utterance
        ys = [y[:max(int(n), 0)] for y, n in zip(ys, ol.tolist())]
        yf = torch.cat(ys + [torch.zeros(1, dtype=torch.int64)]).contiguous()      # (never empty: the pointer is never null)
        maxL = max(int(ol.max()), 0)
        self._decode_ws("masr_ctc_align_workspace_bytes", B, T, maxL)
        out, ptrs = align_outputs(B, T // 4, maxL, self.device)
        check(self._l.masr_recog_ctc_align(self.h, _ptr(xs), _ptr(il), B, T, _ptr(yf), _ptr(ol), maxL, *ptrs, self.stream()),
              "masr_recog_ctc_align")
        self._last_x = xs
        return out if raw else align_lists(*out, [y.tolist() for y in ys], ol.tolist())

    @staticmethod
    def _rescore_weights(att_w, ctc_w):
        att_w, ctc_w = float(att_w), float(ctc_w)
        if not (math.isfinite(att_w) and att_w > 0.0):
            raise ValueError(f"att_w must be finite and > 0, got {att_w}")
        if not (math.isfinite(ctc_w) and ctc_w >= 0.0):
            raise ValueError(f"ctc_w must be finite and >= 0, got {ctc_w}")
        return att_w, ctc_w

    def _rescore_outputs(self, B, N, ld):
        """tokens, lens, scores, att, ctc, order"""
        return self._outputs(B, N, ld=ld, extra="ffi")

    def recog_rescore(self, xs: torch.Tensor, ilens, beam_size: int, nbest=None, att_w: float = 0.5, ctc_w: float = 0.5, raw: bool = False):
        """attention rescoring of the CTC beam's N-best (masr_recog_rescore; needs a hybrid model): the CTC prefix beam of
        recog_ctc_beam(beam_size, nbest), then ONE teacher-forced decoder pass over all B * nbest hypotheses, and the list re-ranked by
        att_w * log p_att + ctc_w * log p_ctc.  Returns per utterance a list of (tokens, score, att, ctc, first_pass_rank), best first
        (raw: the device tensors tokens, lens, scores, att, ctc, order instead).  The call waits for the stream once, between the passes."""
        K, N = check_beam_args(beam_size, nbest)
        att_w, ctc_w = self._rescore_weights(att_w, ctc_w)
        return self._decode("masr_recog_rescore", xs, ilens, raw, K=K, N=N, att_w=att_w, ctc_w=ctc_w)

    def recog_rescore_lm(self, xs: torch.Tensor, ilens, beam_size: int, lm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest=None,
                         att_w: float = 0.5, ctc_w: float = 0.5, raw: bool = False):
        """recog_rescore whose first pass is recog_ctc_beam_lm's LM-fused search (masr_recog_rescore_lm): the `ctc` of an entry
        is that pass's fused score.  Returns what recog_rescore returns."""
        K, N = check_beam_args(beam_size, nbest)
        att_w, ctc_w = self._rescore_weights(att_w, ctc_w)
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus)
        return self._decode("masr_recog_rescore_lm", xs, ilens, raw, K=K, N=N, lm=lm.h, lm_w=lm_w, bonus=len_bonus, att_w=att_w, ctc_w=ctc_w)

    def recog_rescore_nlm(self, xs: torch.Tensor, ilens, beam_size: int, nlm, lm_w: float = 0.3, len_bonus: float = 0.0, nbest=None,
                          att_w: float = 0.5, ctc_w: float = 0.5, raw: bool = False):
        """recog_rescore whose first pass is recog_ctc_beam_nlm's LSTM-LM-fused search (masr_recog_rescore_nlm): the `ctc` of an
        entry is that pass's fused score.  Returns what recog_rescore returns."""
        K, N = check_beam_args(beam_size, nbest)
        att_w, ctc_w = self._rescore_weights(att_w, ctc_w)
        lm_w, len_bonus = check_nlm_args(nlm, lm_w, len_bonus)
        return self._decode("masr_recog_rescore_nlm", xs, ilens, raw, K=K, N=N, lm=nlm.h, lm_w=lm_w, bonus=len_bonus, att_w=att_w, ctc_w=ctc_w)

    def rescore_nbest(self, xs: torch.Tensor, ilens, tokens, lens, ctc, att_w: float = 0.5, ctc_w: float = 0.5, raw: bool = False):
        """attention rescoring of a caller's N-best lists (masr_rescore_nbest): tokens int32 [B, N, ld], lens int32 [B, N] (-1 = no entry),
        ctc fp32 [B, N] (the first-pass scores); every token of a live list in [1, odim - 2].  Returns what recog_rescore returns."""
        att_w, ctc_w = self._rescore_weights(att_w, ctc_w)
        xs, il, B, T = self._decode_inputs(xs, ilens)
        tokens = torch.as_tensor(tokens).to(self.device, torch.int32).contiguous()
        lens = torch.as_tensor(lens).to(self.device, torch.int32).contiguous()
        ctc = torch.as_tensor(ctc).to(self.device, torch.float32).contiguous()
        if tokens.dim() != 3 or tokens.size(0) != B or lens.shape != tokens.shape[:2] or ctc.shape != lens.shape:
            raise ValueError("rescore_nbest needs tokens [B, N, ld], lens [B, N] and ctc [B, N]")
        N, ld = tokens.size(1), tokens.size(2)
        if not 1 <= N <= 64:
            raise ValueError(f"N must be in [1, 64], got {N}")
        self._decode_ws("masr_rescore_workspace_bytes", B, T, N, N, max(0, int(lens.max())))
        out = self._rescore_outputs(B, N, ld)
        check(self._l.masr_rescore_nbest(self.h, _ptr(xs), _ptr(il), B, T, N, _ptr(tokens), ld, _ptr(lens), _ptr(ctc), att_w, ctc_w,
                                         *map(_ptr, out), self.stream()), "masr_rescore_nbest")
        self._last_x = xs
        return out if raw else _rescore_lists(*out)

    def _ws_view(self, ptr, count, dtype):
        """`count` elements of `dtype` at the device address `ptr`, as a view into the workspace"""
        off = ptr - self.ws.data_ptr()
        return self.ws[off:off + count * torch.empty(0, dtype=dtype).element_size()].view(dtype)

    def _head_logits_view(self, B, T, lp, ld, ep):
        """(head logits fp32 [B, T // 4, ld], enc_lens int32 [B]) at the addresses a masr_test_*_logits hook answered"""
        return self._ws_view(lp.value, B * (T // 4) * ld.value, torch.float32).view(B, T // 4, ld.value), self._ws_view(ep.value, B, torch.int32)

    def last_rescore_logits(self):
        """test hook (include/masr_test.h masr_test_rescore_logits): what the last rescoring call's score kernel read, as views into the
        workspace: (decoder logits fp32 [R, L, ld], gold int32 [R, L]); row r = b * N + first-pass rank"""
        lp, gp, ld, R, L = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int(), C.c_int()
        check(self._l.masr_test_rescore_logits(self.h, C.byref(lp), C.byref(ld), C.byref(gp), C.byref(R), C.byref(L)), "masr_test_rescore_logits")
        R, L = R.value, L.value
        return self._ws_view(lp.value, R * L * ld.value, torch.float32).view(R, L, ld.value), self._ws_view(gp.value, R * L, torch.int32).view(R, L)

    def last_ctc_beam_logits(self, B, T, K):
        """test hook (include/masr_test.h masr_test_ctc_beam_logits): what the last recog_ctc_beam of this (B, T, K) searched, as views
        into the workspace: (head logits fp32 [B, T // 4, ld], enc_lens int32 [B])"""
        lp, ep, ld = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._l.masr_test_ctc_beam_logits(self.h, B, T, K, C.byref(lp), C.byref(ld), C.byref(ep)), "masr_test_ctc_beam_logits")
        return self._head_logits_view(B, T, lp, ld, ep)

    def last_ctc_align_logits(self, B, T, maxL):
        """test hook (include/masr_test.h masr_test_ctc_align_logits): what the last ctc_align of this (B, T, maxL) aligned to, as views into
        the workspace: (head logits fp32 [B, T // 4, ld], enc_lens int32 [B])"""
        lp, ep, ld = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._l.masr_test_ctc_align_logits(self.h, B, T, maxL, C.byref(lp), C.byref(ld), C.byref(ep)), "masr_test_ctc_align_logits")
        return self._head_logits_view(B, T, lp, ld, ep)

    # ------------------------------------------------------------------ streaming first pass (include/masr.h masr_stream_*)
    def stream_begin(self, B: int, max_frames: int):
        """open a stream of B utterances of at most max_frames input frames under the engine's chunk policy (size > 0; needs a hybrid model)"""
        self._decode_ws("masr_stream_workspace_bytes", int(B), int(max_frames))
        check(self._l.masr_stream_begin(self.h, int(B), int(max_frames), self.stream()), "masr_stream_begin")
        self._stream_shape = (int(B), int(max_frames))
        self._stream_beam = None

    def stream_feed(self, xs: torch.Tensor, valid=None, last: bool = False) -> int:
        """the next piece xs [B, n, idim] of every utterance; valid[b] < n ends utterance b (later pieces must give it 0).  Returns the number
        of encoder frames emitted so far."""
        if xs.device != self.device:
            xs = xs.to(self.device, non_blocking=True)
        xs = xs.contiguous().float()
        n = int(xs.shape[1])
        v = None if valid is None else (C.c_int32 * xs.shape[0])(*[int(x) for x in valid])
        out = C.c_int(0)
        check(self._l.masr_stream_feed(self.h, _ptr(xs) if n else None, n, v, int(bool(last)), C.byref(out), self.stream()), "masr_stream_feed")
        self._last_x = xs
        return out.value

    def stream_partial(self):
        """the greedy result so far as views into the workspace: (tokens int32 [B, ld], frames int32 [B, ld], lens int32 [B])"""
        tp, fp, lp, ld = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        check(self._l.masr_stream_partial(self.h, C.byref(tp), C.byref(fp), C.byref(lp), C.byref(ld)), "masr_stream_partial")
        B = self._stream_shape[0]
        return (self._ws_view(tp.value, B * ld.value, torch.int32).view(B, ld.value),
                self._ws_view(fp.value, B * ld.value, torch.int32).view(B, ld.value), self._ws_view(lp.value, B, torch.int32))

    def stream_logits(self):
        """the accumulated head logits as views into the workspace: (logits fp32 [B, max_frames // 4, ld], enc_lens int32 [B], frames emitted)"""
        gp, ep, ld, fr = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int()
        check(self._l.masr_stream_logits(self.h, C.byref(gp), C.byref(ld), C.byref(ep), C.byref(fr)), "masr_stream_logits")
        B, cap = self._stream_shape[0], self._stream_shape[1] // 4
        return self._ws_view(gp.value, B * cap * ld.value, torch.float32).view(B, cap, ld.value), self._ws_view(ep.value, B, torch.int32), fr.value

    def stream_ctc_beam(self, beam_size: int, nbest: int = 1, raw: bool = False):
        """after the last piece: the CTC prefix beam of recog_ctc_beam on the logits the stream left behind"""
        K, N = check_beam_args(beam_size, nbest)
        B, cap = self._stream_shape[0], self._stream_shape[1] // 4
        out = self._outputs(B, N, ld=cap)
        check(self._l.masr_stream_ctc_beam(self.h, K, N, *map(_ptr, out), self.stream()), "masr_stream_ctc_beam")
        return out if raw else nbest_lists(*out)

    def stream_beam_open(self, beam_size: int, lm=None, lm_w: float = 0.3, len_bonus: float = 0.0, bias=None, bias_w: float = 3.0):
        """open the resumable CTC prefix beam on the open stream (masr_stream_beam_open): it runs the frames emitted so far at once
        and from the next feed on follows the chunks, with the n-gram LM `lm` and the phrase list `bias` fused in if given (as recog_ctc_beam_lm / recog_ctc_beam_bias do)."""
        K, _ = check_beam_args(beam_size)
        bias_w = check_bias_args(bias, bias_w) if bias is not None else 0.0
        lm_w, len_bonus = check_lm_args(lm, lm_w, len_bonus) if lm is not None else (0.0, 0.0)
        check(self._l.masr_stream_beam_open(self.h, K, getattr(lm, "h", None), lm_w, len_bonus, getattr(bias, "h", None), bias_w, self.stream()),
              "masr_stream_beam_open")
        self._stream_beam = (K, lm is not None, bias is not None, lm, bias)       # (the LM and the list stay alive with the beam)

    def stream_beam_result(self, nbest: int = 1, raw: bool = False):
        """the open beam's result after the frames emitted so far (masr_stream_beam_result): the partial N-best, after the last piece the
        final one.  Lists as recog_ctc_beam / _lm / _bias return them (raw: the device tensors tokens, lens, scores[, am[, nbias]])."""
        beam = getattr(self, "_stream_beam", None)
        K, with_lm, with_bias = beam[:3] if beam else (64, False, False)       # (without a beam the call below says so)
        K, N = check_beam_args(K, nbest)
        B, cap = self._stream_shape[0], self._stream_shape[1] // 4
        out = self._outputs(B, N, ld=cap, extra="fi" if with_bias else "f" if with_lm else "")
        ptrs = list(map(_ptr, out)) + [None] * (6 - len(out))
        check(self._l.masr_stream_beam_result(self.h, N, *ptrs[:5], self.stream()), "masr_stream_beam_result")
        return out if raw else (nbest_lists_bias if with_bias else nbest_lists)(*out)

    def recog_stream(self, xs: torch.Tensor, ilens, piece: int, beam_size=None, nbest: int = 1, sync_beam: bool = False, lm=None,
                     lm_w: float = 0.3, len_bonus: float = 0.0, bias=None, bias_w: float = 3.0):
        """the padded batch xs [B, T, idim] streamed in pieces of `piece` input frames, `valid` derived from ilens.  Returns per utterance
        (greedy token list, the encoder frame of each token); with beam_size the final beam's lists as recog_ctc_beam returns them.
        sync_beam (needs beam_size): the resumable beam follows the feeds (stream_beam_open with lm / bias); returns (the final lists, per
        feed the partial top-1 token list of every utterance)."""
        if int(piece) < 1:
            raise ValueError("recog_stream: piece must be >= 1")
        if sync_beam and beam_size is None:
            raise ValueError("recog_stream: sync_beam needs a beam_size")
        xs, il, B, T = self._decode_inputs(xs, ilens)
        self.stream_begin(B, T)
        if sync_beam:
            self.stream_beam_open(beam_size, lm, lm_w, len_bonus, bias, bias_w)
        partials = []
        for t0 in range(0, T, int(piece)):
            t1 = min(T, t0 + int(piece))
            self.stream_feed(xs[:, t0:t1], [max(0, min(int(l), t1) - t0) for l in il.tolist()], last=t1 == T)
            if sync_beam:
                partials.append([u[0][0] if u else [] for u in self.stream_beam_result(1)])
        if sync_beam:
            return self.stream_beam_result(nbest), partials
        if beam_size is not None:
            return self.stream_ctc_beam(beam_size, nbest)
        tok, frm, lens = (t.cpu() for t in self.stream_partial())
        return [(tok[b, :int(lens[b])].tolist(), frm[b, :int(lens[b])].tolist()) for b in range(B)]

    def read_stats(self):
        out = (C.c_float * 4)()
        check(self._l.masr_read_stats(self.h, out, self.stream()), "masr_read_stats")
        self._last_stats = {"loss": float(out[0]), "n_correct": float(out[1]), "n_total": float(out[2]), "grad_norm": float(out[3])}
        return self._last_stats

    def read_stats_async(self):
        """the same block, copied into page-locked memory by the stream WITHOUT waiting for it (include/masr.h masr_stats_post):
        returns a handle whose .get() waits for that copy only.  The host can then queue the next tasks while these run; the stats
        are what the log lines need one meta-step later."""
        ticket = int(self._l.masr_stats_post(self.h, self.stream()))
        if ticket < 0:
            raise _cabi.MasrError("masr_stats_post: " + self._l.masr_last_error().decode())
        h = PendingStats(self, ticket, self._l.masr_stats_peek(self.h, ticket))
        # a ticket expires after 64 newer posts (the ring of include/masr.h).  A loop that keeps a whole meta-step of handles per
        # engine (FOMAML, many tasks on one slot) could get there: handles still unread when the ring is 3/4 around are read NOW
        # (their copies are dozens of batches old) and keep the numbers, so the limit never reaches a caller
        out = self.__dict__.setdefault("_outstanding", [])
        out.append(h)
        while len(out) > 48:
            out.pop(0).get()
        return h

    def set_step_graphs(self, on: bool):
        """opt-in graph replay of repeated batch shapes (include/masr.h masr_set_step_graphs)"""
        self._l.masr_set_step_graphs(self.h, int(bool(on)))

    def set_split_wgrad_launches(self, on: bool):
        """the step's Linear weight gradients as two launches instead of one (include/masr.h masr_set_split_wgrad_launches; A/B, same bits)"""
        self._l.masr_set_split_wgrad_launches(self.h, int(bool(on)))

    def set_ksplit(self, on: bool):
        """k-split of the decoder's long-reduction few-row GEMMs with the combine inside the next LayerNorm (include/masr.h masr_set_ksplit).
        Default OFF: it changes the fp32 summation order of those GEMMs, so it follows only this call, never the slot count.  The one-task-per-stream
        loops (train.py: mono / multi interface) turn it on (+3 %); the FOMAML interface leaves it off for every --tasks_per_gpu."""
        self._l.masr_set_ksplit(self.h, int(bool(on)))

    def set_drop_nan_grads(self, on: bool):
        """clip_grads / clip_accumulate turn a gradient whose norm is NaN into zeros (include/masr.h masr_set_drop_nan_grads; pretrain.py
        --fix_nan_meta_grad).  Default off: the reference accumulates the NaNs (fo_meta_interface.py:151-154)."""
        self._l.masr_set_drop_nan_grads(self.h, int(bool(on)))

    def step_counters(self):
        """{'direct', 'captured', 'replayed'}: how run_batch calls reached the GPU (kernel by kernel / graph capture / graph replay);
        'ksplit_gemms': k-split GEMM launches of the last step launched or captured (0 = whole reductions: masr_set_ksplit off)"""
        out = (C.c_int64 * 4)()
        self._l.masr_step_counters(self.h, out)
        return {"direct": int(out[0]), "captured": int(out[1]), "replayed": int(out[2]), "ksplit_gemms": int(out[3])}

    def last_logits(self):
        """[B, L, odim] fp32 view of the last forward's logits and gold [B, L] (int32, -1 = pad)."""
        lp, gp = C.c_void_p(), C.c_void_p()
        rows, L, ld = C.c_int(), C.c_int(), C.c_int()
        check(self._l.masr_last_logits(self.h, C.byref(lp), C.byref(gp), C.byref(rows), C.byref(L), C.byref(ld)), "masr_last_logits")
        ws_base = self.ws.data_ptr()
        lo = (lp.value - ws_base)
        logits = self.ws[lo:lo + rows.value * ld.value * 4].view(torch.float32).view(rows.value // L.value, L.value, ld.value)[..., :self.odim]
        go = (gp.value - ws_base)
        gold = self.ws[go:go + rows.value * 4].view(torch.int32).view(rows.value // L.value, L.value)
        return logits, gold

    # ------------------------------------------------------------------ optimiser passes
    def clip_sgd_step(self, momentum_buf, max_norm, lr, momentum, nesterov, first_step):
        check(self._l.masr_clip_sgd_step(self.h, _ptr(momentum_buf), max_norm, lr, momentum, int(nesterov), int(first_step), self.stream()),
              "masr_clip_sgd_step")
        self._dirty = False            # the C call refreshes the shadows itself

    def clip_grads(self, max_norm):
        check(self._l.masr_clip_grads(self.h, max_norm, self.stream()), "masr_clip_grads")

    def clip_accumulate(self, updates, max_norm):
        check(self._l.masr_clip_accumulate(self.h, _ptr(updates), max_norm, self.stream()), "masr_clip_accumulate")

    def grad_norm(self):
        check(self._l.masr_grad_norm(self.h, self.stream()), "masr_grad_norm")

    def grad_norm_device_ptr(self):
        """address of the device float that holds the gradient norm after grad_norm() / clip_grads() (include/masr.h masr_stats_device)"""
        return int(self._l.masr_stats_device(self.h)) + 3 * 4

    def adam_step(self, params, grads, m, v, lr, b1, b2, eps, step, weight_decay=0.0, decoupled=False):
        if weight_decay:
            check(self._l.masr_adamw_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), lr, b1, b2, eps, weight_decay,
                                          int(decoupled), step, self.stream()), "masr_adamw_step")
        else:
            check(self._l.masr_adam_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), lr, b1, b2, eps, step, self.stream()), "masr_adam_step")

    def adam_step_guarded(self, params, grads, m, v, lr_a, t_a, lr_b, t_b, b1, b2, eps, weight_decay, decoupled, slot):
        """Adam / AdamW step skipped on the device when the stats block's gradient norm is NaN (include/masr.h masr_adam_step_guarded)"""
        check(self._l.masr_adam_step_guarded(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), lr_a, t_a, lr_b, t_b, b1, b2, eps,
                                             weight_decay, int(decoupled), slot, self.stream()), "masr_adam_step_guarded")

    def adam_sum_step(self, params, grad_list, gscale, m, v, lr, b1, b2, eps, step):
        """Adam on (sum of grad_list, in order) * gscale in one pass (include/masr.h masr_adam_sum_step)"""
        arr = (C.c_void_p * len(grad_list))(*[g.data_ptr() for g in grad_list])
        check(self._l.masr_adam_sum_step(_ptr(params), arr, len(grad_list), gscale, _ptr(m), _ptr(v), params.numel(), lr, b1, b2, eps, step,
                                         self.stream()), "masr_adam_sum_step")

    def sum_n(self, out, grad_list, scale=1.0):
        """out = (sum of grad_list, in order) * scale in one pass (include/masr.h masr_sum_n)"""
        arr = (C.c_void_p * len(grad_list))(*[g.data_ptr() for g in grad_list])
        check(self._l.masr_sum_n(_ptr(out), arr, len(grad_list), scale, out.numel(), self.stream()), "masr_sum_n")

    def radam_step(self, params, grads, m, v, lr, b1, b2, eps, step, weight_decay=0.0, variant=1):
        """variant 1: torch_optimizer.RAdam's conventions (the reference's import), 0: torch.optim.RAdam's (include/masr.h)"""
        check(self._l.masr_radam_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), params.numel(), lr, b1, b2, eps, weight_decay, step, int(variant),
                                      self.stream()), "masr_radam_step")

    def sgd_step(self, params, grads, mom, lr, momentum, nesterov, first_step):
        check(self._l.masr_sgd_step(_ptr(params), _ptr(grads), _ptr(mom), params.numel(), lr, momentum, int(nesterov), int(first_step), self.stream()), "masr_sgd_step")

    def scale(self, x, a):
        check(self._l.masr_scale(_ptr(x), x.numel(), a, self.stream()), "masr_scale")

    def axpy(self, y, x, a):
        check(self._l.masr_axpy(_ptr(y), _ptr(x), x.numel(), a, self.stream()), "masr_axpy")

    def copy(self, dst, src):
        check(self._l.masr_copy(_ptr(dst), _ptr(src), src.numel(), self.stream()), "masr_copy")

    # ------------------------------------------------------------------ profiling
    def profile(self, on: bool):
        check(self._l.masr_profile_enable(self.h, int(on)), "masr_profile_enable")

    def profile_read(self):
        ms = (C.c_float * len(_cabi.PROF_NAMES))()
        n = (C.c_int * len(_cabi.PROF_NAMES))()
        check(self._l.masr_profile_read(self.h, ms, n), "masr_profile_read")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_cabi.PROF_NAMES)}
