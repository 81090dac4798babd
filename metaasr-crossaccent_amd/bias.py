"""Contextual phrase biasing of the CTC prefix beam: the owner of one masr_bias handle (the device trie of a phrase list) and the
reader of a phrase file.  A phrase is a sequence of 1 .. 64 unit ids in [1, C - 2]; mapping text to units is the caller's business."""
import ctypes as C
import math

import numpy as np

from . import _cabi

MAX_PHRASE, MAX_PHRASES = 64, 65536


def read_phrases(path, C_):
    """the phrase file `path`: one phrase per line as space-separated unit ids (the format tools/train_nlm.py reads), blank lines skipped ->
    list of id lists.  ValueError with the line number for anything that is no id in [1, C_ - 2], a phrase above 64 ids or a repeated phrase"""
    C_ = int(C_)
    bad = lambda no, why: ValueError(f"{path}:{no}: {why}")  # noqa: E731
    out, seen = [], set()
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            words = line.split()
            if not words:
                continue
            try:
                ids = tuple(int(w) for w in words)
            except ValueError:
                raise bad(no, f"a phrase is a list of unit ids, got {line.strip()!r}") from None
            if any(not 1 <= i <= C_ - 2 for i in ids):
                raise bad(no, f"unit ids must lie in [1, {C_ - 2}]")
            if len(ids) > MAX_PHRASE:
                raise bad(no, f"a phrase holds at most {MAX_PHRASE} ids, got {len(ids)}")
            if ids in seen:
                raise bad(no, "duplicate phrase")
            seen.add(ids)
            out.append(list(ids))
    if not out:
        raise ValueError(f"{path}: no phrase")
    if len(out) > MAX_PHRASES:
        raise ValueError(f"{path}: at most {MAX_PHRASES} phrases, got {len(out)}")
    return out


def check_bias_args(bias, bias_w):
    """what the biased searches vet on the Python side -> bias_w as a float"""
    bias_w = float(bias_w)
    if not (math.isfinite(bias_w) and bias_w >= 0.0):
        raise ValueError(f"bias_w must be finite and >= 0, got {bias_w}")
    if not isinstance(bias, ContextBias) or bias.h is None:
        raise ValueError("bias must be a live ContextBias")
    return bias_w


class ContextBias:
    """Owner of one masr_bias handle (the device trie of the phrase list `phrases`, a sequence of id sequences over C_ classes); destroys it
    with itself.  What masr_bias_create refuses raises MasrError with its message."""

    def __init__(self, C_, phrases):
        self.h = None
        self._l = _cabi.lib()
        phrases = [[int(t) for t in p] for p in phrases]
        off = np.zeros(len(phrases) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in phrases])
        tok = np.ascontiguousarray([t for p in phrases for t in p] or [0], dtype=np.int32)
        self.C, self.phrases = int(C_), len(phrases)
        h = self._l.masr_bias_create(self.C, self.phrases, tok.ctypes.data, off.ctypes.data)
        if not h:
            raise _cabi.MasrError(f"masr_bias_create failed: {self._l.masr_last_error().decode()}")
        self.h = C.c_void_p(h)

    @classmethod
    def from_file(cls, path, C_):
        """the phrase file `path` (read_phrases) over C_ classes"""
        return cls(C_, read_phrases(path, C_))

    @property
    def bytes(self):
        return int(self._l.masr_bias_bytes(self.h))

    @property
    def nodes(self):
        return int(self._l.masr_bias_nodes(self.h))

    def close(self):
        if self.h is not None:
            self._l.masr_bias_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
