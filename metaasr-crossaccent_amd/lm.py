"""Backoff n-gram language models for shallow fusion (`--decode_mode lm_beam`): a reader of plain-text ARPA files over the
model's output units and the owner of the device tables (include/masr.h masr_lm_create).  The LM's ids are the model's: <s> = sos,
</s> = eos, a unit string = its index in load_units' list."""
import ctypes as C
import math
import re
from types import SimpleNamespace

import numpy as np

from . import _cabi
from .marcos import EOS_SYMBOL, SOS_SYMBOL
from .monitor import logger

MAX_ORDER = 4
UNK_SYMBOL = '<unk>'
_LN10 = math.log(10.0)


def _nat(x):
    """an ARPA log10 value as the natural-log fp32 the tables hold"""
    return np.float32(np.float64(x) * _LN10)


def read_arpa(path, unit2id, sos_id, eos_id):
    """Plain-text ARPA (\\data\\, `ngram n=count`, \\n-grams: sections, \\end\\) -> SimpleNamespace(order, C, counts, grams, logp, backoff,
    dropped): per order n, grams[n - 1] int32 [count][n], logp / backoff fp32 [count] in natural log (float32(float64(x) * ln 10)).
    Words are unit strings (unit2id); <s> -> sos_id, </s> -> eos_id; C = eos_id + 1.  Order 1 comes out dense: a class without a unigram gets
    <unk>'s logp with backoff 0 (ValueError when the file has no <unk>).  An n-gram of order >= 2 with a word that is no unit is dropped and
    counted (one log line).  A malformed line, a count mismatch, an order above 4 or a positive value raises ValueError with its line number."""
    C_ = int(eos_id) + 1
    word2id = dict(unit2id)
    word2id[SOS_SYMBOL], word2id[EOS_SYMBOL] = int(sos_id), int(eos_id)

    def bad(no, why):
        return ValueError(f"{path}: line {no}: {why}")

    declared, rows, seen = {}, {}, {}
    unk = None
    section, state, dropped, no = 0, 'start', 0, 0

    def close_section(no):
        if section and len_read[section] != declared[section]:
            raise bad(no, f"count mismatch: \\{section}-grams: holds {len_read[section]} n-grams, the header says {declared[section]}")

    len_read = {}
    with open(path, encoding='utf-8') as f:
        for no, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if state == 'start':
                if line != '\\data\\':
                    raise bad(no, "expected \\data\\")
                state = 'header'
                continue
            if state == 'end':
                raise bad(no, "text behind \\end\\")
            m = re.fullmatch(r'\\(\d+)-grams:', line)
            if m or line == '\\end\\':
                close_section(no)
                if line == '\\end\\':
                    if section != len(declared) or not declared:
                        raise bad(no, f"\\end\\ after {section} of {len(declared)} declared sections")
                    state = 'end'
                    continue
                n = int(m.group(1))
                if n != section + 1 or n not in declared:
                    raise bad(no, f"section \\{n}-grams: out of order or not declared")
                section, state = n, 'grams'
                rows[n], seen[n], len_read[n] = [], set(), 0
                continue
            if state == 'header':
                m = re.fullmatch(r'ngram\s+(\d+)\s*=\s*(\d+)', line)
                if not m:
                    raise bad(no, "malformed header line (expected `ngram n=count`)")
                n, cnt = int(m.group(1)), int(m.group(2))
                if n != len(declared) + 1:
                    raise bad(no, "orders must be declared 1, 2, ... in turn")
                if n > MAX_ORDER:
                    raise bad(no, f"order {n} > {MAX_ORDER} is not supported")
                declared[n] = cnt
                continue
            # an n-gram line: log10 p, n words, and below the highest order optionally log10 backoff
            n = section
            fld = line.split()
            if len(fld) not in (n + 1, n + 2):
                raise bad(no, f"malformed {n}-gram line ({len(fld)} fields)")
            try:
                lp = float(fld[0])
                bo = float(fld[n + 1]) if len(fld) == n + 2 else 0.0
            except ValueError:
                raise bad(no, "malformed number") from None
            if not (math.isfinite(lp) and math.isfinite(bo)):
                raise bad(no, "non-finite value")
            if lp > 0.0 or bo > 0.0:
                raise bad(no, "positive value: log-probabilities and backoff weights must be <= 0")
            len_read[n] += 1
            words = fld[1:n + 1]
            if n == 1 and words[0] == UNK_SYMBOL and UNK_SYMBOL not in word2id:
                unk = _nat(lp)
                continue
            if any(w not in word2id for w in words):
                dropped += n >= 2                               # (a unigram of a word that is no unit is skipped)
                continue
            ids = tuple(word2id[w] for w in words)
            if n > 1 and (int(sos_id) in ids[1:] or int(eos_id) in ids[:-1]):
                raise bad(no, "malformed n-gram: <s> may only come first, </s> only last")
            if ids in seen[n]:
                raise bad(no, "duplicate n-gram")
            seen[n].add(ids)
            rows[n].append((ids, _nat(lp), _nat(bo) if n < len(declared) else np.float32(0.0)))
    if state != 'end':
        raise bad(no, "no \\end\\")
    order = len(declared)
    have = {ids[0] for ids, _, _ in rows[1]}
    missing = [c for c in range(C_) if c not in have]
    if missing:
        if unk is None:
            raise ValueError(f"{path}: {len(missing)} classes have no unigram (first: id {missing[0]}) and the file has no {UNK_SYMBOL} to stand in")
        rows[1] += [((c,), unk, np.float32(0.0)) for c in missing]
    if dropped:
        logger.notice(f"{path}: dropped {dropped} n-grams of order >= 2 that hold a word outside the {C_} output units")
    out = SimpleNamespace(order=order, C=C_, dropped=dropped, grams=[], logp=[], backoff=[], counts=[])
    for n in range(1, order + 1):
        out.grams.append(np.array([ids for ids, _, _ in rows[n]], dtype=np.int32).reshape(-1, n))
        out.logp.append(np.array([lp for _, lp, _ in rows[n]], dtype=np.float32))
        out.backoff.append(np.array([bo for _, _, bo in rows[n]], dtype=np.float32))
        out.counts.append(len(rows[n]))
    return out


class NGramLM:
    """Owner of one masr_lm handle (the device tables of a backoff n-gram model); destroys it with itself.  grams[n - 1] int32 [count][n],
    logp[n - 1] / backoff[n - 1] fp32 [count], natural log, <= 0; what masr_lm_create refuses raises MasrError with its message."""

    def __init__(self, order, C_, grams, logp, backoff):
        self.h = None
        self._l = _cabi.lib()
        order, C_ = int(order), int(C_)
        if not 1 <= order <= MAX_ORDER or not len(grams) == len(logp) == len(backoff) == order:
            raise ValueError(f"need 1 <= order <= {MAX_ORDER} and one array of n-grams, logp and backoff per order")
        g = [np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1, n + 1)) for n, a in enumerate(grams)]
        lp = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in logp]
        bo = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in backoff]
        if any(len(g[n]) != len(lp[n]) or len(g[n]) != len(bo[n]) for n in range(order)):
            raise ValueError("n-grams, logp and backoff of one order must have one length")
        self.order, self.C, self.counts = order, C_, [len(a) for a in g]
        ptrs = lambda arrs: (C.c_void_p * order)(*[a.ctypes.data if a.size else None for a in arrs])  # noqa: E731
        h = self._l.masr_lm_create(order, C_, (C.c_int64 * order)(*self.counts), ptrs(g), ptrs(lp), ptrs(bo))
        if not h:
            raise _cabi.MasrError(f"masr_lm_create failed: {self._l.masr_last_error().decode()}")
        self.h = C.c_void_p(h)

    @classmethod
    def from_arpa(cls, path, id2units, sos_id=None, eos_id=None):
        """the ARPA file `path` over the units id2units (load_units' list: <s> first, </s> last)"""
        sos_id = 0 if sos_id is None else sos_id
        eos_id = len(id2units) - 1 if eos_id is None else eos_id
        a = read_arpa(path, {u: i for i, u in enumerate(id2units)}, sos_id, eos_id)
        lm = cls(a.order, a.C, a.grams, a.logp, a.backoff)
        lm.dropped = a.dropped
        return lm

    @property
    def device_bytes(self):
        return int(self._l.masr_lm_bytes(self.h))

    def close(self):
        if self.h is not None:
            self._l.masr_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
