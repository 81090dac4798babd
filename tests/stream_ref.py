"""Restatement of the streaming first pass (include/masr.h masr_stream_*) on the CPU oracle, in whatever dtype the parameters
have (the tests use fp64).  Four parts:

  1. the windowed front-end: chunk n = encoder frames [s, e) comes from ref_cpu.extract_feat on the input window
     [max(0, 4s - halo), min(T, 4e + halo)) -- halo 8 is exact (encoder frame t reads the input frames 4t - 6 .. 4t + 9), halo 4 is not;
  2. the per-layer K / V caches, appended for every utterance, padding rows included;
  3. the key range [lo, min(e, klen_b)) of every row of the step, with the empty-row rule (no key: the block's output is the out-projection's
     bias);
  4. greedy CTC with the carried {previous arg-max, len}.

A helper module like chunk_ref.py: no fixtures, no tests."""
import math

import torch

import hybrid_ref
from oracle import ref_cpu


def best_path(am, klen):
    """tokens and their frames of the arg-max sequence am[:klen]: repeats merged, blanks (0) dropped"""
    tok, frm, prev = [], [], 0
    for t, a in enumerate(am[:klen]):
        if a != 0 and a != prev:
            tok.append(int(a)); frm.append(t)
        prev = a
    return tok, frm


class StreamRef:
    def __init__(self, p, cfg, B, c, left, halo=8):
        assert c > 0 and left >= -1 and halo % 4 == 0
        self.p, self.cfg, self.B, self.c, self.left, self.halo = p, cfg, B, c, left, halo
        self.x = None                                    # the buffered input [B, recv, D], zero behind an utterance's end
        self.len = [0] * B; self.ended = [False] * B; self.last = False
        self.emitted = 0
        nl = cfg["encoder"]["nlayers"]
        self.K = [None] * nl; self.V = [None] * nl       # [B, frames, E] per layer
        self.memory, self.logits = [], []                # per step [B, R, E] / [B, R, odim]
        self.prev = [0] * B; self.tokens = [[] for _ in range(B)]; self.frames = [[] for _ in range(B)]

    # ---- 1. the windowed front-end
    def _front_end(self, s, e):
        T = self.x.shape[1]
        w0, w1 = max(0, 4 * s - self.halo), min(T, 4 * e + self.halo)
        v, _ = ref_cpu.extract_feat(self.p, self.x[:, w0:w1], torch.full((self.B,), w1 - w0))
        off = s - w0 // 4
        pe = self.p["pos_encoder.pe"].reshape(-1, v.shape[-1])[s:e].to(v.dtype)
        return v[:, off:off + e - s] + pe

    # ---- 2. + 3. one encoder layer on the step's rows against its cache
    def _attention(self, l, x, s, e, lo):
        p, H = self.p, self.cfg["nheads"]
        pre = f"encoder.layers.{l}.self_attn"
        B, R, E = x.shape
        hd = E // H
        W, b = p[f"{pre}.in_proj_weight"], p[f"{pre}.in_proj_bias"]
        q, k, v = ((x @ W[i * E:(i + 1) * E].t() + b[i * E:(i + 1) * E]) for i in range(3))
        self.K[l] = k if self.K[l] is None else torch.cat([self.K[l], k], 1)
        self.V[l] = v if self.V[l] is None else torch.cat([self.V[l], v], 1)
        bias = p[f"{pre}.out_proj.bias"]
        out = torch.empty_like(x)
        for u in range(B):
            hi = min(e, self.len[u] // 4)
            if hi <= lo:                                 # the empty-row rule
                out[u] = bias
                continue
            qh = q[u].reshape(R, H, hd).transpose(0, 1)
            kh = self.K[l][u, lo:hi].reshape(hi - lo, H, hd).transpose(0, 1)
            vh = self.V[l][u, lo:hi].reshape(hi - lo, H, hd).transpose(0, 1)
            a = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd), -1)
            out[u] = (a @ vh).transpose(0, 1).reshape(R, E) @ p[f"{pre}.out_proj.weight"].t() + bias
        return out

    def _step(self, s, e):
        n = s // self.c
        lo = 0 if self.left < 0 else max(0, (n - self.left) * self.c)
        x = self._front_end(s, e)
        for l in range(self.cfg["encoder"]["nlayers"]):
            pre = f"encoder.layers.{l}"
            x = ref_cpu._ln(self.p, f"{pre}.norm1", x + self._attention(l, x, s, e, lo))
            x = ref_cpu._ln(self.p, f"{pre}.norm2", x + ref_cpu._ffn(self.p, pre, x))
        mem = ref_cpu._ln(self.p, "encoder.norm", x)
        z = mem @ self.p[hybrid_ref.HEAD[0]].t() + self.p[hybrid_ref.HEAD[1]]
        self.memory.append(mem); self.logits.append(z)
        # ---- 4. greedy with carry
        am = z.argmax(-1)
        for u in range(self.B):
            for i in range(e - s):
                t = s + i
                if t >= self.len[u] // 4:
                    break
                a = int(am[u, i])
                if a != 0 and a != self.prev[u]:
                    self.tokens[u].append(a); self.frames[u].append(t)
                self.prev[u] = a

    def feed(self, xs, valid=None, last=False):
        """the next piece xs [B, n, D]; valid[b] < n ends utterance b.  -> encoder frames emitted so far"""
        assert not self.last, "a piece after the last"
        n = xs.shape[1]
        valid = [n] * self.B if valid is None else [int(v) for v in valid]
        for u, v in enumerate(valid):
            if not 0 <= v <= n:
                raise ValueError("valid[b] must lie in [0, n]")
            if self.ended[u] and v != 0:
                raise ValueError("an utterance that has ended must be given valid[b] = 0")
        xs = xs.clone()
        for u, v in enumerate(valid):
            xs[u, v:] = 0                                # the zero fill behind an utterance's end
            self.len[u] += v
            if v < n or last:
                self.ended[u] = True
        self.x = xs if self.x is None else torch.cat([self.x, xs], 1)
        self.last = last
        recv = self.x.shape[1]
        while True:
            s, e = self.emitted, self.emitted + self.c
            if last:
                if s >= recv // 4:
                    break
                e = min(e, recv // 4)
            elif recv < 4 * e + 8:
                break
            self._step(s, e)
            self.emitted = e
        return self.emitted

    def result(self):
        """memory [B, frames, E], head logits [B, frames, odim]"""
        return torch.cat(self.memory, 1), torch.cat(self.logits, 1)


def stream(p, cfg, xs, ilens, c, left, piece, halo=8):
    """the padded batch xs [B, T, D] streamed in pieces of `piece` frames, valid derived from ilens -> the StreamRef after the last piece"""
    B, T = xs.shape[:2]
    st = StreamRef(p, cfg, B, c, left, halo)
    for t0 in range(0, T, piece):
        t1 = min(T, t0 + piece)
        st.feed(xs[:, t0:t1], [max(0, min(int(l), t1) - t0) for l in ilens], last=t1 == T)
    return st


def full_pass(p, cfg, xs, ilens, c, left):
    """the chunk-masked full pass on the padded batch: memory [B, T / 4, E], head logits [B, T / 4, odim], enc_lens"""
    import chunk_ref
    enc, enc_lens = ref_cpu.extract_feat(p, xs, torch.as_tensor(ilens))
    enc = enc.transpose(0, 1)
    enc = enc + p["pos_encoder.pe"].reshape(-1, 1, enc.shape[-1])[:enc.shape[0]].to(enc.dtype)
    mem = chunk_ref.encoder_forward_chunk(p, cfg, enc, ref_cpu.make_bool_pad_mask(enc_lens), c, left).transpose(0, 1)
    return mem, mem @ p[hybrid_ref.HEAD[0]].t() + p[hybrid_ref.HEAD[1]], enc_lens.tolist()
