"""The chunk mask of the encoder's self-attention (include/masr.h masr_chunk_policy) restated for the tests: the visible set, the dynamic
policy's draw (Python ints, the hash of csrc/common.h as tests/specaug_ref.py states it), one attention forward / backward in fp64 with the
empty-row rule, and the oracle's encoder under a chunk.  No GPU, no libmasr."""
import contextlib

import numpy as np
import torch

from oracle import ref_cpu
from specaug_ref import dropout_key, dropout_word, step_seed, uni

SITE = 0x43484E4B


def visible(T, klen, c, left):
    """bool [T, T]: vis[i, j] = query i sees key j under a chunk of c (0: full context) with `left` earlier chunks (-1: all) and klen valid keys"""
    i = np.arange(T)[:, None]
    j = np.arange(T)[None, :]
    vis = np.broadcast_to(j < klen, (T, T)).copy()
    if c > 0:
        ci = i // c
        vis &= j < (ci + 1) * c
        if left >= 0:
            vis &= j >= (ci - left) * c
    return vis


def chunk_draw(seed, step, Tp):
    """the chunk a dynamic policy's training step runs with at the dropout position (seed, step): 0 = full context, else 1..25"""
    if Tp < 2:
        return 0
    w = dropout_word(dropout_key(step_seed(seed, step), SITE), 0)
    r = 1 + uni(w, Tp - 1)
    return 0 if r > Tp // 2 else r % 25 + 1


def attention(q, k, v, dout, klens, c, left, keep=None):
    """q, k, v, dout [B, T, H, hd] (any float dtype), klens [B] or None, keep [B, H, T, T] keep-scales of the probabilities or None ->
    dict of fp64 tensors: o, dq, dk, dv [B, T, H, hd], lse [B, H, T], and empty bool [B, T] (rows without a visible key: o = lse = 0 there and
    they pass 0 to every gradient)."""
    q, k, v, dout = (torch.as_tensor(t).detach().cpu().double().permute(0, 2, 1, 3) for t in (q, k, v, dout))     # [B, H, T, hd]
    B, H, T, hd = q.shape
    klens = [T] * B if klens is None else [int(x) for x in klens]
    vis = torch.from_numpy(np.stack([visible(T, klens[b], c, left) for b in range(B)]))[:, None]                 # [B, 1, T, T]
    empty = ~vis.any(-1)                                                                                          # [B, 1, T]
    scale = 1.0 / hd ** 0.5
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(empty[..., None], torch.zeros_like(m), m)
    e = torch.exp(s - m)                                                                                          # exp(-inf) = 0
    l = e.sum(-1, keepdim=True)
    p = torch.where(empty[..., None], torch.zeros_like(e), e / torch.where(empty[..., None], torch.ones_like(l), l))
    lse = torch.where(empty, torch.zeros_like(m[..., 0]), m[..., 0] + torch.log(torch.where(empty[..., None], torch.ones_like(l), l))[..., 0])
    pm = p if keep is None else p * torch.as_tensor(keep).detach().cpu().double()
    o = pm @ v
    dpm = dout @ v.transpose(-1, -2)
    dp = dpm if keep is None else dpm * torch.as_tensor(keep).detach().cpu().double()
    delta = (dout * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    out = {"o": o, "dq": ds @ k * scale, "dk": ds.transpose(-1, -2) @ q * scale, "dv": pm.transpose(-1, -2) @ dout}
    out = {n: t.permute(0, 2, 1, 3).contiguous() for n, t in out.items()}
    out["lse"] = lse.expand(B, H, T).contiguous()
    out["empty"] = empty[:, 0]
    return out


def encoder_forward_chunk(p, cfg, x, pad_mask, c, left):
    """ref_cpu.encoder_forward with the chunk mask on every layer's self-attention.  x [T, B, E], pad_mask bool [B, T] (True = padding).  The
    key-padding mask and the chunk mask go into _mha as ONE additive mask [B, 1, T, T]; a row without a visible key attends to nothing: its
    attention output is zero, so the block's output there is the out-projection's bias (WeNet zeroes such rows behind its softmax)."""
    T, B, _ = x.shape
    H = cfg["nheads"]
    klens = (~pad_mask).sum(-1)
    vis = torch.from_numpy(np.stack([visible(T, int(klens[b]), c, left) for b in range(B)]))                      # [B, T, T]
    empty = ~vis.any(-1)                                                                                          # [B, T]
    add = torch.zeros(B, 1, T, T, dtype=x.dtype).masked_fill(~(vis | empty[..., None])[:, None], float("-inf"))
    for l in range(cfg["encoder"]["nlayers"]):
        pre = f"encoder.layers.{l}"
        a = ref_cpu._mha(p, f"{pre}.self_attn", x, x, H, attn_mask=add)
        a = torch.where(empty.t()[:, :, None], p[f"{pre}.self_attn.out_proj.bias"].expand_as(a), a)
        x = ref_cpu._ln(p, f"{pre}.norm1", x + a)
        x = ref_cpu._ln(p, f"{pre}.norm2", x + ref_cpu._ffn(p, pre, x))
    return ref_cpu._ln(p, "encoder.norm", x)


@contextlib.contextmanager
def chunked_oracle(c, left=-1):
    """inside: ref_cpu.encoder_forward is the chunked encoder, so ref_cpu.model_forward / run_batch_train / recog_greedy and tests/hybrid_ref.py
    run under the chunk unchanged"""
    prev = ref_cpu.encoder_forward
    ref_cpu.encoder_forward = lambda p, cfg, x, pad_mask: encoder_forward_chunk(p, cfg, x, pad_mask, c, left)
    try:
        yield
    finally:
        ref_cpu.encoder_forward = prev
