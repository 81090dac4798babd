"""LSTM language models for shallow fusion (`--decode_mode nlm_beam`): the reader of a torch checkpoint of
Embedding -> LSTM -> Linear over the model's output units and the owner of the device weights (include/masr.h masr_nlm_create).  The LM's ids
are the model's; its start token is the model's sos (0) or, for LMs trained with sos = eos, the last class."""
import ctypes as C

import numpy as np
import torch

from . import _cabi

MAX_LAYERS = 4
_PER_LAYER = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _f32(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().to(torch.float32).cpu().numpy())


def parse_state_dict(sd):
    """the weights of either accepted key layout -> dict(embed [C, E], w_ih / w_hh / b_ih / b_hh (lists, one entry per layer), lo_w [C, H],
    lo_b [C]) as contiguous fp32 numpy arrays.  Layouts: this project's (embed.weight, rnn.weight_ih_l{k}, rnn.weight_hh_l{k},
    rnn.bias_ih_l{k}, rnn.bias_hh_l{k}, lo.weight, lo.bias; at top level or under "model") and the per-layer LSTMCell one
    (predictor.embed.weight, predictor.rnn.{k}.weight_ih / weight_hh / bias_ih / bias_hh, predictor.lo.weight / bias).  Anything else raises
    ValueError naming the missing keys."""
    if not isinstance(sd, dict):
        raise ValueError(f"an LSTM LM checkpoint must be a dict of tensors, got {type(sd).__name__}")
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    if any(str(k).startswith("predictor.") for k in sd):
        layer_key = lambda k, n: f"predictor.rnn.{k}.{n}"  # noqa: E731
        head = {"embed": "predictor.embed.weight", "lo_w": "predictor.lo.weight", "lo_b": "predictor.lo.bias"}
    else:
        layer_key = lambda k, n: f"rnn.{n}_l{k}"  # noqa: E731
        head = {"embed": "embed.weight", "lo_w": "lo.weight", "lo_b": "lo.bias"}
    L = 0
    while L < MAX_LAYERS + 1 and any(layer_key(L, n) in sd for n in _PER_LAYER):
        L += 1
    missing = [k for k in head.values() if k not in sd]
    missing += [layer_key(k, n) for k in range(max(L, 1)) for n in _PER_LAYER if layer_key(k, n) not in sd]
    if missing:
        raise ValueError(f"not an LSTM LM checkpoint: missing keys {missing}")
    if L > MAX_LAYERS:
        raise ValueError(f"an LSTM LM of more than {MAX_LAYERS} layers is not supported")
    out = {name: _f32(sd[key]) for name, key in head.items()}
    for short, n in zip(("w_ih", "w_hh", "b_ih", "b_hh"), _PER_LAYER):
        out[short] = [_f32(sd[layer_key(k, n)]) for k in range(L)]
    C_, E = out["embed"].shape
    H = out["w_hh"][0].shape[1]
    want = {"lo_w": (C_, H), "lo_b": (C_,)}
    for k in range(L):
        want.update({f"w_ih[{k}]": (4 * H, H if k else E), f"w_hh[{k}]": (4 * H, H), f"b_ih[{k}]": (4 * H,), f"b_hh[{k}]": (4 * H,)})
    for name, shape in want.items():
        a = out[name] if "[" not in name else out[name[:4]][int(name[5:-1])]
        if a.shape != shape:
            raise ValueError(f"LSTM LM checkpoint: {name} has shape {a.shape}, expected {shape}")
    return out


class LstmLM:
    """Owner of one masr_nlm handle (the device weights of an Embedding -> LSTM -> Linear language model); destroys it with itself.  What
    masr_nlm_create refuses raises MasrError with its message."""

    def __init__(self, embed, w_ih, w_hh, b_ih, b_hh, lo_w, lo_b, start_id=0):
        self.h = None
        self._l = _cabi.lib()
        embed, lo_w, lo_b = _f32(embed), _f32(lo_w), _f32(lo_b)
        w_ih, w_hh, b_ih, b_hh = ([_f32(a) for a in arrs] for arrs in (w_ih, w_hh, b_ih, b_hh))
        L = len(w_ih)
        if not (1 <= L <= MAX_LAYERS and len(w_hh) == len(b_ih) == len(b_hh) == L):
            raise ValueError(f"need 1 .. {MAX_LAYERS} layers and one w_ih, w_hh, b_ih and b_hh per layer")
        self.C, self.E = (int(n) for n in embed.shape)
        self.H, self.L, self.start_id = int(w_hh[0].shape[1]), L, int(start_id)
        ptrs = lambda arrs: (C.c_void_p * L)(*[a.ctypes.data for a in arrs])  # noqa: E731
        h = self._l.masr_nlm_create(self.C, self.E, self.H, L, self.start_id, embed.ctypes.data, ptrs(w_ih), ptrs(w_hh), ptrs(b_ih), ptrs(b_hh),
                                    lo_w.ctypes.data, lo_b.ctypes.data)
        if not h:
            raise _cabi.MasrError(f"masr_nlm_create failed: {self._l.masr_last_error().decode()}")
        self.h = C.c_void_p(h)

    @classmethod
    def from_state_dict(cls, sd, start_id=0):
        return cls(**parse_state_dict(sd), start_id=start_id)

    @classmethod
    def load(cls, path, start_id=0):
        """a checkpoint written by torch.save (tools/train_nlm.py writes one)"""
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), start_id=start_id)

    @property
    def device_bytes(self):
        return int(self._l.masr_nlm_bytes(self.h))

    def score(self, token_lists, device="cuda:0"):
        """the teacher-forced log-probability of each token list followed by eos (masr_nlm_score) -> fp32 tensor [R] on the host"""
        R = len(token_lists)
        ld = max([len(t) for t in token_lists] + [0])
        tok = torch.zeros(R, max(ld, 1), dtype=torch.int32)
        for r, t in enumerate(token_lists):
            tok[r, :len(t)] = torch.as_tensor(list(t), dtype=torch.int32)
        tok = tok[:, :ld].contiguous() if ld else tok
        dev = torch.device(device)
        tok_d, lens_d = tok.to(dev), torch.tensor([len(t) for t in token_lists], dtype=torch.int32, device=dev)
        need = int(self._l.masr_nlm_score_work_bytes(self.h, R, ld))
        _cabi.check(need if need < 0 else 0, "masr_nlm_score_work_bytes")
        work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = (work.data_ptr() + 255) // 256 * 256
        out = torch.empty(R, dtype=torch.float32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(self._l.masr_nlm_score(self.h, C.c_void_p(tok_d.data_ptr()), C.c_void_p(lens_d.data_ptr()), R, ld, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(base), need, stream), "masr_nlm_score")
        return out.cpu()

    def close(self):
        if self.h is not None:
            self._l.masr_nlm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
