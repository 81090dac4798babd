"""CTC prefix beam decoding (masr_ctc_beam_search) beside the forward alone, ms per decode for K = 1, 4, 10, 20, at
  - the BLSTM bench shape of tools/bench_blstm.py (config/blstm/mono-test.yaml, B 8 x 400 frames): BlstmEngine.forward vs .ctc_beam on
    the batch, and the same 8 utterances one by one (what MonoBLSTM.ctc_beam_decode and hence the Tester run)
  - the hkust hybrid geometry (B 16, T 1000, T' 250, C 367): MasrEngine.recog_ctc_beam; "forward" is the same call at K = 1 minus the
    search, measured as the search alone on logits of the same shape (masr_ctc_beam_search on random logits, [16][250][367]).
Times include the copy of the N-best lists to the host.  For the per-launch times of ctc_beam_frames_kernel / ctc_beam_sweep_kernel run
`rocprofv3 --kernel-trace --stats -- python tools/bench_ctc_beam.py` and read the two kernels in the stats.
usage: python tools/bench_ctc_beam.py"""
import ctypes as C
import json
import sys

import torch

sys.path.insert(0, ".")
import masr_amd  # noqa
from masr_amd._cabi import lib
from masr_amd.blstm_engine import BlstmEngine
from masr_amd.blstm_engine import reference_init_state_dict as blstm_init
from decode_bench import hkust_engine, timed as timed_on

KS = (1, 4, 10, 20)


def timed(fn, n=3):
    return round(timed_on(fn, n)[0], 3)


def search_alone(B, Tp, Cn, K, scale):
    l = lib()
    z = torch.randn(B, Tp, Cn, device="cuda") * scale
    lens = torch.full((B,), Tp, dtype=torch.int32, device="cuda")
    nb = int(l.masr_ctc_beam_work_bytes(B, Tp, Cn, K))
    work = torch.empty(nb, dtype=torch.uint8, device="cuda")
    tok = torch.empty(B, 1, Tp, dtype=torch.int32, device="cuda")
    ln = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, 1, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731

    def run():
        rc = l.masr_ctc_beam_search(p(z), Cn, p(lens), B, Tp, Cn, K, 1, 0, Cn - 1, p(work), nb, p(tok), p(ln), p(sc),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, l.masr_last_error()
    return timed(run, 5)


def main():
    torch.manual_seed(531)
    res = {}
    cfg = {"encoder": {"idim": 83, "enc_dim": 360, "proj_dim": 360, "odim": 360, "sample_rate": "1_1_1", "dropout": "0_0_0"}}
    eng = BlstmEngine(cfg, 367)
    eng.load_state_dict(blstm_init(cfg, 367))
    B, T = 8, 400
    xs = torch.randn(B, T, 83, device="cuda")
    il = torch.full((B,), T, dtype=torch.int64)
    r = {"B": B, "T": T, "Tp": (T + 3) // 4, "forward_ms": timed(lambda: eng.forward(xs, il))}
    for K in KS:
        r[f"ctc_beam_K{K}_ms"] = timed(lambda: eng.ctc_beam(xs, il, K))
        r[f"search_alone_K{K}_ms"] = search_alone(B, (T + 3) // 4, 367, K, 1.0)
        # the Tester's path (MonoBLSTM.ctc_beam_decode): every utterance alone, B forwards and B one-workgroup sweeps
        r[f"per_utterance_K{K}_ms"] = timed(lambda: [eng.ctc_beam(xs[b:b + 1], il[b:b + 1], K) for b in range(B)])
    res["blstm"] = r
    print(json.dumps({"blstm": r}), flush=True)
    del eng
    eng = hkust_engine(ctc=True, seed=None)                     # (the seed of this process was set above)
    B, T = 16, 1000
    xs = torch.randn(B, T, 80, device="cuda")
    il = torch.full((B,), T, dtype=torch.int64)
    r = {"B": B, "T": T, "Tp": T // 4}
    for K in KS:
        r[f"ctc_beam_K{K}_ms"] = timed(lambda: eng.recog_ctc_beam(xs, il, K))
        r[f"search_alone_K{K}_ms"] = search_alone(B, T // 4, 367, K, 1.0)
    r["encoder_and_head_ms"] = round(r["ctc_beam_K1_ms"] - r["search_alone_K1_ms"], 3)
    res["hybrid"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
