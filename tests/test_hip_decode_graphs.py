"""The cached step graphs of the three decoders (masr_recog, masr_recog_beam, masr_recog_beam_ctc): capture, replay, re-capture on a
new key, and the three caches side by side.  MasrEngine.stream() hands the library torch's current stream; on the default stream that
is the NULL stream, where the decoders launch every step directly -- so the graph paths are reached on a side stream only.

One interleaved sequence of calls runs three times: on the default stream (direct launches; it also grows the workspace to its final
size, so the pointer part of the graph keys stays put afterwards), on a side stream (graphs), and on the side stream with
MASR_RECOG_NO_GRAPH set (direct launches again; the library reads the variable on every call).  A graph replays the launches of the
direct path with the same arguments, so every call must give the same tokens and the same score bits in all three runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from oracle.make_goldens import TINY, synth_batch  # noqa: E402
from test_hip_joint_beam import joint_engine, joint_state_dict  # noqa: E402

W1, W2 = (0.5, 0.5), (0.7, 0.3)
# (decoder, batch, K, joint weights).  Batch "a": B = 3, T = 48, 12 steps; batch "b": B = 2, T = 60, 15 steps.
CALLS = (
    [("greedy", "a", 0, None), ("beam", "a", 3, None), ("joint", "a", 3, W1)] * 2 +      # capture, then the same call again: a cache hit
    [("greedy", "b", 0, None), ("joint", "b", 3, W1), ("beam", "b", 3, None),             # another B: each decoder re-captures
     ("beam", "b", 2, None), ("joint", "b", 2, W1),                                       # another K
     ("joint", "b", 2, W2),                                                               # other joint weights
     ("greedy", "a", 0, None), ("beam", "a", 3, None), ("joint", "a", 3, W1),             # back to each decoder's first shape
     ("joint", "a", 3, W2)]
)


def _run(eng, batches):
    out = []
    for kind, name, K, w in CALLS:
        xs, il = batches[name]
        if kind == "greedy":
            out.append((eng.recog(xs, il).cpu().T.tolist(), None))
        elif kind == "beam":
            out.append(eng.recog_beam(xs, il, K))
        else:
            out.append(eng.recog_beam(xs, il, K, att_weight=w[0], ctc_weight=w[1]))
    return out


def test_decode_graphs_equal_direct_launches(monkeypatch):
    monkeypatch.delenv("MASR_RECOG_NO_GRAPH", raising=False)
    eng = joint_engine(TINY, joint_state_dict(TINY, 7))
    batches = {}
    for name, seed, ilens in (("a", 12, [48, 48, 44]), ("b", 13, [37, 60])):
        xs, il, _, _ = synth_batch(seed, ilens, [3] * len(ilens))
        batches[name] = (xs.cuda(), il)
    assert torch.cuda.current_stream().cuda_stream == 0       # the NULL stream: direct launches
    direct = _run(eng, batches)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream != 0
        graphs = _run(eng, batches)
    side.synchronize()
    monkeypatch.setenv("MASR_RECOG_NO_GRAPH", "1")
    with torch.cuda.stream(side):
        no_graph = _run(eng, batches)
    side.synchronize()
    for call, (t0, s0), (t1, s1), (t2, s2) in zip(CALLS, direct, graphs, no_graph):
        assert t1 == t0 and t2 == t0, call
        if s0 is not None:
            assert not torch.isnan(s0).any(), call
            assert torch.equal(s1, s0) and torch.equal(s2, s0), (call, s0, s1, s2)
    # the sequence is not trivial: the decoders, the beam widths and the weights do not all give one answer
    assert len({repr(t) for t, _ in direct}) > 3
