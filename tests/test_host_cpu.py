"""CPU tests of the host mirror (no GPU): data path vs goldens captured from the reference, Noam schedule,
init replay, masks, metric, parameter table, and that libmasr.so exports every symbol of include/masr.h and include/masr_test.h."""
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import masr_amd
from masr_amd import _cabi
from masr_amd.io.dataset import BucketSampler, DataContainer, collate_fn, get_loader
from masr_amd.model import reference_init_state_dict
from masr_amd.monitor.metric import levenshtein
from masr_amd.optimizer import TransformerOptimizer
from oracle.make_goldens import TINY, flat_checks, write_toy_shard

REPO = Path(__file__).resolve().parents[1]
HK = dict(idim=83, nheads=8, d_model=512, d_inner=2048, dropout=0.1, pos_dropout=0.1, tgt_share_weight=1,
          encoder=dict(nlayers=2), decoder=dict(nlayers=4))


def test_cabi_exports_every_declared_symbol():
    """include/masr.h (operator API) + include/masr_test.h (test-only entry points) <-> libmasr.so <-> ctypes table (load + symbol
    lookup only, no compute); the operator header holds no test entry point and the test header nothing else."""
    api = set(re.findall(r"\b(masr_[a-z0-9_]+)\s*\(", (REPO / "include" / "masr.h").read_text()))
    tst = set(re.findall(r"\b(masr_[a-z0-9_]+)\s*\(", (REPO / "include" / "masr_test.h").read_text()))
    assert not any(n.startswith("masr_test_") for n in api), sorted(n for n in api if n.startswith("masr_test_"))
    assert all(n.startswith("masr_test_") for n in tst), sorted(n for n in tst if not n.startswith("masr_test_"))
    declared = api | tst
    lib = ctypes.CDLL(str(_cabi.LIB_PATH))
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/*.h but not exported"
    assert declared == set(_cabi.EXPORTS), declared ^ set(_cabi.EXPORTS)
    assert _cabi.lib().masr_version() >= 1


def test_param_table_matches_reference_state_dict(golden_dir):
    g = np.load(golden_dir / "init.npz")
    l = _cabi.lib()
    for tag, cfg in (("tiny", TINY), ("hkust", HK)):
        c = _cabi.MasrConfig(cfg["idim"], 367, cfg["d_model"], cfg["nheads"], cfg["d_inner"], cfg["encoder"]["nlayers"],
                             cfg["decoder"]["nlayers"], 1, 0.0, 0.0, 0.0)
        h = l.masr_create(ctypes.byref(c))
        names = []
        name = ctypes.create_string_buffer(256); shape = (ctypes.c_int64 * 4)(); nd = ctypes.c_int(); off = ctypes.c_int64()
        for i in range(l.masr_param_count(h)):
            assert l.masr_param_info(h, i, name, 256, shape, ctypes.byref(nd), ctypes.byref(off)) == 0
            names.append(name.value.decode())
        ref = [k for k in g[f"{tag}/keys"] if k not in ("pos_encoder.pe", "pre_embed.weight")]
        assert names == ref
        assert int(l.masr_param_numel(h)) == int(g[f"{tag}/nparams"])
        l.masr_destroy(h)


@pytest.mark.parametrize("tag", ["tiny", "hkust"])
def test_init_replay_matches_reference_seed_531(golden_dir, tag):
    g = np.load(golden_dir / "init.npz")
    torch.manual_seed(531)
    sd = reference_init_state_dict(TINY if tag == "tiny" else HK, 367)
    for n, t in sd.items():
        np.testing.assert_allclose(flat_checks(t), g[f"{tag}/fp/{n}"], rtol=1e-6, atol=1e-9, err_msg=n)


def test_noam_schedule(golden_dir):
    """(the reference's mask helpers have no host-side mirror in the product: key-padding and causal masks are applied analytically
    inside attention.hip -- tests/test_hip_kernels.py::test_attention; the oracle's own are pinned in tests/test_oracle_golden.py)"""
    g = np.load(golden_dir / "masks_noam.npz")

    class _Opt:
        param_groups = [{"lr": 0.0}]
        def step(self): pass
        def zero_grad(self): pass
    for key, (k, d, w) in {"noam_lr_512_25000": (1.0, 512, 25000), "noam_lr_64_4_k0.7": (0.7, 64, 4)}.items():
        o = TransformerOptimizer(_Opt(), k, d, w)
        lrs = []
        for _ in range(12):
            o.step()
            lrs.append(o.lr)
        np.testing.assert_allclose(lrs, g[key], rtol=1e-12)


def test_bucket_sampler_matches_reference(golden_dir):
    g = np.load(golden_dir / "bucket_sampler.npz")
    random.seed(531); np.random.seed(531)
    s = BucketSampler(g["ilens"], min_ilen=10, max_ilen=50, half_batch_ilen=30, batch_size=4)
    for ep in range(2):
        batches = list(iter(s))
        np.testing.assert_array_equal(np.array([i for b in batches for i in b]), g[f"epoch{ep}_flat"])
        np.testing.assert_array_equal(np.array([len(b) for b in batches]), g[f"epoch{ep}_sizes"])
    assert len(s) == int(g["len"])


def test_data_container_replays_reference_batches(golden_dir, tmp_path):
    """DataContainer + get_loader + BucketSampler + collate_fn feed the FOMAML loop the same batches, in the same
    order, as the reference did in the golden run (2 accents, meta_k 2, 2 meta-steps)."""
    g = np.load(golden_dir / "fomaml_toy.npz")
    for ai, a in enumerate(["african", "australia"]):
        write_toy_shard(tmp_path, a, "train", 16, seed=100 + ai)
        write_toy_shard(tmp_path, a, "dev", 4, seed=200 + ai)
    random.seed(531); np.random.seed(531)
    dc = DataContainer([tmp_path / "african", tmp_path / "australia"], batch_size=4, dev_batch_size=4, is_memmap=True,
                       is_bucket=True, min_ilen=10, max_ilen=50, half_batch_ilen=30)
    task_ids = [0, 1]
    call = 0
    for _ in range(2):
        random.shuffle(task_ids)
        for ai in task_ids[:2]:
            for acc, (x, il, ys, ol) in dc.get_item(ai, 2) + dc.get_item(ai):
                assert int(acc) == int(g[f"call{call}/accent"])
                np.testing.assert_array_equal(il.numpy(), g[f"call{call}/ilens"])
                np.testing.assert_array_equal(ol.numpy(), g[f"call{call}/olens"])
                np.testing.assert_array_equal(np.concatenate([y.numpy() for y in ys]), g[f"call{call}/ys"])
                np.testing.assert_allclose(flat_checks(x), g[f"call{call}/x_fp"], rtol=1e-6)
                call += 1
    assert call == int(g["n_calls"])


def test_collate_sorts_and_pads():
    items = [{"feat": torch.ones(n, 3) * n, "ilen": torch.tensor(n), "label": torch.arange(n % 4 + 1), "olen": torch.tensor(n % 4 + 1)}
             for n in (5, 9, 7)]
    xs, il, ys, ol = collate_fn(items)
    assert il.tolist() == [9, 7, 5] and xs.shape == (3, 9, 3)
    assert torch.all(xs[1, 7:] == 0) and torch.all(xs[1, :7] == 7)
    assert [len(y) for y in ys] == ol.tolist()


def test_edge_buckets_are_dropped_like_the_reference():
    # utterances at/below min_ilen or above max_ilen-2 fall in the first/last bin, which the reference never iterates
    random.seed(0); np.random.seed(0)
    s = BucketSampler(np.array([10, 11, 48, 49, 50, 200]), min_ilen=10, max_ilen=50, half_batch_ilen=30, batch_size=4)
    kept = sorted(i for b in s for i in b)
    assert kept == [1, 2]


def test_levenshtein():
    assert levenshtein("kitten", "sitting") == 3
    assert levenshtein([], [1, 2]) == 2
    assert levenshtein(["a", "b"], ["a", "b"]) == 0
    assert levenshtein("abc", "") == 3 and levenshtein("", "") == 0

    def dp(a, b):                                    # textbook DP as the checker
        prev = list(range(len(b) + 1))
        for i, x in enumerate(a, 1):
            cur = [i]
            for j, y in enumerate(b, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
            prev = cur
        return prev[-1]
    rng = random.Random(3)
    for _ in range(200):
        a = [rng.randrange(6) for _ in range(rng.randrange(0, 40))]
        b = [rng.randrange(6) for _ in range(rng.randrange(0, 40))]
        assert levenshtein(a, b) == dp(a, b)


def test_metric_matches_reference(golden_dir):
    """eval metric path: teacher-forced argmax -> trim -> DecodePieces -> Levenshtein, with the toy
    sentencepiece model the reference's Metric ran on when tests/golden/metric.npz was made."""
    from masr_amd.monitor.metric import Metric
    g = np.load(golden_dir / "metric.npz")
    units = ['<s>'] + [l.rstrip().split(' ')[0] for l in open(golden_dir / "toy_spm_units.txt")] + ['</s>']
    m = Metric(golden_dir / "toy_spm.model", units, 0, len(units) - 1)
    pred_ids, gold = torch.from_numpy(g["pred_ids"]), torch.from_numpy(g["gold"])
    logits = torch.nn.functional.one_hot(pred_ids, 367).float()
    assert abs(m.batch_cal_er(logits, gold, ['att'], ['cer'])['att_cer'] - float(g["cer"])) < 1e-9
    assert abs(m.batch_cal_er(logits, gold, ['att'], ['wer'])['att_wer'] - float(g["wer"])) < 1e-9
    for b in range(len(gold)):
        assert abs(m.cal_att_cer(pred_ids[b], gold[b]) - g["per_cer"][b]) < 1e-9
        assert abs(m.cal_att_wer(pred_ids[b], gold[b]) - g["per_wer"][b]) < 1e-9


def test_blstm_init_replay_matches_reference_seed_531(golden_dir):
    """MonoBLSTM's initial weights (module construction order + lecun_normal_init_parameters) for torch.manual_seed(531)"""
    from masr_amd.blstm_engine import reference_init_state_dict as blstm_init
    from oracle.make_goldens import BLSTM_TINY
    g = np.load(golden_dir / "blstm_tiny.npz")
    torch.manual_seed(531)
    sd = blstm_init(BLSTM_TINY, 367)
    assert list(sd.keys()) == g["state_dict_keys"].tolist()
    for n, t in sd.items():
        np.testing.assert_allclose(flat_checks(t), g[f"init/{n}"], rtol=1e-6, atol=1e-7, err_msg=n)


def test_cli_level_init_parity_after_load_data(golden_dir, tmp_path, monkeypatch):
    """pretrain.py order: seeds -> load_data() -> set_model().  The reference's DataLoader iterators draw their base seeds from
    the torch default generator while load_data() runs, so the model initialised afterwards differs from one initialised
    straight after manual_seed(531).  Our Loader replays those draws: DataContainer over the chain's 4 accents followed by the
    init replay yields the weights the reference's own CLI flow started from (tests/golden/chain_toy.npz)."""
    import random
    from masr_amd.io.dataset import DataContainer
    from masr_amd.model import reference_init_state_dict
    from oracle.make_goldens import CFG3_ACCENTS, ODIM, chain_workspace, flat_checks
    g = np.load(golden_dir / "chain_toy.npz")
    pre, _ = chain_workspace(tmp_path, golden_dir)
    monkeypatch.chdir(tmp_path)
    sv = pre["solver"]
    random.seed(531); np.random.seed(531); torch.manual_seed(531)
    DataContainer([tmp_path / "data" / a for _, a in CFG3_ACCENTS], batch_size=sv["batch_size"], dev_batch_size=sv["dev_batch_size"],
                  is_memmap=True, is_bucket=True, min_ilen=sv["min_ilen"], max_ilen=sv["max_ilen"], half_batch_ilen=sv["half_batch_ilen"])
    sd = reference_init_state_dict(pre["asr_model"], ODIM)
    np.testing.assert_allclose(flat_checks(sd["vgg2enc.weight"]), g["pre/init/fp/vgg2enc.weight"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("is_bucket", [True, False])
def test_data_stream_state_round_trip(tmp_path, is_bucket):
    """what `--resume` relies on: DataContainer.state_dict() + the three RNG streams, taken in the middle of an epoch, and restored
    into a FRESH container (whose construction consumed the streams on its own), reproduce the batch stream that followed --
    through several epoch roll-overs (sampler rebuilt with `random`, buckets re-shuffled with np.random / RandomSampler seeds
    from the torch stream)."""
    import pickle
    from masr_amd.io.dataset import capture_rng, restore_rng
    for ai, a in enumerate(["african", "australia"]):
        write_toy_shard(tmp_path, a, "train", 16, seed=100 + ai)
        write_toy_shard(tmp_path, a, "dev", 4, seed=200 + ai)
    mk = lambda: DataContainer([tmp_path / "african", tmp_path / "australia"], batch_size=4, dev_batch_size=4, is_memmap=True,
                               is_bucket=is_bucket, min_ilen=10, max_ilen=50, half_batch_ilen=30)
    random.seed(531); np.random.seed(531); torch.manual_seed(531)
    dc = mk()

    def draw(c, n):
        out = []
        for _ in range(n):
            for acc, (x, il, ys, ol) in c.get_item(None, 1) + c.get_item(1, 2):
                out.append((int(acc), il.tolist(), [y.tolist() for y in ys], round(float(x.sum()), 3)))
        return out
    draw(dc, 3)                                                    # somewhere inside the first epoch
    saved = pickle.loads(pickle.dumps({"data": dc.state_dict(), "rng": capture_rng()}))
    cnt = dc.reload_cnt
    after = draw(dc, 12)                                           # rolls over several epochs
    assert dc.reload_cnt > cnt
    random.seed(1); np.random.seed(2); torch.manual_seed(3)        # a new process: different streams ...
    dc2 = mk()                                                     # ... consumed by the construction
    dc2.load_state_dict(saved["data"])
    restore_rng(saved["rng"])
    assert draw(dc2, 12) == after


def test_slot_cap_rule_and_transport_names():
    """what bench.py reports as meta_step.slot_cap / meta_step.transport (fo_meta_interface.slot_cap, parallel.TaskSharder.transport)"""
    from masr_amd.fo_meta_interface import slot_cap
    from masr_amd.parallel import TaskSharder
    assert slot_cap(4, 8, 1, False) == 4                       # one rank, no collective: nothing to make room for
    assert slot_cap(4, 8, 8, True) == 4                        # one task per rank and meta-step: a single wave
    assert slot_cap(4, 8, 1, True) == 3 and slot_cap(4, 16, 2, True) == 3          # several waves whose all-reduce overlaps the next wave
    assert slot_cap(4, 8, 1, True, no_slot_cap=True) == 4 and slot_cap(3, 8, 1, True) == 3 and slot_cap(2, 8, 2, True) == 2
    assert TaskSharder().transport == "none"
    assert TaskSharder(0, 2, "gloo").transport == "pg_gloo" and TaskSharder(0, 8, "nccl").transport == "pg_nccl"
    import os
    os.environ["MASR_NATIVE_ALLREDUCE"] = "1"
    try:
        assert TaskSharder(0, 8, "nccl").transport == "native" and TaskSharder(0, 8, "gloo").transport == "pg_gloo"
    finally:
        del os.environ["MASR_NATIVE_ALLREDUCE"]
