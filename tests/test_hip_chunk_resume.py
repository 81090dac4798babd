"""--resume under a dynamic chunk policy (asr_model.chunk.dynamic): the chunk of a step is drawn from the step's dropout seed, whose position
the snapshot holds, so 4 steps + snapshot + resume + 4 steps end on the weights of 8 uninterrupted steps, bit for bit -- the way
tests/test_hip_resume.py checks a run without a policy."""
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
from oracle.make_goldens import cfg3_workspace  # noqa: E402
from test_hip_resume import _assert_state_equal  # noqa: E402


def test_pretrain_resume_under_a_dynamic_chunk_is_an_exact_continuation(golden_dir, tmp_path, monkeypatch):
    import pretrain
    monkeypatch.chdir(tmp_path)
    cfg = cfg3_workspace(tmp_path, golden_dir)
    cfg["solver"].update(eval_ival=4, save_ival=4)
    cfg["asr_model"].update(dropout=0.1, pos_dropout=0.1)

    def cli(suffix, max_step, policy, *extra):
        cfg["asr_model"].pop("chunk", None)
        if policy:
            cfg["asr_model"]["chunk"] = policy
        yaml.safe_dump(cfg, open(tmp_path / "cfg.yaml", "w"))
        pretrain.main(["--config", "cfg.yaml", "--pretrain_suffix", suffix, "--pretrain_accents", "af", "au", "en", "us", "--num_pretrain", "4",
                       "--tgt_accent", "ca", "--algo", "fomaml", "--meta_k", "1", "--meta_batch_size", "4", "--max_step", str(max_step), "--njobs", "2",
                       *extra])
        torch.cuda.synchronize()
        return tmp_path / "testing-logs" / "pretrain" / "cfg3" / "fomaml" / suffix / "canada" / "0"
    pol = dict(size=2, left=1, dynamic=1)
    full = cli("full", 8, pol, "--overwrite")
    part = cli("part", 4, pol, "--overwrite")
    assert int((part / "global_step").read_text()) == 4
    part = cli("part", 8, pol, "--resume")
    assert int((part / "global_step").read_text()) == int((full / "global_step").read_text()) == 8
    for name in ("snapshot.latest", "meta_state.latest"):
        _assert_state_equal(torch.load(full / name, weights_only=False), torch.load(part / name, weights_only=False), name)
    # (the policy did act: the same 8 steps without it end elsewhere)
    off = cli("off", 8, None, "--overwrite")
    a, b = torch.load(full / "snapshot.latest", weights_only=False), torch.load(off / "snapshot.latest", weights_only=False)
    assert any(not torch.equal(a[k], b[k]) for k in a if isinstance(a[k], torch.Tensor))
