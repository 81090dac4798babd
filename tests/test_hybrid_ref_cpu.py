"""The CPU restatement of the joint CTC/attention objective (tests/hybrid_ref.py) against independent facts, and the hybrid model's
initial weights (masr_amd.model.reference_init_state_dict with asr_model.ctc_weight).  CPU only."""
import numpy as np
import torch

import hybrid_ref
from masr_amd.model import reference_init_state_dict
from oracle import ref_cpu
from oracle.make_goldens import TINY, ODIM, synth_batch


def _setup(ilens, olens, seed=11):
    sd = hybrid_ref.with_head(ref_cpu.deterministic_state_dict(TINY, ODIM, seed=7), ODIM, seed=3)
    return sd, synth_batch(seed, ilens, olens)


def test_ctc_term_matches_numpy_lattice():
    # the last utterance is infeasible (enc_len 5 < 9 labels): zero_infinity drops it from both
    sd, (xs, il, ys, ol) = _setup([64, 52, 40, 20], [9, 7, 5, 9])
    p = hybrid_ref.leafify(sd, TINY)
    with torch.no_grad():
        loss, lp = hybrid_ref.ctc_term(p, TINY, xs, il, ys, ol)
    tgt = torch.cat(ys).numpy()
    enc_lens = (il // 4).numpy()
    want, _ = ref_cpu.ctc_loss_np(lp.numpy(), tgt, enc_lens, ol.numpy())
    assert np.isfinite(float(loss))
    assert abs(float(loss) - want) <= 1e-5 * abs(want), (float(loss), want)
    # ... and the infeasible utterance adds nothing: the mean over the other three, divided by 4
    keep = [0, 1, 2]
    tgt3 = torch.cat([ys[b] for b in keep]).numpy()
    want3, _ = ref_cpu.ctc_loss_np(lp[:, keep].numpy(), tgt3, enc_lens[keep], ol.numpy()[keep])
    assert abs(float(loss) - want3 * 3 / 4) <= 1e-5 * abs(want), (float(loss), want3 * 3 / 4)


def test_weight_zero_is_run_batch_train():
    sd, (xs, il, ys, ol) = _setup([64, 52, 40, 33], [9, 7, 5, 3])
    p = hybrid_ref.leafify(sd, TINY)
    info, grads = hybrid_ref.run_batch_train(p, TINY, (xs, il, ys, ol), 0.2, 0.0)
    q = ref_cpu.leafify({k: v for k, v in sd.items() if k not in hybrid_ref.HEAD}, TINY)
    ref, rgrads, _, _ = ref_cpu.run_batch_train(q, TINY, (xs, il, ys, ol.clone()), 0.2)
    assert info["loss"] == ref["loss"]
    for n, g in rgrads.items():
        torch.testing.assert_close(grads[n], g, rtol=0, atol=0)
    assert all(float(grads[k].abs().max()) == 0.0 for k in hybrid_ref.HEAD)
    # and w > 0 mixes the two terms
    info3, _ = hybrid_ref.run_batch_train(p, TINY, (xs, il, ys, ol), 0.2, 0.3)
    assert abs(info3["loss"] - (0.7 * info3["att"] + 0.3 * info3["ctc"])) <= 1e-6 * info3["loss"]
    assert abs(info3["att"] - ref["loss"]) <= 1e-6 * ref["loss"]


def test_reference_init_with_ctc_head():
    cfg = dict(TINY, ctc_weight=0.3)
    torch.manual_seed(1234)
    plain = reference_init_state_dict(TINY, ODIM)
    torch.manual_seed(1234)
    hyb = reference_init_state_dict(cfg, ODIM)
    assert list(hyb.keys()) == list(plain.keys()) + ["ctc.ctc_lo.weight", "ctc.ctc_lo.bias"]
    for k, v in plain.items():
        assert torch.equal(hyb[k], v), k
    E = TINY["d_model"]
    assert hyb["ctc.ctc_lo.weight"].shape == (ODIM, E) and hyb["ctc.ctc_lo.bias"].shape == (ODIM,)
    a = (6.0 / (E + ODIM)) ** 0.5                        # xavier_uniform_ bound on the weight, Linear's default on the bias
    assert float(hyb["ctc.ctc_lo.weight"].abs().max()) <= a and float(hyb["ctc.ctc_lo.weight"].std()) > 0.3 * a
    assert 0 < float(hyb["ctc.ctc_lo.bias"].abs().max()) <= 1 / E ** 0.5
    # w = 0 (explicit) is the plain init
    torch.manual_seed(1234)
    zero = reference_init_state_dict(dict(TINY, ctc_weight=0.0), ODIM)
    assert list(zero.keys()) == list(plain.keys())


def test_ctc_weight_validation():
    import pytest
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            reference_init_state_dict(dict(TINY, ctc_weight=bad), ODIM)
