"""What Tester.exec() does with --decode_mode ctc_align before anything is aligned, without a device: the stub of
test_tester_settings_cpu.py (a Tester made with Tester.__new__ that carries only what the settings functions read).  The mode reads no
solver.beam_decode block, needs a CTC output layer on a transformer and accepts the BLSTM; a stub that passes the vetting gets as far as
the eval set, which it does not have."""
from types import SimpleNamespace

import pytest

import masr_amd  # noqa: F401
from masr_amd import tester as tester_module


def vetted(mode, block, *, model="transformer", head=True):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=None)
    t.decode_mode, t.model_name = mode, model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, 0
    return t


def test_ctc_align_is_a_mode():
    assert "ctc_align" in tester_module.Tester.MODES
    assert "ctc_align" in tester_module.__doc__ and "ctc-ali" in tester_module.__doc__


@pytest.mark.parametrize("block", [None, {}, {"beam_size": 0}], ids=["no block", "empty block", "beam_size 0 is not read"])
def test_no_head_is_refused_whatever_the_block(block):
    with pytest.raises(ValueError) as e:
        vetted("ctc_align", block, head=False).exec()
    assert str(e.value) == ("decode_mode 'ctc_align' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
                            "use --decode_mode greedy or beam to decode instead")


@pytest.mark.parametrize("model", ["transformer", "blstm"])
@pytest.mark.parametrize("block", [None, {"beam_size": 65}], ids=["no block", "a block nobody reads"])
def test_accepted_up_to_the_eval_set(model, block):
    # on a Tester without the mode this is NotImplementedError("ctc_align haven't supported yet")
    with pytest.raises(AttributeError, match="eval_set"):
        vetted("ctc_align", block, model=model, head=model != "blstm").exec()


def test_unknown_mode_message_is_unchanged():
    with pytest.raises(NotImplementedError) as e:
        vetted("ctc_segment", None).exec()
    assert str(e.value) == "ctc_segment haven't supported yet"


def test_train_py_offers_the_mode():
    import train
    act = next(a for a in train.build_parser()._actions if a.dest == "decode_mode")
    assert "ctc_align" in act.choices
