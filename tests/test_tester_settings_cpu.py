"""What Tester.exec() refuses before anything is decoded, per decode mode, without a device: the exception type and the full message
of every fault that is raised before the LM file is read (the faults behind that stay with the GPU tests).  The Tester is made with
Tester.__new__ and carries only what the settings functions read; its model is a stub whose engine.ctc_weight says whether there is a
CTC head.  The expected texts are literals recorded before the settings functions were folded onto shared helpers."""
from types import SimpleNamespace

import masr_amd  # noqa: F401
from masr_amd import tester as tester_module                  # (not `Tester` itself: pytest would try to collect it as a test class)

INF = float("inf")
MODES = ("beam", "lm_beam", "ctc_beam", "rescore", "lm_ctc_beam", "lm_rescore", "lm_joint_beam")
LM_MODES = ("lm_beam", "lm_ctc_beam", "lm_rescore", "lm_joint_beam")
NEED_HEAD = ("ctc_beam", "rescore", "lm_ctc_beam", "lm_rescore", "lm_joint_beam")
REFUSE_BLSTM = ("beam", "lm_beam", "rescore", "lm_rescore", "lm_joint_beam")
OK = {"beam_size": 4, "ctc_w": 0.3}                             # valid in every mode on a hybrid transformer (lm_beam: with ctc_w 0)


def vetted(mode, block, *, model="transformer", head=True, path="no/such/file.arpa", blank=0):
    t = tester_module.Tester.__new__(tester_module.Tester)
    t.config = {"solver": {} if block is None else {"beam_decode": block}}
    t.paras = SimpleNamespace(lm_model_path=path)
    t.decode_mode, t.model_name = mode, model
    t.asr_model = SimpleNamespace(engine=SimpleNamespace(ctc_weight=0.3 if head else 0.0))
    t.id2ch, t.sos_id, t.eos_id, t.blank_id = ["<s>"] + [f"u{i}" for i in range(1, 12)] + ["</s>"], 0, 12, blank
    return t


def cases():
    """(label, mode, block, keyword arguments of vetted())"""
    for mode in MODES:
        ok = dict(OK, ctc_w=0.0) if mode == "lm_beam" else OK
        yield "no block", mode, None, {}
        yield "block without beam_size", mode, {"lm_w": 0.3}, {}
        yield "beam_size 0", mode, dict(ok, beam_size=0), {}
        yield "beam_size 65", mode, dict(ok, beam_size=65), {}
        if mode in REFUSE_BLSTM:
            yield "blstm", mode, ok, dict(model="blstm")
        if mode in NEED_HEAD:
            yield "no head", mode, ok, dict(head=False)
            yield "no head + beam_size 0", mode, dict(ok, beam_size=0), dict(head=False)
        if mode in LM_MODES:
            yield "no path", mode, ok, dict(path=None)
            yield "no path + blstm + no block", mode, None, dict(path=None, model="blstm")
            yield "lm_w -0.5", mode, dict(ok, lm_w=-0.5), {}
            yield "lm_w nan", mode, dict(ok, lm_w=float("nan")), {}
        if mode in ("lm_ctc_beam", "lm_rescore", "lm_joint_beam"):
            yield "len_bonus inf", mode, dict(ok, len_bonus=INF), {}
            yield "lm_w -1 + len_bonus inf", mode, dict(ok, lm_w=-1.0, len_bonus=INF), {}
        if mode in ("rescore", "lm_rescore", "lm_joint_beam"):
            yield "nbest 0", mode, dict(ok, nbest=0), {}
            yield "nbest beam_size + 1", mode, dict(ok, nbest=5), {}
        if mode in ("rescore", "lm_rescore"):
            yield "att_w 0", mode, dict(ok, att_w=0.0), {}
            yield "ctc_w 1 (att_w defaults to 0)", mode, dict(ok, ctc_w=1.0), {}
            yield "nbest 5 + att_w 0 + no head", mode, dict(ok, nbest=5, att_w=0.0), dict(head=False)
            yield "att_w 0 + no head", mode, dict(ok, att_w=0.0), dict(head=False)
        if mode in ("beam", "rescore", "lm_rescore", "lm_joint_beam"):
            yield "ctc_w -1", mode, dict(ok, ctc_w=-1.0), {}
            yield "att_w inf", mode, dict(ok, att_w=INF), {}
        if mode == "beam":
            yield "ctc_w 1.5 without att_w", mode, dict(ok, ctc_w=1.5), {}
            yield "ctc_w 1.5 without att_w, no head", mode, dict(ok, ctc_w=1.5), dict(head=False)
    yield "ctc_w absent", "lm_joint_beam", {"beam_size": 4}, {}
    yield "ctc_w 0", "lm_joint_beam", {"beam_size": 4, "ctc_w": 0.0}, {}
    yield "ctc_w absent + no head", "lm_joint_beam", {"beam_size": 4}, dict(head=False)
    yield "ctc_w absent + lm_w -1", "lm_joint_beam", {"beam_size": 4, "lm_w": -1.0}, {}
    yield "len_bonus inf + nbest 0", "lm_joint_beam", dict(OK, len_bonus=INF, nbest=0), {}
    yield "att_w -1 + lm_w -1", "lm_joint_beam", dict(OK, att_w=-1.0, lm_w=-1.0), {}
    yield "ctc_w 0.3 on a hybrid model", "lm_beam", OK, {}
    yield "ctc_w 0.3 on a hybrid model + lm_w -1", "lm_beam", dict(OK, lm_w=-1.0), {}
    yield "ctc_w -1", "lm_beam", dict(OK, ctc_w=-1.0), {}
    yield "blank not at 0", "lm_ctc_beam", OK, dict(model="blstm", blank=3)
    yield "blank not at 0 + lm_w -1", "lm_ctc_beam", dict(OK, lm_w=-1.0), dict(model="blstm", blank=3)
    yield "unknown mode", "nbest_beam", OK, {}


def measure():
    out = {}
    for label, mode, block, kw in cases():
        try:
            vetted(mode, block, **kw).exec()
            out[f"{mode}: {label}"] = None                          # (no case gets here: each is refused before the eval set is touched)
        except Exception as e:                                      # noqa: BLE001
            out[f"{mode}: {label}"] = (type(e).__name__, str(e))
    return out


EXPECTED = {'beam: att_w inf': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got inf'),
 'beam: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'beam: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'beam: block without beam_size': ('ValueError', "decode_mode 'beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'beam: blstm': ('NotImplementedError',
                 "beam: beam search is only implemented for the transformer (the reference's BLSTM beam decoder is dead code, DESIGN 9); use "
                 '--decode_mode greedy'),
 'beam: ctc_w -1': ('ValueError', 'solver.beam_decode.ctc_w must be finite and >= 0, got -1.0'),
 'beam: ctc_w 1.5 without att_w': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got -0.5'),
 'beam: ctc_w 1.5 without att_w, no head': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got -0.5'),
 'beam: no block': ('ValueError', "decode_mode 'beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'ctc_beam: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'ctc_beam: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'ctc_beam: block without beam_size': ('ValueError', "decode_mode 'ctc_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'ctc_beam: no block': ('ValueError', "decode_mode 'ctc_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'ctc_beam: no head': ('ValueError',
                       "decode_mode 'ctc_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use "
                       '--decode_mode beam or greedy'),
 'ctc_beam: no head + beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_beam: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_beam: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'lm_beam: block without beam_size': ('ValueError', "decode_mode 'lm_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_beam: blstm': ('NotImplementedError',
                    "lm_beam: LM fusion is only implemented for the transformer's attention beam; use --decode_mode ctc_beam or greedy"),
 'lm_beam: ctc_w -1': ('ValueError', 'solver.beam_decode.ctc_w must be finite and >= 0, got -1.0'),
 'lm_beam: ctc_w 0.3 on a hybrid model': ('ValueError',
                                          'lm_beam: the LM is not fused into the joint CTC/attention beam (beam_decode.ctc_w = 0.3); set '
                                          'beam_decode.ctc_w: 0 to fuse it into the attention beam, or use --decode_mode beam without an LM'),
 'lm_beam: ctc_w 0.3 on a hybrid model + lm_w -1': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -1.0'),
 'lm_beam: lm_w -0.5': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -0.5'),
 'lm_beam: lm_w nan': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got nan'),
 'lm_beam: no block': ('ValueError', "decode_mode 'lm_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_beam: no path': ('NotImplementedError', 'lm_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'lm_beam: no path + blstm + no block': ('NotImplementedError',
                                         'lm_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'lm_ctc_beam: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_ctc_beam: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'lm_ctc_beam: blank not at 0': ('ValueError', "decode_mode 'lm_ctc_beam' needs the blank at id 0 (its slot serves as the LM's <s>), got 3"),
 'lm_ctc_beam: blank not at 0 + lm_w -1': ('ValueError',
                                           "decode_mode 'lm_ctc_beam' needs the blank at id 0 (its slot serves as the LM's <s>), got 3"),
 'lm_ctc_beam: block without beam_size': ('ValueError',
                                          "decode_mode 'lm_ctc_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_ctc_beam: len_bonus inf': ('ValueError', 'solver.beam_decode.len_bonus must be finite, got inf'),
 'lm_ctc_beam: lm_w -0.5': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -0.5'),
 'lm_ctc_beam: lm_w -1 + len_bonus inf': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -1.0'),
 'lm_ctc_beam: lm_w nan': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got nan'),
 'lm_ctc_beam: no block': ('ValueError', "decode_mode 'lm_ctc_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_ctc_beam: no head': ('ValueError',
                          "decode_mode 'lm_ctc_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use "
                          '--decode_mode lm_beam, beam or greedy'),
 'lm_ctc_beam: no head + beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_ctc_beam: no path': ('NotImplementedError',
                          'lm_ctc_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'lm_ctc_beam: no path + blstm + no block': ('NotImplementedError',
                                             'lm_ctc_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output '
                                             'units)'),
 'lm_joint_beam: att_w -1 + lm_w -1': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got -1.0'),
 'lm_joint_beam: att_w inf': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got inf'),
 'lm_joint_beam: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_joint_beam: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'lm_joint_beam: block without beam_size': ('ValueError',
                                            "decode_mode 'lm_joint_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_joint_beam: blstm': ('NotImplementedError',
                          "lm_joint_beam: the joint CTC/attention beam needs the transformer's decoder, the BLSTM has none; use --decode_mode "
                          'lm_ctc_beam, ctc_beam or greedy'),
 'lm_joint_beam: ctc_w -1': ('ValueError', 'solver.beam_decode.ctc_w must be finite and >= 0, got -1.0'),
 'lm_joint_beam: ctc_w 0': ('ValueError',
                            'lm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LM into the attention beam alone '
                            'use --decode_mode lm_beam'),
 'lm_joint_beam: ctc_w absent': ('ValueError',
                                 'lm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LM into the attention beam '
                                 'alone use --decode_mode lm_beam'),
 'lm_joint_beam: ctc_w absent + lm_w -1': ('ValueError',
                                           'lm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LM into the '
                                           'attention beam alone use --decode_mode lm_beam'),
 'lm_joint_beam: ctc_w absent + no head': ('ValueError',
                                           "decode_mode 'lm_joint_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is "
                                           '0 or absent); use --decode_mode lm_beam, beam or greedy'),
 'lm_joint_beam: len_bonus inf': ('ValueError', 'solver.beam_decode.len_bonus must be finite, got inf'),
 'lm_joint_beam: len_bonus inf + nbest 0': ('ValueError', 'solver.beam_decode.len_bonus must be finite, got inf'),
 'lm_joint_beam: lm_w -0.5': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -0.5'),
 'lm_joint_beam: lm_w -1 + len_bonus inf': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -1.0'),
 'lm_joint_beam: lm_w nan': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got nan'),
 'lm_joint_beam: nbest 0': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 0'),
 'lm_joint_beam: nbest beam_size + 1': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 5'),
 'lm_joint_beam: no block': ('ValueError', "decode_mode 'lm_joint_beam' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_joint_beam: no head': ('ValueError',
                            "decode_mode 'lm_joint_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
                            'use --decode_mode lm_beam, beam or greedy'),
 'lm_joint_beam: no head + beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_joint_beam: no path': ('NotImplementedError',
                            'lm_joint_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'lm_joint_beam: no path + blstm + no block': ('NotImplementedError',
                                               'lm_joint_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output '
                                               'units)'),
 'lm_rescore: att_w 0': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'lm_rescore: att_w 0 + no head': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'lm_rescore: att_w inf': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got inf'),
 'lm_rescore: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_rescore: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'lm_rescore: block without beam_size': ('ValueError',
                                         "decode_mode 'lm_rescore' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_rescore: blstm': ('NotImplementedError',
                       "rescore: attention rescoring needs the transformer's decoder, the BLSTM has none; use --decode_mode ctc_beam or greedy"),
 'lm_rescore: ctc_w -1': ('ValueError', 'solver.beam_decode.ctc_w must be finite and >= 0, got -1.0'),
 'lm_rescore: ctc_w 1 (att_w defaults to 0)': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'lm_rescore: len_bonus inf': ('ValueError', 'solver.beam_decode.len_bonus must be finite, got inf'),
 'lm_rescore: lm_w -0.5': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -0.5'),
 'lm_rescore: lm_w -1 + len_bonus inf': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got -1.0'),
 'lm_rescore: lm_w nan': ('ValueError', 'solver.beam_decode.lm_w must be finite and >= 0, got nan'),
 'lm_rescore: nbest 0': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 0'),
 'lm_rescore: nbest 5 + att_w 0 + no head': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 5'),
 'lm_rescore: nbest beam_size + 1': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 5'),
 'lm_rescore: no block': ('ValueError', "decode_mode 'lm_rescore' needs a solver.beam_decode block with at least beam_size in the config"),
 'lm_rescore: no head': ('ValueError',
                         "decode_mode 'rescore' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use "
                         '--decode_mode beam or greedy'),
 'lm_rescore: no head + beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'lm_rescore: no path': ('NotImplementedError',
                         'lm_rescore: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'lm_rescore: no path + blstm + no block': ('NotImplementedError',
                                            'lm_rescore: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)'),
 'nbest_beam: unknown mode': ('NotImplementedError', "nbest_beam haven't supported yet"),
 'rescore: att_w 0': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'rescore: att_w 0 + no head': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'rescore: att_w inf': ('ValueError', 'solver.beam_decode.att_w must be finite and >= 0, got inf'),
 'rescore: beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0'),
 'rescore: beam_size 65': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 65'),
 'rescore: block without beam_size': ('ValueError', "decode_mode 'rescore' needs a solver.beam_decode block with at least beam_size in the config"),
 'rescore: blstm': ('NotImplementedError',
                    "rescore: attention rescoring needs the transformer's decoder, the BLSTM has none; use --decode_mode ctc_beam or greedy"),
 'rescore: ctc_w -1': ('ValueError', 'solver.beam_decode.ctc_w must be finite and >= 0, got -1.0'),
 'rescore: ctc_w 1 (att_w defaults to 0)': ('ValueError', "solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got 0.0"),
 'rescore: nbest 0': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 0'),
 'rescore: nbest 5 + att_w 0 + no head': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 5'),
 'rescore: nbest beam_size + 1': ('ValueError', 'solver.beam_decode.nbest must be in [1, beam_size], got 5'),
 'rescore: no block': ('ValueError', "decode_mode 'rescore' needs a solver.beam_decode block with at least beam_size in the config"),
 'rescore: no head': ('ValueError',
                      "decode_mode 'rescore' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); use "
                      '--decode_mode beam or greedy'),
 'rescore: no head + beam_size 0': ('ValueError', 'solver.beam_decode.beam_size must be in [1, 64], got 0')}


def test_every_mode_refuses_what_it_refused():
    got = measure()
    assert sorted(got) == sorted(EXPECTED)
    wrong = {k: (got[k], EXPECTED[k]) for k in EXPECTED if got[k] != EXPECTED[k]}
    assert not wrong, wrong
    assert all(v is not None and v[0] in ("ValueError", "NotImplementedError") for v in EXPECTED.values())
