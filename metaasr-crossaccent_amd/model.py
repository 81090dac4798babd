"""MyTransformer: the reference's model object (src/model/transformer_pytorch/mono_transformer_torch.py:35-208)
as a facade over MasrEngine.  It keeps the surface the interfaces use -- state_dict / load_state_dict /
parameters / train / eval / forward / recog, sos_id / eos_id -- while every FLOP runs in libmasr."""
from collections import OrderedDict

import torch

from .engine import MasrEngine


def reference_init_state_dict(model_para, odim):
    """Initial weights identical to the reference's for the same torch seed: replays the reference's RNG consumption
    (module construction order of mono_transformer_torch.py:49-104, then xavier_uniform_ over parameters() with
    dim > 1, :106-109) with throw-away torch.nn modules on the host.  Pinned by tests/golden/init.npz.
    asr_model.ctc_weight > 0 (the joint objective; no counterpart in the reference): the CTC head ctc.ctc_lo is built AFTER that whole
    sequence -- nn.Linear(E, odim), then xavier_uniform_ on its weight (its bias keeps Linear's init) -- so every other tensor is the
    same for the same seed, and its two tensors follow the rest of the state_dict."""
    from .engine import ctc_weight_of
    import warnings
    from torch import nn
    p = model_para
    E, H = p['d_model'], p['nheads']
    feat = nn.Sequential(nn.Conv2d(1, 64, 3, 1, 1), nn.ReLU(), nn.Conv2d(64, 64, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2),
                         nn.Conv2d(64, 128, 3, 1, 1), nn.ReLU(), nn.Conv2d(128, 128, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2))
    vgg2enc = nn.Linear(128 * (p['idim'] // 4), E)
    char_trans = nn.Linear(E, odim)
    pre_embed = nn.Embedding(odim, E)
    if p.get('tgt_share_weight', 0) != 0:
        char_trans.weight = pre_embed.weight
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc_layer = nn.TransformerEncoderLayer(E, H, p['d_inner'], p.get('dropout', 0.0))
        enc = nn.TransformerEncoder(enc_layer, p['encoder']['nlayers'], nn.LayerNorm(E))
        dec_layer = nn.TransformerDecoderLayer(E, H, p['d_inner'], p.get('dropout', 0.0))
        dec = nn.TransformerDecoder(dec_layer, p['decoder']['nlayers'], nn.LayerNorm(E))
    mods = OrderedDict(feat_extractor=feat, vgg2enc=vgg2enc, char_trans=char_trans, pre_embed=pre_embed, encoder=enc, decoder=dec)
    seen = set()
    for mod in mods.values():
        for prm in mod.parameters():
            if id(prm) in seen:
                continue
            seen.add(id(prm))
            if prm.dim() > 1:
                nn.init.xavier_uniform_(prm)
    sd = OrderedDict()
    for mname, mod in mods.items():
        for n, t in mod.state_dict().items():
            sd[f"{mname}.{n}"] = t.detach()
    if ctc_weight_of(p) > 0.0:
        ctc_lo = nn.Linear(E, odim)
        nn.init.xavier_uniform_(ctc_lo.weight)
        sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"] = ctc_lo.weight.detach(), ctc_lo.bias.detach()
    return sd


class MyTransformer:
    def __init__(self, id2char, model_para, label_smoothing=0.0, device="cuda:0", init=True):
        self.idim = model_para['idim']
        self.odim = len(id2char)
        self.sos_id, self.eos_id = 0, len(id2char) - 1                      # :45-46
        self.d_model, self.nhead = model_para['d_model'], model_para['nheads']
        self.engine = MasrEngine(model_para, self.odim, label_smoothing, device)
        self.training = True
        if init:
            self.init_parameters()

    @property
    def device(self):
        return self.engine.device

    def cuda(self):
        return self                                                          # already there (reference hard-codes .cuda(), F9)

    def init_parameters(self):
        self.engine.load_state_dict(reference_init_state_dict(self.engine.model_para, self.odim))

    # ---- nn.Module-like surface ---------------------------------------------------------------
    def parameters(self):
        return [self.engine.params]

    def state_dict(self, keep_vars=False):
        return self.engine.state_dict(clone=not keep_vars)

    def load_state_dict(self, sd, strict=True):
        self.engine.load_state_dict(sd)

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    # ---- operator ------------------------------------------------------------------------------
    def forward(self, xs_pad, ilens, ys, olens):
        """(:178-208) -> (logit [B,L,odim] on device, ys_out_pad [B,L] int64 on device, -1 padded).
        Inference-only entry (no autograd graph exists on this path); training goes through run_batch.
        Reproduces quirk Q6: olens is incremented in place."""
        assert xs_pad.size(0) == ilens.size(0) == len(ys) == olens.size(0), "Batch size mismatch"
        self.engine.run_batch(xs_pad, ilens, ys, olens, train=False)
        olens += 1
        logit, gold = self.engine.last_logits()
        return logit, gold.to(torch.int64)

    __call__ = forward

    def recog(self, xs_pad, ilens):
        """greedy decode (:143-176): encoder once, max(enc_lens) full re-decodes, arg-max of every position -> [Ldec, B]"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog(xs_pad, ilens)

    def beam_decode(self, xs_pad, ilens, beam_size, min_step_ratio=0.0, max_step_ratio=1.0, att_weight=1.0, ctc_weight=0.0):
        """beam search (masr_recog_beam, or masr_recog_beam_ctc when ctc_weight != 0; the reference has none for this model):
        (B token lists without sos / eos, scores [B])"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam(xs_pad, ilens, beam_size, min_step_ratio, max_step_ratio, att_weight, ctc_weight)

    def lm_beam_decode(self, xs_pad, ilens, beam_size, lm, lm_weight, min_step_ratio=0.0, max_step_ratio=1.0):
        """beam search with shallow fusion of the n-gram LM `lm` (an NGramLM; masr_recog_beam_lm): (B token lists without sos / eos,
        scores [B])"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_lm(xs_pad, ilens, beam_size, lm, lm_weight, min_step_ratio, max_step_ratio)

    def nlm_beam_decode(self, xs_pad, ilens, beam_size, nlm, lm_weight, min_step_ratio=0.0, max_step_ratio=1.0):
        """beam search with shallow fusion of the LSTM LM `nlm` (an LstmLM; masr_recog_beam_nlm): (B token lists without sos / eos,
        scores [B])"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_nlm(xs_pad, ilens, beam_size, nlm, lm_weight, min_step_ratio, max_step_ratio)

    def lm_joint_beam_decode(self, xs_pad, ilens, beam_size, lm, lm_weight=0.3, len_bonus=0.0, nbest=1, min_step_ratio=0.0, max_step_ratio=1.0,
                             att_weight=0.7, ctc_weight=0.3):
        """one-pass joint CTC/attention beam search with the n-gram LM `lm`, a per-token bonus and an N-best list (masr_recog_beam_ctc_lm,
        hybrid models only): per utterance a list of at most nbest (token list, score), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_ctc_lm(xs_pad, ilens, beam_size, lm, lm_weight, len_bonus, nbest, min_step_ratio, max_step_ratio,
                                             att_weight, ctc_weight)

    def nlm_joint_beam_decode(self, xs_pad, ilens, beam_size, nlm, lm_weight=0.3, len_bonus=0.0, nbest=1, min_step_ratio=0.0, max_step_ratio=1.0,
                              att_weight=0.7, ctc_weight=0.3):
        """lm_joint_beam_decode with the LSTM LM `nlm` (an LstmLM) in the n-gram's place (masr_recog_beam_ctc_nlm, hybrid models only): per
        utterance a list of at most nbest (token list, score), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_ctc_nlm(xs_pad, ilens, beam_size, nlm, lm_weight, len_bonus, nbest, min_step_ratio, max_step_ratio,
                                              att_weight, ctc_weight)

    def ctc_beam_decode(self, xs_pad, ilens, beam_size, nbest=1):
        """CTC prefix beam search on the CTC head alone (masr_recog_ctc_beam, hybrid models only): per utterance a list of at most
        nbest (token list, score), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_ctc_beam(xs_pad, ilens, beam_size, nbest)

    def ctc_align(self, xs_pad, ilens, ys, olens):
        """CTC forced alignment of each utterance's transcript on the CTC head (masr_recog_ctc_align, hybrid models only): per utterance
        (score, [(token, start, end), ...], frames list) in encoder frames (4 input frames each)"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.ctc_align(xs_pad, ilens, ys, olens)

    def lm_ctc_beam_decode(self, xs_pad, ilens, beam_size, lm, lm_weight=0.3, len_bonus=0.0, nbest=1):
        """CTC prefix beam search with the n-gram LM `lm` and a per-token bonus fused in (masr_recog_ctc_beam_lm, hybrid models only): per
        utterance a list of at most nbest (token list, fused score, acoustic score), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_ctc_beam_lm(xs_pad, ilens, beam_size, lm, lm_weight, len_bonus, nbest)

    def lm_rescore_decode(self, xs_pad, ilens, beam_size, lm, lm_weight=0.3, len_bonus=0.0, nbest=None, att_weight=0.5, ctc_weight=0.5):
        """attention rescoring of the LM-fused CTC beam's nbest list (masr_recog_rescore_lm, hybrid models only): rescore_decode with
        lm_ctc_beam_decode's search as the first pass"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_rescore_lm(xs_pad, ilens, beam_size, lm, lm_weight, len_bonus, nbest, att_weight, ctc_weight)

    def bias_ctc_beam_decode(self, xs_pad, ilens, beam_size, bias, bias_weight=3.0, lm=None, lm_weight=0.3, len_bonus=0.0, nbest=1):
        """CTC prefix beam search with the phrase list `bias` (a ContextBias) boosting its phrases (masr_recog_ctc_beam_bias, hybrid models
        only), the n-gram LM `lm` fused in when one is given: per utterance a list of at most nbest (token list, final score, acoustic
        score, credited tokens), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_ctc_beam_bias(xs_pad, ilens, beam_size, bias, bias_weight, lm, lm_weight, len_bonus, nbest)

    def bias_beam_decode(self, xs_pad, ilens, beam_size, bias, bias_weight=3.0, lm=None, lm_weight=0.3, min_step_ratio=0.0, max_step_ratio=1.0):
        """the attention beam with the phrase list `bias` (a ContextBias) boosting its phrases (masr_recog_beam_bias), the n-gram LM `lm` fused
        in when one is given: (B token lists without sos / eos, scores [B], credited tokens [B])"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_bias(xs_pad, ilens, beam_size, bias, bias_weight, lm, lm_weight, min_step_ratio, max_step_ratio)

    def bias_joint_beam_decode(self, xs_pad, ilens, beam_size, bias, bias_weight=3.0, lm=None, lm_weight=0.3, len_bonus=0.0, nbest=1,
                               min_step_ratio=0.0, max_step_ratio=1.0, att_weight=0.7, ctc_weight=0.3):
        """the one-pass joint CTC/attention beam with the phrase list `bias` (masr_recog_beam_ctc_bias, hybrid models only), lm_joint_beam_decode's
        search with or without its LM: per utterance a list of at most nbest (token list, score, credited tokens), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_beam_ctc_bias(xs_pad, ilens, beam_size, bias, bias_weight, lm, lm_weight, len_bonus, nbest, min_step_ratio,
                                               max_step_ratio, att_weight, ctc_weight)

    def bias_rescore_decode(self, xs_pad, ilens, beam_size, bias, bias_weight=3.0, lm=None, lm_weight=0.3, len_bonus=0.0, nbest=None,
                            att_weight=0.5, ctc_weight=0.5):
        """attention rescoring of the phrase-biased CTC beam's nbest list (masr_recog_rescore_bias, hybrid models only): rescore_decode with
        bias_ctc_beam_decode's search as the first pass"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_rescore_bias(xs_pad, ilens, beam_size, bias, bias_weight, lm, lm_weight, len_bonus, nbest, att_weight, ctc_weight)

    def nlm_ctc_beam_decode(self, xs_pad, ilens, beam_size, nlm, lm_weight=0.3, len_bonus=0.0, nbest=1):
        """lm_ctc_beam_decode with the LSTM LM `nlm` (an LstmLM) in the n-gram's place (masr_recog_ctc_beam_nlm, hybrid models only): per
        utterance a list of at most nbest (token list, fused score, acoustic score), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_ctc_beam_nlm(xs_pad, ilens, beam_size, nlm, lm_weight, len_bonus, nbest)

    def nlm_rescore_decode(self, xs_pad, ilens, beam_size, nlm, lm_weight=0.3, len_bonus=0.0, nbest=None, att_weight=0.5, ctc_weight=0.5):
        """attention rescoring of the LSTM-LM-fused CTC beam's nbest list (masr_recog_rescore_nlm, hybrid models only): rescore_decode with
        nlm_ctc_beam_decode's search as the first pass"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_rescore_nlm(xs_pad, ilens, beam_size, nlm, lm_weight, len_bonus, nbest, att_weight, ctc_weight)

    def rescore_decode(self, xs_pad, ilens, beam_size, nbest=None, att_weight=0.5, ctc_weight=0.5):
        """attention rescoring (masr_recog_rescore, hybrid models only): the CTC prefix beam's nbest list re-ranked by
        att_weight * log p_att + ctc_weight * log p_ctc after one teacher-forced decoder pass; per utterance a list of
        (tokens, score, att, ctc, first_pass_rank), best first"""
        assert xs_pad.size(0) == ilens.size(0), "Batch size mismatch"
        return self.engine.recog_rescore(xs_pad, ilens, beam_size, nbest, att_weight, ctc_weight)
