"""Tester: greedy decoding of the test shard into `<log_dir>/<decode_suffix>/best-hyp` (reference: src/tester.py:18-273).
Line format "<ref ids> TAB <hyp ids>" (space separated), `trim` = cut at the first </s> after position 0 -- unchanged, so
translate.py / score.sh of the reference run on these files as they are.  Only the transformer + greedy path exists in
the reference for this model (beam search raises NotImplementedError there, tester.py:121-124); `--decode_mode beam` with the
transformer runs this project's GPU beam search (masr_recog_beam) with the config's solver.beam_decode block and writes the
best hypothesis of each utterance in the same line format.  On a hybrid model (asr_model.ctc_weight > 0) a block with ctc_w > 0 runs
the joint CTC/attention search (masr_recog_beam_ctc) with att_w (default 1 - ctc_w) and ctc_w.  The weights are checked on every model,
hybrid or plain, before anything is decoded: a negative or non-finite ctc_w or att_w raises ValueError, and so does ctc_w > 1 without an
att_w (the default 1 - ctc_w is then negative).  A plain model with valid weights decodes as before and logs that they are ignored.
`--decode_mode rescore` (hybrid transformers) is the two-pass decode of DESIGN 5.4 (masr_recog_rescore): the CTC prefix beam of
`ctc_beam` with beam_size, its nbest (default beam_size) best re-ranked by att_w * attention score + ctc_w * CTC score after one
teacher-forced decoder pass; ctc_w defaults to 0.5, att_w to 1 - ctc_w, and att_w must be > 0.
`--decode_mode lm_beam` (transformers) is the attention beam with an n-gram LM fused in (masr_recog_beam_lm): the ARPA file of
`--lm_model_path` over the output units, weighted by beam_decode.lm_w (default 0.3); beam_size and the step ratios as for `beam`.  The path is
read at exec(): without one the mode raises NotImplementedError (the reference asserts the path when its Tester is constructed).  The LM
is not fused into the joint CTC/attention beam by this mode: a hybrid model with beam_decode.ctc_w > 0 raises ValueError (`lm_joint_beam` below
is that search).
`--decode_mode lm_ctc_beam` (BLSTM-CTC and hybrid transformers) is the CTC prefix beam of `ctc_beam` with that n-gram LM and a per-token
bonus fused into the search (masr_ctc_beam_search_lm): `--lm_model_path` as for `lm_beam`, beam_decode.beam_size, lm_w (default
0.3, finite and >= 0) and len_bonus (default 0, finite, any sign).  `--decode_mode lm_rescore` (hybrid transformers) is `rescore` with that
search as its first pass (masr_recog_rescore_lm): nbest, att_w and ctc_w as for `rescore`.  Both vet every setting at exec(), before
anything is decoded, and build the LM once per Tester.
`--decode_mode lm_joint_beam` (hybrid transformers) is the one-pass joint CTC/attention beam with that n-gram LM in the pre-beam and the score,
a per-token bonus and an N-best list (masr_recog_beam_ctc_lm): `--lm_model_path` as for `lm_beam`; beam_size, att_w / ctc_w and the
step ratios as for `beam`, with ctc_w > 0 required (ctc_w absent or 0 raises ValueError: that search is `lm_beam`); lm_w (default 0.3),
len_bonus (default 0, finite, any sign) and nbest (default 1, in [1, beam_size]).  The best entry of each utterance is written.  Every
setting is vetted at exec(): no path or a BLSTM raises NotImplementedError, a transformer without a CTC head ValueError."""
import math
from pathlib import Path
from shutil import rmtree

import torch

from .io.dataset import get_loader
from .marcos import *  # noqa: F401,F403
from .model import MyTransformer
from .monitor import logger
from .pretrain_interface import load_units


class Tester:
    def __init__(self, config, paras, id2accent):
        self.config, self.paras = config, paras
        self.train_type = 'evaluation'
        self.is_memmap, self.model_name = paras.is_memmap, paras.model_name
        if paras.algo == 'no' and paras.pretrain_suffix is None:
            paras.pretrain_suffix = paras.eval_suffix
        self.data_dir = Path(config['solver']['data_root'], id2accent[paras.accent])
        self.log_dir = Path(Path.cwd(), LOG_DIR, self.train_type, config['solver']['setting'], paras.algo, paras.pretrain_suffix,
                            paras.eval_suffix, id2accent[paras.accent], str(paras.runs))
        self.model_path = Path(self.log_dir, paras.test_model)
        assert self.model_path.exists(), f"{self.model_path.as_posix()} not exists..."
        self.decode_dir = Path(self.log_dir, paras.decode_suffix)
        self.decode_mode = paras.decode_mode
        self.batch_size = paras.decode_batch_size
        if not paras.resume:
            if self.decode_dir.exists():
                assert paras.overwrite, f"Path exists ({self.decode_dir}). Use --overwrite or change decode suffix"
                rmtree(self.decode_dir)
            self.decode_dir.mkdir(parents=True)
            self.prev_decode_step = -1
        else:
            with open(Path(self.decode_dir, 'best-hyp')) as f:
                self.prev_decode_step = sum(1 for _ in f)

    def load_data(self):
        if self.model_name not in ('transformer', 'blstm'):
            raise NotImplementedError
        self.id2ch = load_units(self.config, self.model_name)
        self.eval_set = get_loader(self.data_dir.joinpath('test'), batch_size=self.batch_size,
                                   half_batch_ilen=512 if self.batch_size > 1 else None, is_memmap=self.is_memmap,
                                   is_bucket=False, shuffle=False, num_workers=1)

    def set_model(self):
        device = getattr(self.paras, 'device', None) or "cuda:0"
        if self.model_name == 'blstm':
            from .blstm_engine import MonoBLSTM
            self.asr_model = MonoBLSTM(self.id2ch, self.config['asr_model'], device=device, init=False)
            self.asr_model.load_state_dict(torch.load(self.model_path, map_location='cpu'))
            self.asr_model.eval()
            self.sos_id, self.eos_id, self.blank_id = self.asr_model.sos_id, self.asr_model.eos_id, self.asr_model.blank_id
            return
        self.blank_id = None
        self.asr_model = MyTransformer(self.id2ch, self.config['asr_model'], device=device, init=False)
        self.asr_model.load_state_dict(torch.load(self.model_path, map_location='cpu'))
        self.asr_model.eval()
        self.sos_id, self.eos_id = self.asr_model.sos_id, self.asr_model.eos_id

    def trim(self, hyp):
        """tester.py:189-207 (transformer): everything from the first </s> at position >= 1 is dropped; a
        hypothesis of length <= 1 becomes empty."""
        assert isinstance(hyp, list)
        if self.model_name == 'blstm':                         # tester.py:191-193
            return [i for i in hyp if i < self.eos_id]
        if len(hyp) <= 1:
            return []
        for pos in range(1, len(hyp)):
            if hyp[pos] == self.eos_id:
                return hyp[:pos]
        return hyp

    def batch_greedy_decode(self, xs, ilens, ys, olens):
        if self.model_name == 'blstm':
            # tester.py:216-225: arg-max over ALL T' frames of the padded batch (frames past enc_lens included, as the
            # reference does), trim, collapse repeats, drop blanks
            from itertools import groupby
            logits, _ = self.asr_model(xs, ilens)
            preds = torch.argmax(logits, dim=-1).cpu()
            for pred, y in zip(preds, ys):
                hyp = [x[0] for x in groupby(self.trim(pred.tolist()))]
                self.write_hyp(y.tolist(), [x for x in hyp if x != self.blank_id])
            return True
        preds = self.asr_model.recog(xs, ilens).transpose(0, 1).cpu()
        for pred, y in zip(preds, ys):
            self.write_hyp(y.tolist(), self.trim(pred.tolist()))
        return True

    def write_hyp(self, y, hyp):
        if getattr(self, '_skip_lines', 0) > 0:                  # utterance already in best-hyp (resumed inside a batch)
            self._skip_lines -= 1
            return
        with open(Path(self.decode_dir, 'best-hyp'), 'a') as fout:
            fout.write("{}\t{}\n".format(" ".join(str(i) for i in y), " ".join(str(i) for i in hyp)))

    def batch_beam_decode(self, xs, ilens, ys, olens):
        hyps, _ = self.asr_model.beam_decode(xs, ilens, self.beam_size, self.min_step_ratio, self.max_step_ratio,
                                             self.att_weight, self.ctc_weight)
        for hyp, y in zip(hyps, ys):
            self.write_hyp(y.tolist(), hyp)
        return True

    def batch_lm_beam_decode(self, xs, ilens, ys, olens):
        hyps, _ = self.asr_model.lm_beam_decode(xs, ilens, self.beam_size, self.lm, self.lm_weight, self.min_step_ratio, self.max_step_ratio)
        for hyp, y in zip(hyps, ys):
            self.write_hyp(y.tolist(), hyp)
        return True

    def batch_ctc_beam_decode(self, xs, ilens, ys, olens):
        for nbest, y in zip(self.asr_model.ctc_beam_decode(xs, ilens, self.beam_size), ys):
            hyp = nbest[0][0]
            # (the search never emits blank or eos, so the BLSTM's trim changes nothing; it is applied to keep the Tester's contract)
            self.write_hyp(y.tolist(), self.trim(hyp) if self.model_name == 'blstm' else hyp)
        return True

    def batch_lm_ctc_beam_decode(self, xs, ilens, ys, olens):
        if self.model_name == 'blstm':
            lists = self.asr_model.ctc_beam_decode(xs, ilens, self.beam_size, 1, self.lm, self.lm_weight, self.len_bonus)
        else:
            lists = self.asr_model.lm_ctc_beam_decode(xs, ilens, self.beam_size, self.lm, self.lm_weight, self.len_bonus)
        for nbest, y in zip(lists, ys):
            hyp = nbest[0][0]
            self.write_hyp(y.tolist(), self.trim(hyp) if self.model_name == 'blstm' else hyp)
        return True

    def batch_lm_rescore_decode(self, xs, ilens, ys, olens):
        lists = self.asr_model.lm_rescore_decode(xs, ilens, self.beam_size, self.lm, self.lm_weight, self.len_bonus, self.nbest, self.att_weight,
                                                 self.ctc_weight)
        for nbest, y in zip(lists, ys):
            self.write_hyp(y.tolist(), nbest[0][0])
        return True

    def batch_lm_joint_beam_decode(self, xs, ilens, ys, olens):
        lists = self.asr_model.lm_joint_beam_decode(xs, ilens, self.beam_size, self.lm, self.lm_weight, self.len_bonus, self.nbest,
                                                    self.min_step_ratio, self.max_step_ratio, self.att_weight, self.ctc_weight)
        for nbest, y in zip(lists, ys):
            self.write_hyp(y.tolist(), nbest[0][0] if nbest else [])
        return True

    def batch_rescore_decode(self, xs, ilens, ys, olens):
        for nbest, y in zip(self.asr_model.rescore_decode(xs, ilens, self.beam_size, self.nbest, self.att_weight, self.ctc_weight), ys):
            self.write_hyp(y.tolist(), nbest[0][0])
        return True

    def _rescore_settings(self):
        if self.model_name == 'blstm':
            raise NotImplementedError("rescore: attention rescoring needs the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self.nbest = int(bd.get('nbest', self.beam_size))
        if not 1 <= self.nbest <= self.beam_size:
            raise ValueError(f"solver.beam_decode.nbest must be in [1, beam_size], got {self.nbest}")
        self.ctc_weight = self._weight(bd, 'ctc_w', 0.5)
        self.att_weight = self._weight(bd, 'att_w', 1.0 - self.ctc_weight)
        if not self.att_weight > 0.0:
            raise ValueError(f"solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got {self.att_weight}")
        if not self.asr_model.engine.ctc_weight > 0.0:
            raise ValueError("decode_mode 'rescore' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
                             "use --decode_mode beam or greedy")

    def _beam_size(self):
        bd = self.config.get('solver', {}).get('beam_decode')
        if not isinstance(bd, dict) or 'beam_size' not in bd:
            raise ValueError(f"decode_mode '{self.decode_mode}' needs a solver.beam_decode block with at least beam_size in the config")
        self.beam_size = int(bd['beam_size'])
        if not 1 <= self.beam_size <= 64:
            raise ValueError(f"solver.beam_decode.beam_size must be in [1, 64], got {self.beam_size}")
        return bd

    def _ctc_beam_settings(self):
        self._beam_size()
        if self.model_name != 'blstm' and not self.asr_model.engine.ctc_weight > 0.0:
            raise ValueError("decode_mode 'ctc_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
                             "use --decode_mode beam or greedy")

    def _lm_beam_settings(self):
        lm_path = getattr(self.paras, 'lm_model_path', None)
        if lm_path is None:
            raise NotImplementedError("lm_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)")
        if self.model_name == 'blstm':
            raise NotImplementedError("lm_beam: LM fusion is only implemented for the transformer's attention beam; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self.min_step_ratio = float(bd.get('min_step_ratio', 0.0))
        self.max_step_ratio = float(bd.get('max_step_ratio', 1.0))
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        ctc_w = self._weight(bd, 'ctc_w', 0.0)
        if ctc_w > 0.0:
            if self.asr_model.engine.ctc_weight > 0.0:
                raise ValueError(f"lm_beam: the LM is not fused into the joint CTC/attention beam (beam_decode.ctc_w = {bd['ctc_w']}); "
                                 "set beam_decode.ctc_w: 0 to fuse it into the attention beam, or use --decode_mode beam without an LM")
            logger.notice(f"beam_decode.ctc_w = {bd['ctc_w']} ignored: this model has no CTC head")
        from .lm import NGramLM
        self.lm = NGramLM.from_arpa(lm_path, self.id2ch, self.sos_id, self.eos_id)
        logger.notice(f"LM shallow fusion: {lm_path}, order {self.lm.order}, n-grams {' / '.join(str(c) for c in self.lm.counts)}, "
                      f"lm_w = {self.lm_weight}")

    def _lm_joint_settings(self):
        """lm_joint_beam: the path, the model, then every setting -- all before anything is decoded"""
        lm_path = getattr(self.paras, 'lm_model_path', None)
        if lm_path is None:
            raise NotImplementedError("lm_joint_beam: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)")
        if self.model_name == 'blstm':
            raise NotImplementedError("lm_joint_beam: the joint CTC/attention beam needs the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode lm_ctc_beam, ctc_beam or greedy")
        bd = self._beam_size()
        if not self.asr_model.engine.ctc_weight > 0.0:
            raise ValueError("decode_mode 'lm_joint_beam' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or "
                             "absent); use --decode_mode lm_beam, beam or greedy")
        self.min_step_ratio = float(bd.get('min_step_ratio', 0.0))
        self.max_step_ratio = float(bd.get('max_step_ratio', 1.0))
        self.ctc_weight = self._weight(bd, 'ctc_w', 0.0)
        if not self.ctc_weight > 0.0:
            raise ValueError("lm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LM into the attention beam "
                             "alone use --decode_mode lm_beam")
        self.att_weight = self._weight(bd, 'att_w', 1.0 - self.ctc_weight)
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self.len_bonus = float(bd.get('len_bonus', 0.0))
        if not math.isfinite(self.len_bonus):
            raise ValueError(f"solver.beam_decode.len_bonus must be finite, got {bd.get('len_bonus')}")
        self.nbest = int(bd.get('nbest', 1))
        if not 1 <= self.nbest <= self.beam_size:
            raise ValueError(f"solver.beam_decode.nbest must be in [1, beam_size], got {self.nbest}")
        if getattr(self, 'lm', None) is None or getattr(self, '_lm_path', None) != lm_path:
            from .lm import NGramLM
            self.lm = NGramLM.from_arpa(lm_path, self.id2ch, self.sos_id, self.eos_id)
            self._lm_path = lm_path
        logger.notice(f"Joint CTC/attention beam with LM: {lm_path}, order {self.lm.order}, n-grams {' / '.join(str(c) for c in self.lm.counts)}, "
                      f"att_w = {self.att_weight}, ctc_w = {self.ctc_weight}, lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}, "
                      f"nbest = {self.nbest}")

    def _lm_ctc_settings(self):
        """lm_ctc_beam and lm_rescore: the path, the model, then every setting -- all before anything is decoded"""
        mode = self.decode_mode
        lm_path = getattr(self.paras, 'lm_model_path', None)
        if lm_path is None:
            raise NotImplementedError(f"{mode}: no language model given; pass --lm_model_path (an ARPA n-gram file over the output units)")
        if mode == 'lm_rescore':
            self._rescore_settings()                             # (BLSTM: NotImplementedError; no CTC head: ValueError; nbest, att_w, ctc_w)
        else:
            self._beam_size()
            if self.model_name != 'blstm' and not self.asr_model.engine.ctc_weight > 0.0:
                raise ValueError(f"decode_mode '{mode}' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or "
                                 "absent); use --decode_mode lm_beam, beam or greedy")
            if self.model_name == 'blstm' and self.blank_id != 0:
                raise ValueError(f"decode_mode '{mode}' needs the blank at id 0 (its slot serves as the LM's <s>), got {self.blank_id}")
        bd = self.config['solver']['beam_decode']
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self.len_bonus = float(bd.get('len_bonus', 0.0))
        if not math.isfinite(self.len_bonus):
            raise ValueError(f"solver.beam_decode.len_bonus must be finite, got {bd.get('len_bonus')}")
        if getattr(self, 'lm', None) is None or getattr(self, '_lm_path', None) != lm_path:
            from .lm import NGramLM
            self.lm = NGramLM.from_arpa(lm_path, self.id2ch, 0, len(self.id2ch) - 1)       # <s> = 0 (the BLSTM's <blank> slot), </s> last
            self._lm_path = lm_path
        logger.notice(f"LM-fused CTC beam: {lm_path}, order {self.lm.order}, n-grams {' / '.join(str(c) for c in self.lm.counts)}, "
                      f"lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}")

    def _beam_settings(self):
        if self.model_name == 'blstm':
            raise NotImplementedError("beam: beam search is only implemented for the transformer (the reference's BLSTM beam "
                                      "decoder is dead code, DESIGN 9); use --decode_mode greedy")
        bd = self._beam_size()
        self.min_step_ratio = float(bd.get('min_step_ratio', 0.0))
        self.max_step_ratio = float(bd.get('max_step_ratio', 1.0))
        ctc_w = self._weight(bd, 'ctc_w', 0.0)
        att_w = self._weight(bd, 'att_w', 1.0 - ctc_w)
        self.att_weight, self.ctc_weight = 1.0, 0.0                 # attention decoder alone (masr_recog_beam)
        if self.asr_model.engine.ctc_weight > 0.0:
            if ctc_w > 0.0:
                self.att_weight, self.ctc_weight = att_w, ctc_w
                logger.notice(f"Joint CTC/attention beam decoding: att_w = {att_w}, ctc_w = {ctc_w}")
            elif 'att_w' in bd:
                logger.notice(f"beam_decode.att_w = {bd['att_w']} ignored: beam_decode.ctc_w is absent or 0, so the beam runs on the "
                              "attention decoder alone and this model's CTC head is not used")
        else:
            if ctc_w > 0.0:
                logger.notice(f"beam_decode.ctc_w = {bd['ctc_w']} ignored: this model has no CTC head")
            if 'att_w' in bd:
                logger.notice(f"beam_decode.att_w = {bd['att_w']} ignored: this model has no CTC head to weigh against the attention decoder")

    @staticmethod
    def _weight(bd, key, default):
        w = float(bd.get(key, default))
        if not math.isfinite(w) or w < 0.0:
            raise ValueError(f"solver.beam_decode.{key} must be finite and >= 0, got {bd.get(key, default)}")
        return w

    def exec(self):
        if self.decode_mode not in ('greedy', 'beam', 'lm_beam', 'ctc_beam', 'rescore', 'lm_ctc_beam', 'lm_rescore', 'lm_joint_beam'):
            raise NotImplementedError(f"{self.decode_mode} haven't supported yet")
        decode = self.batch_greedy_decode
        if self.decode_mode == 'ctc_beam':
            self._ctc_beam_settings()
            decode = self.batch_ctc_beam_decode
            logger.notice(f"Start CTC prefix beam decoding (beam {self.beam_size}): {len(self.eval_set)} batches of <= {self.batch_size}")
        elif self.decode_mode == 'rescore':
            self._rescore_settings()
            decode = self.batch_rescore_decode
            logger.notice(f"Start attention rescoring (CTC beam {self.beam_size}, {self.nbest}-best, att_w = {self.att_weight}, ctc_w = {self.ctc_weight}): "
                          f"{len(self.eval_set)} batches of <= {self.batch_size}")
        elif self.decode_mode in ('lm_ctc_beam', 'lm_rescore'):
            self._lm_ctc_settings()
            decode = self.batch_lm_ctc_beam_decode if self.decode_mode == 'lm_ctc_beam' else self.batch_lm_rescore_decode
            logger.notice(f"Start {'LM-fused CTC prefix beam decoding' if self.decode_mode == 'lm_ctc_beam' else 'attention rescoring of the LM-fused CTC beam'}"
                          f" (beam {self.beam_size}): {len(self.eval_set)} batches of <= {self.batch_size}")
        elif self.decode_mode == 'lm_joint_beam':
            self._lm_joint_settings()
            decode = self.batch_lm_joint_beam_decode
            logger.notice(f"Start joint CTC/attention beam decoding with LM fusion (beam {self.beam_size}): {len(self.eval_set)} batches of "
                          f"<= {self.batch_size}")
        elif self.decode_mode == 'lm_beam':
            self._lm_beam_settings()
            decode = self.batch_lm_beam_decode
            logger.notice(f"Start beam decoding with LM fusion (beam {self.beam_size}): {len(self.eval_set)} batches of <= {self.batch_size}")
        elif self.decode_mode != 'greedy':
            self._beam_settings()
            decode = self.batch_beam_decode
            logger.notice(f"Start beam decoding (beam {self.beam_size}): {len(self.eval_set)} batches of <= {self.batch_size}")
        else:
            logger.notice(f"Start greedy decoding: {len(self.eval_set)} batches of <= {self.batch_size}")
        # --resume: prev_decode_step counts the LINES (utterances) already in best-hyp.  The reference's batch path does not
        # skip at all (tester.py:149-152: a resumed batch decode appends everything again); its per-utterance path skips
        # by step.  Here whole batches are skipped while all their utterances are already written; a partially written
        # batch (killed between two write_hyp calls) is decoded again and only its missing tail is appended.
        done = max(self.prev_decode_step, 0)
        seen = 0
        for idxs in self.eval_set.iter_indices():
            n = len(idxs)
            if seen + n <= done:
                seen += n
                continue
            self._skip_lines = done - seen if seen < done else 0
            decode(*self.eval_set.materialize(idxs))
            seen += n
        self._skip_lines = 0
