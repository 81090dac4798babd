"""Tester: decoding of the test shard into `<log_dir>/<decode_suffix>/best-hyp` (reference: src/tester.py:18-273).
Line format "<ref ids> TAB <hyp ids>" (space separated), `trim` = cut at the first </s> after position 0 -- unchanged, so
translate.py / score.sh of the reference run on these files as they are.  Only the transformer + greedy path exists in the reference
for this model (beam search raises NotImplementedError there, tester.py:121-124); every other `--decode_mode` is this project's GPU
search and writes the best hypothesis of each utterance in the same line format.  All read the config's solver.beam_decode block
(beam_size in [1, 64] is required; every weight must be finite and >= 0, else ValueError) and vet every setting at exec(), before
anything is decoded.  Tester.MODES is the table of them:
  greedy         masr_recog; transformer and BLSTM-CTC.
  beam           masr_recog_beam; transformers (a BLSTM: NotImplementedError).  min_step_ratio (0), max_step_ratio (1).  On a hybrid model
                 (asr_model.ctc_weight > 0) ctc_w > 0 runs the joint CTC/attention search masr_recog_beam_ctc with att_w (default 1 - ctc_w,
                 so ctc_w > 1 without an att_w is refused) and ctc_w.  The weights are checked on every model, hybrid or plain; a plain
                 model with valid weights decodes as before and logs that they are ignored.
  ctc_beam       masr_recog_ctc_beam (BLSTM-CTC: masr_ctc_beam_search per utterance); needs a CTC output layer (a transformer without
                 one: ValueError).
  rescore        masr_recog_rescore, the two-pass decode of DESIGN 5.4: the CTC prefix beam of `ctc_beam`, its nbest (default beam_size, in
                 [1, beam_size]) best re-ranked by att_w * attention score + ctc_w * CTC score after one teacher-forced decoder pass.
                 ctc_w (0.5), att_w (1 - ctc_w, must be > 0).  Hybrid transformers (a BLSTM: NotImplementedError, no head: ValueError).
  lm_beam        masr_recog_beam_lm, the attention beam with an n-gram LM fused in: the ARPA file of `--lm_model_path` over
                 the output units, weighted by lm_w (0.3); the step ratios as for `beam`.  The path is read at exec(): without one
                 the mode raises NotImplementedError (the reference asserts the path when its Tester is constructed); so does a BLSTM.
                 The LM is not fused into the joint beam by this mode: a hybrid model with ctc_w > 0 raises ValueError (that search is
                 `lm_joint_beam`); a plain model logs that ctc_w is ignored.
  nlm_beam       masr_recog_beam_nlm, the attention beam with an LSTM LM fused in: `--lm_model_path` is read as a torch
                 checkpoint of Embedding -> LSTM -> Linear over the output units (nlm.py has the two key layouts; tools/train_nlm.py
                 writes one), weighted by lm_w (0.3); the step ratios as for `beam`; lm_start: sos | eos (sos) is the token the LM is
                 started with (eos: LMs trained with sos = eos).  Without a path the mode raises NotImplementedError; so does a BLSTM.
                 A hybrid model with ctc_w > 0 raises ValueError (set ctc_w: 0; the joint search with this LM is `nlm_joint_beam`); a
                 plain model logs that ctc_w is ignored.
  lm_ctc_beam    masr_recog_ctc_beam_lm (BLSTM-CTC: masr_ctc_beam_search_lm), `ctc_beam` with that LM and a per-token bonus fused into
                 the search: `--lm_model_path` as for `lm_beam`, lm_w (0.3), len_bonus (0, finite, any sign).  Refuses what
                 `ctc_beam` refuses, and a BLSTM whose blank is not id 0 (its slot serves as the LM's <s>).
  lm_rescore     masr_recog_rescore_lm, `rescore` with `lm_ctc_beam`'s search as its first pass: nbest, att_w and ctc_w as for `rescore`, the
                 path, lm_w and len_bonus as for `lm_ctc_beam`.  Refuses what `rescore` refuses.
  lm_joint_beam  masr_recog_beam_ctc_lm, the one-pass joint CTC/attention beam with that LM in the pre-beam and the score, a per-token
                 bonus and an N-best list whose best entry is written: `--lm_model_path` as for `lm_beam`; att_w / ctc_w and
                 the step ratios as for `beam`, with ctc_w > 0 required (absent or 0: ValueError, that search is `lm_beam`); lm_w (0.3),
                 len_bonus (0, finite, any sign), nbest (1, in [1, beam_size]).  No path or a BLSTM raises NotImplementedError, a
                 transformer without a CTC head ValueError.
  nlm_joint_beam masr_recog_beam_ctc_nlm, `lm_joint_beam` with the LSTM LM of `nlm_beam` in the n-gram's place: the LM's term in the
                 pre-beam and the score, a per-token bonus and an N-best list whose best entry is written.  `--lm_model_path` and lm_start
                 as for `nlm_beam`; att_w / ctc_w (ctc_w > 0 required: absent or 0 raises ValueError, that search is `nlm_beam`), the step
                 ratios, lm_w (0.3), len_bonus (0, finite, any sign) and nbest (1, in [1, beam_size]) as for `lm_joint_beam`.  This is where a
                 hybrid model that `nlm_beam` refuses for its ctc_w goes.  No path or a BLSTM raises NotImplementedError, a transformer
                 without a CTC head ValueError, an LM over another number of classes ValueError.
  nlm_ctc_beam   masr_recog_ctc_beam_nlm (BLSTM-CTC: masr_ctc_beam_search_nlm), `lm_ctc_beam` with the LSTM LM of `nlm_beam` in the n-gram's
                 place: the search runs frame by frame and every beam row carries the LM's state.  `--lm_model_path` and
                 lm_start as for `nlm_beam`; beam_size, lm_w (0.3) and len_bonus (0, finite, any sign) as for `lm_ctc_beam`.  Refuses what
                 `lm_ctc_beam` refuses (a BLSTM whose blank is not id 0 included), and an LM over another number of classes (ValueError).
  nlm_rescore    masr_recog_rescore_nlm, `rescore` with `nlm_ctc_beam`'s search as its first pass: nbest, att_w and ctc_w as for `rescore`,
                 the rest as for `nlm_ctc_beam`.  Refuses what `rescore` refuses (a BLSTM: NotImplementedError).
  bias_ctc_beam  masr_recog_ctc_beam_bias (BLSTM-CTC: masr_ctc_beam_search_bias), `ctc_beam` with contextual phrase biasing: the
                 phrases of `--context_path` (one phrase per line as space-separated unit ids, blank lines skipped) are boosted by bias_w
                 (3.0, finite and >= 0) per credited token.  Without a path the mode raises NotImplementedError; a bad file ValueError
                 with its line number.  `--lm_model_path` is optional here: given, the n-gram LM is fused with lm_w / len_bonus as in
                 `lm_ctc_beam`; absent, no LM is fused.  Refuses what `ctc_beam` refuses, and a BLSTM whose blank is not id 0.
  bias_rescore   masr_recog_rescore_bias, `rescore` with `bias_ctc_beam`'s search as its first pass (the attention pass is not biased): nbest,
                 att_w and ctc_w as for `rescore`, the rest as for `bias_ctc_beam`.  Refuses what `rescore` refuses (a BLSTM:
                 NotImplementedError).
  bias_beam      masr_recog_beam_bias, the attention beam (`beam`, with `--lm_model_path` `lm_beam`) with contextual phrase biasing (DESIGN
                 5.14): `--context_path` and bias_w (3.0) as for `bias_ctc_beam`, the step ratios as for `beam`; `--lm_model_path` is optional
                 (given: lm_w as for `lm_beam`).  Without a context path or on a BLSTM the mode raises NotImplementedError.  A hybrid model
                 with ctc_w > 0 raises ValueError (that search is `bias_joint_beam`); a plain model logs that ctc_w is ignored.
  bias_joint_beam masr_recog_beam_ctc_bias, `lm_joint_beam` with the same biasing, with or without its LM: att_w / ctc_w (ctc_w > 0
                 required: absent or 0 raises ValueError, that search is `bias_beam`), the step ratios, len_bonus and nbest as for
                 `lm_joint_beam`; `--context_path` and bias_w as above; `--lm_model_path` optional.  A BLSTM raises NotImplementedError, a
                 transformer without a CTC head ValueError.  The LSTM-LM modes (`nlm_beam`, `nlm_joint_beam`, `nlm_ctc_beam`) are not biased.
  ctc_align      masr_recog_ctc_align (BLSTM-CTC: masr_ctc_align per utterance), the CTC forced alignment of DESIGN 5.9: no search, so no
                 solver.beam_decode block is read.  Each test utterance's REFERENCE transcript is aligned to the frames of the CTC output
                 layer, and one line per utterance is appended to `<decode_dir>/ctc-ali` (no best-hyp is written):
                 "<ref ids> TAB <start:end of each token, space separated> TAB <repr of the path's log-probability as a Python float>",
                 start and end (one past the last) in ENCODER frames -- one encoder frame is 4 input frames on both models.  An utterance
                 with too few frames for its transcript gets an empty middle field and -inf.  `--resume` counts the lines of ctc-ali.
                 Needs a CTC output layer (a transformer without one: ValueError).
  stream_ctc_greedy  masr_stream_*, the streaming first pass of DESIGN 5.16: every batch is fed to the incremental chunk-cached encoder in pieces
                 of `--stream_piece N` input frames (default 4 * the chunk size) and the greedy (best-path) CTC decode that follows the chunks
                 is written.  Needs a chunk size (asr_model.chunk.size or `--decode_chunk`; without one: ValueError) and a CTC output layer (a
                 transformer without one: ValueError); a BLSTM raises NotImplementedError.  No solver.beam_decode block is read.
  stream_ctc_beam    the same stream, then `ctc_beam`'s search (beam_size) on the logits it left behind.  Refuses what `stream_ctc_greedy` does.
  stream_sync_ctc_beam  the same stream with the resumable prefix beam of DESIGN 5.17 following the feeds (masr_stream_beam_open; beam_size): the
                 final result is written, which without an LM and a phrase list is `stream_ctc_beam`'s bit for bit.  `--lm_model_path` (an
                 ARPA file, fused with lm_w 0.3 / len_bonus 0 as in `lm_ctc_beam`) and `--context_path` (phrases boosted by bias_w 3.0 as in
                 `bias_ctc_beam`) are optional, separately or together.  Refuses what `stream_ctc_greedy` does.
The LM modes build the LM once per Tester and (path, <s> id, </s> id).
Every mode of a transformer runs one encoder forward, under the chunk mask of asr_model.chunk where the config has one;
`--decode_chunk SIZE` / `--decode_left N` put their values over its `size` / `left` for this run (SIZE 0: full context), so one checkpoint is
scored at several latencies.  A BLSTM with either flag raises ValueError."""
import math
from pathlib import Path
from shutil import rmtree

import torch

from .io.dataset import get_loader
from .marcos import *  # noqa: F401,F403
from .model import MyTransformer
from .monitor import logger
from .pretrain_interface import load_units


def decode_chunk_policy(model_para, paras, model_name='transformer'):
    """the chunk policy of a --test run: asr_model.chunk with --decode_chunk SIZE / --decode_left N over its size / left, so one checkpoint is
    scored at several latencies (every --decode_mode runs one encoder forward, under `size`).  -> (policy dict or None, overridden?)"""
    from .engine import _chunk_policy, chunk_of
    size, left = getattr(paras, 'decode_chunk', None), getattr(paras, 'decode_left', None)
    if size is None and left is None:
        return (None if model_name == 'blstm' else chunk_of(model_para)), False
    if model_name == 'blstm':
        raise ValueError("--decode_chunk / --decode_left: transformer only")
    if size is not None and size < 0:
        raise ValueError(f"--decode_chunk must be >= 0 (encoder frames; 0 = full context), got {size}")
    if left is not None and left < -1:
        raise ValueError(f"--decode_left must be >= -1 (-1 = every earlier chunk), got {left}")
    pol = dict(chunk_of(model_para) or {"size": 0, "left": -1, "dynamic": 0})
    if size is not None:
        pol["size"] = int(size)
    if left is not None:
        pol["left"] = int(left)
    if pol["size"] == 0 and left is not None:
        raise ValueError("--decode_left needs a chunk: pass --decode_chunk SIZE or set asr_model.chunk.size")
    return _chunk_policy(pol, "--decode_chunk / --decode_left"), True


STREAM_MODES = ('stream_ctc_greedy', 'stream_ctc_beam', 'stream_sync_ctc_beam')


def _no_ctc_head_error(mode, instead):
    return ValueError(f"decode_mode '{mode}' needs a CTC output layer: this transformer has none (asr_model.ctc_weight is 0 or absent); "
                      f"use --decode_mode {instead}")


def stream_decode_args(model_para, paras, mode, chunk_policy, model_name='transformer'):
    """the argument errors of the streaming modes (before any I/O) -> the input frames per feed, --stream_piece or 4 * the chunk size"""
    from .engine import ctc_weight_of
    if model_name == 'blstm':
        raise NotImplementedError(f"{mode}: the streaming first pass runs the transformer's chunk-masked encoder, the BLSTM has none; "
                                  "use --decode_mode ctc_beam or greedy")
    if not chunk_policy or chunk_policy['size'] <= 0:
        raise ValueError(f"{mode}: no chunk size; pass --decode_chunk SIZE or set asr_model.chunk.size")
    if not ctc_weight_of(model_para) > 0.0:
        raise _no_ctc_head_error(mode, "beam or greedy")
    piece = getattr(paras, 'stream_piece', None)
    if piece is not None and piece < 1:
        raise ValueError(f"--stream_piece must be >= 1 (input frames per feed), got {piece}")
    return int(piece) if piece is not None else 4 * chunk_policy['size']


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
        self.chunk_policy, self.chunk_override = decode_chunk_policy(config['asr_model'], paras, self.model_name)   # (argument errors before any I/O)
        self.chunk_last = None                                     # the chunk the last batch's encoder ran with (engine.chunk_last)
        if self.decode_mode in STREAM_MODES:
            self.stream_piece = stream_decode_args(config['asr_model'], paras, self.decode_mode, self.chunk_policy, self.model_name)
        if not paras.resume:
            if self.decode_dir.exists():
                assert paras.overwrite, f"Path exists ({self.decode_dir}). Use --overwrite or change decode suffix"
                rmtree(self.decode_dir)
            self.decode_dir.mkdir(parents=True)
            self.prev_decode_step = -1
        else:
            with open(Path(self.decode_dir, 'ctc-ali' if self.decode_mode == 'ctc_align' else 'best-hyp')) as f:
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
        if self.chunk_override:
            self.asr_model.engine.set_chunk(self.chunk_policy)
        if self.chunk_policy:
            logger.notice(f"encoder self-attention under a chunk of {self.chunk_policy['size']} encoder frames, left {self.chunk_policy['left']}")

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

    def _append(self, name, *fields):
        if getattr(self, '_skip_lines', 0) > 0:                  # utterance already in the file (resumed inside a batch)
            self._skip_lines -= 1
            return
        with open(Path(self.decode_dir, name), 'a') as fout:
            fout.write("\t".join(fields) + "\n")

    def write_hyp(self, y, hyp):
        self._append('best-hyp', " ".join(str(i) for i in y), " ".join(str(i) for i in hyp))

    def batch_ctc_align(self, xs, ilens, ys, olens):
        """ctc-ali: the reference transcript, each token's start:end in encoder frames, the path's log-probability"""
        ys = [y[:int(n)] for y, n in zip(ys, olens)]
        for y, (score, segs, _) in zip(ys, self.asr_model.ctc_align(xs, ilens, ys, olens)):
            self._append('ctc-ali', " ".join(str(i) for i in y.tolist()), " ".join(f"{st}:{en}" for _, st, en in segs), repr(float(score)))
        return True

    # ------------------------------------------------------------------ settings: what the modes' vetting shares
    def _beam_size(self):
        bd = self.config.get('solver', {}).get('beam_decode')
        if not isinstance(bd, dict) or 'beam_size' not in bd:
            raise ValueError(f"decode_mode '{self.decode_mode}' needs a solver.beam_decode block with at least beam_size in the config")
        self.beam_size = int(bd['beam_size'])
        if not 1 <= self.beam_size <= 64:
            raise ValueError(f"solver.beam_decode.beam_size must be in [1, 64], got {self.beam_size}")
        return bd

    @staticmethod
    def _weight(bd, key, default):
        w = float(bd.get(key, default))
        if not math.isfinite(w) or w < 0.0:
            raise ValueError(f"solver.beam_decode.{key} must be finite and >= 0, got {bd.get(key, default)}")
        return w

    def _lm_model_path(self, what="an ARPA n-gram file over the output units"):
        path = getattr(self.paras, 'lm_model_path', None)
        if path is None:
            raise NotImplementedError(f"{self.decode_mode}: no language model given; pass --lm_model_path ({what})")
        return path

    def _need_ctc_head(self, mode, instead):
        if not self.asr_model.engine.ctc_weight > 0.0:
            raise _no_ctc_head_error(mode, instead)

    def _step_ratios(self, bd):
        self.min_step_ratio = float(bd.get('min_step_ratio', 0.0))
        self.max_step_ratio = float(bd.get('max_step_ratio', 1.0))

    def _len_bonus(self, bd):
        self.len_bonus = float(bd.get('len_bonus', 0.0))
        if not math.isfinite(self.len_bonus):
            raise ValueError(f"solver.beam_decode.len_bonus must be finite, got {bd.get('len_bonus')}")

    def _nbest(self, bd, default):
        self.nbest = int(bd.get('nbest', default))
        if not 1 <= self.nbest <= self.beam_size:
            raise ValueError(f"solver.beam_decode.nbest must be in [1, beam_size], got {self.nbest}")

    def _load_lm(self, path, sos, eos):
        """self.lm = the ARPA file as an NGramLM with <s> / </s> at the ids sos / eos, built once per Tester and (path, sos, eos) -> what the
        modes' log lines say about it"""
        key = (path, sos, eos)
        if getattr(self, 'lm', None) is None or getattr(self, '_lm_key', None) != key:
            from .lm import NGramLM
            self.lm, self._lm_key = NGramLM.from_arpa(path, self.id2ch, sos, eos), key
        return f"{path}, order {self.lm.order}, n-grams {' / '.join(str(c) for c in self.lm.counts)}"

    # ------------------------------------------------------------------ settings per mode: everything is vetted before anything is decoded
    def _beam_settings(self):
        if self.model_name == 'blstm':
            raise NotImplementedError("beam: beam search is only implemented for the transformer (the reference's BLSTM beam "
                                      "decoder is dead code, DESIGN 9); use --decode_mode greedy")
        bd = self._beam_size()
        self._step_ratios(bd)
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

    def _lm_beam_settings(self):
        lm_path = self._lm_model_path()
        if self.model_name == 'blstm':
            raise NotImplementedError("lm_beam: LM fusion is only implemented for the transformer's attention beam; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self._step_ratios(bd)
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        if self._weight(bd, 'ctc_w', 0.0) > 0.0:
            if self.asr_model.engine.ctc_weight > 0.0:
                raise ValueError(f"lm_beam: the LM is not fused into the joint CTC/attention beam (beam_decode.ctc_w = {bd['ctc_w']}); "
                                 "set beam_decode.ctc_w: 0 to fuse it into the attention beam, or use --decode_mode beam without an LM")
            logger.notice(f"beam_decode.ctc_w = {bd['ctc_w']} ignored: this model has no CTC head")
        logger.notice(f"LM shallow fusion: {self._load_lm(lm_path, self.sos_id, self.eos_id)}, lm_w = {self.lm_weight}")

    @staticmethod
    def _lm_start(bd):
        start = bd.get('lm_start', 'sos')
        if start not in ('sos', 'eos'):
            raise ValueError(f"solver.beam_decode.lm_start must be sos or eos, got {start!r}")
        return start

    def _load_nlm(self, path, start, mode):
        """self.nlm = the checkpoint as an LstmLM started with the token `start` (sos | eos), built once per Tester and (path, start id); one
        over another number of classes than the model's is refused under `mode`'s name -> what the modes' log lines say about it"""
        key = (path, self.sos_id if start == 'sos' else self.eos_id)
        if getattr(self, 'nlm', None) is None or getattr(self, '_nlm_key', None) != key:
            from .nlm import LstmLM
            self.nlm, self._nlm_key = LstmLM.load(path, start_id=key[1]), key
        if self.nlm.C != len(self.id2ch):
            raise ValueError(f"{mode}: the LSTM LM has {self.nlm.C} classes, the model {len(self.id2ch)} output units")
        return f"{path}, {self.nlm.L} x {self.nlm.H} LSTM on {self.nlm.E}-dim embeddings"

    def _nlm_beam_settings(self):
        lm_path = self._lm_model_path("a torch checkpoint of an LSTM LM over the output units")
        if self.model_name == 'blstm':
            raise NotImplementedError("nlm_beam: LM fusion is only implemented for the transformer's attention beam; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self._step_ratios(bd)
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        start = self._lm_start(bd)
        if self._weight(bd, 'ctc_w', 0.0) > 0.0:
            if self.asr_model.engine.ctc_weight > 0.0:
                raise ValueError(f"nlm_beam: the LSTM LM is not fused into the joint CTC/attention beam (beam_decode.ctc_w = {bd['ctc_w']}); "
                                 "set beam_decode.ctc_w: 0 to fuse it into the attention beam, or use --decode_mode beam without an LM")
            logger.notice(f"beam_decode.ctc_w = {bd['ctc_w']} ignored: this model has no CTC head")
        lm = self._load_nlm(lm_path, start, 'nlm_beam')
        logger.notice(f"LSTM LM shallow fusion: {lm}, start token {start}, lm_w = {self.lm_weight}")

    def _ctc_beam_settings(self):
        self._beam_size()
        if self.model_name != 'blstm':
            self._need_ctc_head('ctc_beam', "beam or greedy")

    def _stream_settings(self):
        """stream_ctc_greedy, stream_ctc_beam and stream_sync_ctc_beam (their argument errors: stream_decode_args, in the constructor)"""
        if self.decode_mode != 'stream_ctc_greedy':
            self._beam_size()
        self._need_ctc_head(self.decode_mode, "beam or greedy")
        if self.decode_mode != 'stream_sync_ctc_beam':
            return
        # the resumable beam's optional LM and phrase list, as bias_ctc_beam reads them
        bd = self.config['solver']['beam_decode']
        lm_path, ctx_path = getattr(self.paras, 'lm_model_path', None), getattr(self.paras, 'context_path', None)
        self.lm_weight, self.len_bonus, self.bias_weight = 0.0, 0.0, 0.0
        lm, bias = "no LM", "no phrase list"
        if lm_path is not None:
            self.lm_weight = self._weight(bd, 'lm_w', 0.3)
            self._len_bonus(bd)
            lm = f"{self._load_lm(lm_path, 0, len(self.id2ch) - 1)}, lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}"
        else:
            self.lm = None
        if ctx_path is not None:
            self.bias_weight = self._weight(bd, 'bias_w', 3.0)
            bias = f"phrase list {self._load_bias(ctx_path)}, bias_w = {self.bias_weight}"
        else:
            self.bias = None
        logger.notice(f"stream_sync_ctc_beam: {lm}; {bias}")

    def _ctc_align_settings(self):
        if self.model_name != 'blstm':
            self._need_ctc_head('ctc_align', "greedy or beam to decode instead")

    def _rescore_settings(self):
        if self.model_name == 'blstm':
            raise NotImplementedError("rescore: attention rescoring needs the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self._nbest(bd, self.beam_size)
        self.ctc_weight = self._weight(bd, 'ctc_w', 0.5)
        self.att_weight = self._weight(bd, 'att_w', 1.0 - self.ctc_weight)
        if not self.att_weight > 0.0:
            raise ValueError(f"solver.beam_decode.att_w must be > 0 for decode_mode 'rescore', got {self.att_weight}")
        self._need_ctc_head('rescore', "beam or greedy")

    def _lm_ctc_settings(self):
        """lm_ctc_beam and lm_rescore"""
        mode = self.decode_mode
        lm_path = self._lm_model_path()
        if mode == 'lm_rescore':
            self._rescore_settings()                             # (BLSTM: NotImplementedError; no CTC head: ValueError; nbest, att_w, ctc_w)
        else:
            self._beam_size()
            if self.model_name != 'blstm':
                self._need_ctc_head(mode, "lm_beam, beam or greedy")
            elif self.blank_id != 0:
                raise ValueError(f"decode_mode '{mode}' needs the blank at id 0 (its slot serves as the LM's <s>), got {self.blank_id}")
        bd = self.config['solver']['beam_decode']
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self._len_bonus(bd)
        lm = self._load_lm(lm_path, 0, len(self.id2ch) - 1)         # <s> = 0 (the BLSTM's <blank> slot), </s> last
        logger.notice(f"LM-fused CTC beam: {lm}, lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}")

    def _nlm_ctc_settings(self):
        """nlm_ctc_beam and nlm_rescore: _lm_ctc_settings' searches with _nlm_beam_settings' LM"""
        mode = self.decode_mode
        lm_path = self._lm_model_path("a torch checkpoint of an LSTM LM over the output units")
        if mode == 'nlm_rescore':
            self._rescore_settings()                             # (BLSTM: NotImplementedError; no CTC head: ValueError; nbest, att_w, ctc_w)
        else:
            self._beam_size()
            if self.model_name != 'blstm':
                self._need_ctc_head(mode, "nlm_beam, beam or greedy")
            elif self.blank_id != 0:
                raise ValueError(f"decode_mode '{mode}' needs the blank at id 0 (the search never emits class 0), got {self.blank_id}")
        bd = self.config['solver']['beam_decode']
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self._len_bonus(bd)
        start = self._lm_start(bd)
        lm = self._load_nlm(lm_path, start, mode)
        logger.notice(f"LSTM-LM-fused CTC beam: {lm}, start token {start}, lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}")

    def _lm_joint_settings(self):
        lm_path = self._lm_model_path()
        if self.model_name == 'blstm':
            raise NotImplementedError("lm_joint_beam: the joint CTC/attention beam needs the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode lm_ctc_beam, ctc_beam or greedy")
        bd = self._beam_size()
        self._need_ctc_head('lm_joint_beam', "lm_beam, beam or greedy")
        self._step_ratios(bd)
        self.ctc_weight = self._weight(bd, 'ctc_w', 0.0)
        if not self.ctc_weight > 0.0:
            raise ValueError("lm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LM into the attention beam "
                             "alone use --decode_mode lm_beam")
        self.att_weight = self._weight(bd, 'att_w', 1.0 - self.ctc_weight)
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self._len_bonus(bd)
        self._nbest(bd, 1)
        lm = self._load_lm(lm_path, self.sos_id, self.eos_id)
        logger.notice(f"Joint CTC/attention beam with LM: {lm}, att_w = {self.att_weight}, ctc_w = {self.ctc_weight}, lm_w = {self.lm_weight}, "
                      f"len_bonus = {self.len_bonus}, nbest = {self.nbest}")

    def _nlm_joint_settings(self):
        """_lm_joint_settings' search with _nlm_beam_settings' LM"""
        lm_path = self._lm_model_path("a torch checkpoint of an LSTM LM over the output units")
        if self.model_name == 'blstm':
            raise NotImplementedError("nlm_joint_beam: the joint CTC/attention beam needs the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode ctc_beam or greedy")
        bd = self._beam_size()
        self._need_ctc_head('nlm_joint_beam', "nlm_beam, beam or greedy")
        self._step_ratios(bd)
        self.ctc_weight = self._weight(bd, 'ctc_w', 0.0)
        if not self.ctc_weight > 0.0:
            raise ValueError("nlm_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to fuse the LSTM LM into the attention "
                             "beam alone use --decode_mode nlm_beam")
        self.att_weight = self._weight(bd, 'att_w', 1.0 - self.ctc_weight)
        self.lm_weight = self._weight(bd, 'lm_w', 0.3)
        self._len_bonus(bd)
        self._nbest(bd, 1)
        start = self._lm_start(bd)
        lm = self._load_nlm(lm_path, start, 'nlm_joint_beam')
        logger.notice(f"Joint CTC/attention beam with LSTM LM: {lm}, start token {start}, att_w = {self.att_weight}, ctc_w = {self.ctc_weight}, "
                      f"lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}, nbest = {self.nbest}")

    def _load_bias(self, path):
        """self.bias = the phrase file as a ContextBias over the output units, built once per Tester and path"""
        if getattr(self, 'bias', None) is None or getattr(self, '_bias_key', None) != path:
            from .bias import ContextBias
            self.bias, self._bias_key = ContextBias.from_file(path, len(self.id2ch)), path
        return f"{path}, {self.bias.phrases} phrases"

    def _bias_ctc_settings(self):
        """bias_ctc_beam and bias_rescore: ctc_beam's / rescore's settings, the phrase list, and lm_ctc_beam's LM when a path is given"""
        mode = self.decode_mode
        ctx_path = getattr(self.paras, 'context_path', None)
        if ctx_path is None:
            raise NotImplementedError(f"{mode}: no phrase list given; pass --context_path (one phrase per line as space-separated unit ids)")
        if mode == 'bias_rescore':
            self._rescore_settings()                             # (BLSTM: NotImplementedError; no CTC head: ValueError; nbest, att_w, ctc_w)
        else:
            self._beam_size()
            if self.model_name != 'blstm':
                self._need_ctc_head(mode, "beam or greedy")
            elif self.blank_id != 0:
                raise ValueError(f"decode_mode '{mode}' needs the blank at id 0 (the search never emits class 0), got {self.blank_id}")
        bd = self.config['solver']['beam_decode']
        self.bias_weight = self._weight(bd, 'bias_w', 3.0)
        lm_path = getattr(self.paras, 'lm_model_path', None)
        self.lm_weight, self.len_bonus = 0.0, 0.0
        lm = "no LM"
        if lm_path is not None:
            self.lm_weight = self._weight(bd, 'lm_w', 0.3)
            self._len_bonus(bd)
            lm = f"{self._load_lm(lm_path, 0, len(self.id2ch) - 1)}, lm_w = {self.lm_weight}, len_bonus = {self.len_bonus}"
        else:
            self.lm = None
        logger.notice(f"{mode}: phrase list {self._load_bias(ctx_path)}, bias_w = {self.bias_weight}; {lm}")

    def _bias_step_settings(self):
        """bias_beam and bias_joint_beam: beam's / lm_joint_beam's settings, the phrase list, and lm_beam's LM when a path is given"""
        mode = self.decode_mode
        ctx_path = getattr(self.paras, 'context_path', None)
        if ctx_path is None:
            raise NotImplementedError(f"{mode}: no phrase list given; pass --context_path (one phrase per line as space-separated unit ids)")
        if self.model_name == 'blstm':
            raise NotImplementedError(f"{mode}: the attention and joint beams need the transformer's decoder, the BLSTM has none; "
                                      "use --decode_mode bias_ctc_beam")
        bd = self._beam_size()
        self._step_ratios(bd)
        ctc_w = self._weight(bd, 'ctc_w', 0.0)
        if mode == 'bias_beam':
            if ctc_w > 0.0:
                if self.asr_model.engine.ctc_weight > 0.0:
                    raise ValueError(f"bias_beam: this search is the attention beam alone (beam_decode.ctc_w = {bd['ctc_w']}); the phrase-biased "
                                     "joint CTC/attention beam is --decode_mode bias_joint_beam, or set beam_decode.ctc_w: 0")
                logger.notice(f"beam_decode.ctc_w = {bd['ctc_w']} ignored: this model has no CTC head")
        else:
            self._need_ctc_head(mode, "bias_beam, beam or greedy")
            self.ctc_weight = ctc_w
            if not ctc_w > 0.0:
                raise ValueError("bias_joint_beam: solver.beam_decode.ctc_w must be > 0 (it is absent or 0); to bias the attention beam alone use "
                                 "--decode_mode bias_beam")
            self.att_weight = self._weight(bd, 'att_w', 1.0 - ctc_w)
            self._nbest(bd, 1)
        self.bias_weight = self._weight(bd, 'bias_w', 3.0)
        lm_path = getattr(self.paras, 'lm_model_path', None)
        self.lm_weight, self.len_bonus = 0.0, 0.0
        if mode == 'bias_joint_beam':
            self._len_bonus(bd)                                  # (the bonus needs no LM)
        lm = "no LM"
        if lm_path is not None:
            self.lm_weight = self._weight(bd, 'lm_w', 0.3)
            lm = f"{self._load_lm(lm_path, self.sos_id, self.eos_id)}, lm_w = {self.lm_weight}"
        else:
            self.lm = None
        logger.notice(f"{mode}: phrase list {self._load_bias(ctx_path)}, bias_w = {self.bias_weight}; {lm}")

    # ------------------------------------------------------------------ the decode modes
    def _ctc_best(self, lists):
        """the best entry of each N-best list of a CTC beam (the search never emits blank or eos, so the BLSTM's trim changes nothing; it is
        applied to keep the Tester's contract)"""
        return [self.trim(n[0][0]) if self.model_name == 'blstm' else n[0][0] for n in lists]

    def _fused_ctc_beam_lists(self, mode, lm, xs, ilens, **bias):
        """the N-best lists of lm_ctc_beam, nlm_ctc_beam and bias_ctc_beam (`bias`: its bias and bias_weight): a BLSTM runs them all through
        ctc_beam_decode, per utterance; a transformer through the mode's own <mode>_decode, which takes the phrase list in front of the LM"""
        if self.model_name == 'blstm':
            return self.asr_model.ctc_beam_decode(xs, ilens, self.beam_size, 1, lm, self.lm_weight, self.len_bonus, **bias)
        return getattr(self.asr_model, mode + '_decode')(xs, ilens, self.beam_size, *bias.values(), lm, self.lm_weight, self.len_bonus)

    # mode -> (its settings function, (Tester, xs, ilens) -> the best hypothesis of each utterance, Tester -> what the start-up line names);
    # greedy has neither settings nor such a function: batch_greedy_decode writes its lines itself; nor has ctc_align, which reads the
    # references too and writes ctc-ali (batch_ctc_align).  _fused_ctc_beam_lists is reached through the class: `t` need only carry what it reads
    MODES = {
        'greedy': (None, None, lambda t: "greedy decoding"),
        'beam': (_beam_settings,
                 lambda t, xs, il: t.asr_model.beam_decode(xs, il, t.beam_size, t.min_step_ratio, t.max_step_ratio, t.att_weight, t.ctc_weight)[0],
                 lambda t: f"beam decoding (beam {t.beam_size})"),
        'lm_beam': (_lm_beam_settings,
                    lambda t, xs, il: t.asr_model.lm_beam_decode(xs, il, t.beam_size, t.lm, t.lm_weight, t.min_step_ratio, t.max_step_ratio)[0],
                    lambda t: f"beam decoding with LM fusion (beam {t.beam_size})"),
        'nlm_beam': (_nlm_beam_settings,
                     lambda t, xs, il: t.asr_model.nlm_beam_decode(xs, il, t.beam_size, t.nlm, t.lm_weight, t.min_step_ratio, t.max_step_ratio)[0],
                     lambda t: f"beam decoding with LSTM LM fusion (beam {t.beam_size})"),
        'ctc_beam': (_ctc_beam_settings,
                     lambda t, xs, il: t._ctc_best(t.asr_model.ctc_beam_decode(xs, il, t.beam_size)),
                     lambda t: f"CTC prefix beam decoding (beam {t.beam_size})"),
        'rescore': (_rescore_settings,
                    lambda t, xs, il: [n[0][0] for n in t.asr_model.rescore_decode(xs, il, t.beam_size, t.nbest, t.att_weight, t.ctc_weight)],
                    lambda t: f"attention rescoring (CTC beam {t.beam_size}, {t.nbest}-best, att_w = {t.att_weight}, ctc_w = {t.ctc_weight})"),
        'lm_ctc_beam': (_lm_ctc_settings,
                        lambda t, xs, il: t._ctc_best(Tester._fused_ctc_beam_lists(t, 'lm_ctc_beam', t.lm, xs, il)),
                        lambda t: f"LM-fused CTC prefix beam decoding (beam {t.beam_size})"),
        'lm_rescore': (_lm_ctc_settings,
                       lambda t, xs, il: [n[0][0] for n in t.asr_model.lm_rescore_decode(xs, il, t.beam_size, t.lm, t.lm_weight, t.len_bonus, t.nbest,
                                                                                         t.att_weight, t.ctc_weight)],
                       lambda t: f"attention rescoring of the LM-fused CTC beam (beam {t.beam_size})"),
        'nlm_ctc_beam': (_nlm_ctc_settings,
                         lambda t, xs, il: t._ctc_best(Tester._fused_ctc_beam_lists(t, 'nlm_ctc_beam', t.nlm, xs, il)),
                         lambda t: f"LSTM-LM-fused CTC prefix beam decoding (beam {t.beam_size})"),
        'nlm_rescore': (_nlm_ctc_settings,
                        lambda t, xs, il: [n[0][0] for n in t.asr_model.nlm_rescore_decode(xs, il, t.beam_size, t.nlm, t.lm_weight, t.len_bonus, t.nbest,
                                                                                           t.att_weight, t.ctc_weight)],
                        lambda t: f"attention rescoring of the LSTM-LM-fused CTC beam (beam {t.beam_size})"),
        'bias_ctc_beam': (_bias_ctc_settings,
                          lambda t, xs, il: t._ctc_best(Tester._fused_ctc_beam_lists(t, 'bias_ctc_beam', t.lm, xs, il, bias=t.bias,
                                                                                     bias_weight=t.bias_weight)),
                          lambda t: f"phrase-biased CTC prefix beam decoding (bias_ctc_beam, beam {t.beam_size}, {t.bias.phrases} phrases)"),
        'bias_rescore': (_bias_ctc_settings,
                         lambda t, xs, il: [n[0][0] for n in t.asr_model.bias_rescore_decode(xs, il, t.beam_size, t.bias, t.bias_weight, t.lm, t.lm_weight,
                                                                                             t.len_bonus, t.nbest, t.att_weight, t.ctc_weight)],
                         lambda t: f"attention rescoring of the phrase-biased CTC beam (bias_rescore, beam {t.beam_size}, {t.bias.phrases} phrases)"),
        'bias_beam': (_bias_step_settings,
                      lambda t, xs, il: t.asr_model.bias_beam_decode(xs, il, t.beam_size, t.bias, t.bias_weight, t.lm, t.lm_weight, t.min_step_ratio,
                                                                     t.max_step_ratio)[0],
                      lambda t: f"phrase-biased beam decoding (bias_beam, beam {t.beam_size}, {t.bias.phrases} phrases)"),
        'bias_joint_beam': (_bias_step_settings,
                            lambda t, xs, il: [n[0][0] if n else [] for n in t.asr_model.bias_joint_beam_decode(
                                xs, il, t.beam_size, t.bias, t.bias_weight, t.lm, t.lm_weight, t.len_bonus, t.nbest, t.min_step_ratio, t.max_step_ratio,
                                t.att_weight, t.ctc_weight)],
                            lambda t: f"phrase-biased joint CTC/attention beam decoding (bias_joint_beam, beam {t.beam_size}, {t.bias.phrases} phrases)"),
        'ctc_align': (_ctc_align_settings, None, lambda t: "CTC forced alignment of the reference transcripts"),
        'stream_ctc_greedy': (_stream_settings,
                              lambda t, xs, il: [tok for tok, _ in t.asr_model.engine.recog_stream(xs, il, t.stream_piece)],
                              lambda t: f"streaming greedy CTC decoding (chunk {t.chunk_policy['size']}, pieces of {t.stream_piece} frames)"),
        'stream_ctc_beam': (_stream_settings,
                            lambda t, xs, il: t._ctc_best(t.asr_model.engine.recog_stream(xs, il, t.stream_piece, t.beam_size)),
                            lambda t: f"streaming encoder, CTC prefix beam on its logits (chunk {t.chunk_policy['size']}, beam {t.beam_size})"),
        'stream_sync_ctc_beam': (_stream_settings,
                                 lambda t, xs, il: t._ctc_best(t.asr_model.engine.recog_stream(
                                     xs, il, t.stream_piece, t.beam_size, sync_beam=True, lm=t.lm, lm_w=t.lm_weight, len_bonus=t.len_bonus, bias=t.bias,
                                     bias_w=t.bias_weight)[0]),
                                 lambda t: f"streaming encoder, resumable CTC prefix beam following the feeds (chunk {t.chunk_policy['size']}, "
                                           f"beam {t.beam_size})"),
        'lm_joint_beam': (_lm_joint_settings,
                          lambda t, xs, il: [n[0][0] if n else [] for n in t.asr_model.lm_joint_beam_decode(
                              xs, il, t.beam_size, t.lm, t.lm_weight, t.len_bonus, t.nbest, t.min_step_ratio, t.max_step_ratio, t.att_weight, t.ctc_weight)],
                          lambda t: f"joint CTC/attention beam decoding with LM fusion (beam {t.beam_size})"),
        'nlm_joint_beam': (_nlm_joint_settings,
                           lambda t, xs, il: [n[0][0] if n else [] for n in t.asr_model.nlm_joint_beam_decode(
                               xs, il, t.beam_size, t.nlm, t.lm_weight, t.len_bonus, t.nbest, t.min_step_ratio, t.max_step_ratio, t.att_weight, t.ctc_weight)],
                           lambda t: f"joint CTC/attention beam decoding with LSTM LM fusion (beam {t.beam_size})"),
    }

    def exec(self):
        if self.decode_mode not in self.MODES:
            raise NotImplementedError(f"{self.decode_mode} haven't supported yet")
        settings, best_hyps, what = self.MODES[self.decode_mode]
        if settings is not None:
            settings(self)
        logger.notice(f"Start {what(self)}: {len(self.eval_set)} batches of <= {self.batch_size}")
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
            xs, ilens, ys, olens = self.eval_set.materialize(idxs)
            if self.decode_mode == 'ctc_align':
                self.batch_ctc_align(xs, ilens, ys, olens)
            elif best_hyps is None:
                self.batch_greedy_decode(xs, ilens, ys, olens)
            else:
                for hyp, y in zip(best_hyps(self, xs, ilens), ys):
                    self.write_hyp(y.tolist(), hyp)
            if self.model_name != 'blstm':
                self.chunk_last = self.asr_model.engine.chunk_last()
            seen += n
        self._skip_lines = 0
