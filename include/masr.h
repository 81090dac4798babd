/* libmasr -- C ABI of the MI355X-native meta-ASR training path.
 *
 * Drop-in boundary for the hot path of sunprinceS/MetaASR-CrossAccent.
 * The reference has no native code and no FFI: its "operator boundary" is the Python mixin
 * contract  get_trainer(cls, config, paras, id2accent) -> solver with
 * solver.run_batch(idx, x, ilens, ys, olens, train) (src/transformer_torch_trainer.py:13-99)
 * driven by FOMetaASRInterface.run_task/_partial_meta_update/_final_meta_update
 * (src/fo_meta_interface.py:128-250).  Each entry point below names the reference code it
 * replaces.  The Python host mirror (metaasr-crossaccent_amd/) binds these with ctypes; see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only (no torch types).  All device pointers are HIP
 * device memory owned by the caller.  Every call is ordered on the caller's hipStream_t
 * (passed as void*), allocates nothing and never synchronises unless stated.  Return 0 on
 * success, <0 on error (text via masr_last_error()).  A handle is not thread-safe.
 */
#ifndef MASR_H
#define MASR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct masr_model masr_model;

/* asr_model block of the reference YAML (config/transformer/pretrain/fometa-hkust.yaml:13-27)
 * + odim (= len(id2units), src/pretrain_interface.py:38-43) + solver.label_smoothing. */
typedef struct masr_config {
    int32_t idim, odim, d_model, nheads, d_inner, enc_layers, dec_layers;
    int32_t tie_weights;          /* tgt_share_weight != 0 (mono_transformer_torch.py:66-70) */
    float dropout, pos_dropout, label_smoothing;
} masr_config;

#define MASR_TRAIN 1              /* run_batch(train=True): forward + loss + backward            */
#define MASR_EVAL 0               /* run_batch(train=False): forward + loss only (dropout off)   */

int masr_version(void);
const char* masr_last_error(void);

/* MyTransformer.__init__ (mono_transformer_torch.py:37-104): builds the parameter table only. */
masr_model* masr_create(const masr_config* cfg);
/* Extension (the reference's transformer trains on the decoder's CE alone): joint CTC/attention training, ESPnet's `mtlalpha`
 * (YAML asr_model.ctc_weight).  ctc_weight == 0 is exactly masr_create.  0 < w < 1 adds the head ctc.ctc_lo = Linear(d_model -> odim)
 * over the encoder memory (the output of encoder.norm, no dropout), appended behind every other parameter (ctc.ctc_lo.weight
 * [odim][d_model], ctc.ctc_lo.bias [odim]), and masr_run_batch's loss becomes (1 - w) * CE + w * CTC, the CTC term
 * nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) of log_softmax(head logits) with targets y (no sos / eos), input lengths
 * floor(ilens / 4).  Stats are unchanged in layout: out[0] = the joint loss, out[1] / out[2] the decoder's.  Labels must be shorter than
 * 1024 tokens, odim <= 4096.  A w outside [0, 1) returns null. */
masr_model* masr_create_ctc(const masr_config* cfg, float ctc_weight);
void masr_destroy(masr_model* m);

/* Flat fp32 parameter buffer layout = the reference state_dict order without
 * the pos_encoder.pe buffer and, when tied, without pre_embed.weight (alias of char_trans.weight). */
int64_t masr_param_numel(const masr_model* m);
int masr_param_count(const masr_model* m);
int masr_param_info(const masr_model* m, int idx, char* name, int name_cap, int64_t shape[4], int* ndim, int64_t* offset);

/* workspace needed for a batch of B utterances x T frames with L = max(olen)+1 target positions (with a CTC head: its logits, gradient
 * operand and lattice work buffer included; with a SpecAugment policy set: the augmented batch) */
int64_t masr_workspace_bytes(const masr_model* m, int B, int T, int L);
/* params/grads: fp32 [masr_param_numel]; pe: fp32 [3000][d_model] (PositionalEncoding buffer, :16-28) */
int masr_bind(masr_model* m, float* params, float* grads, const float* pe, void* workspace, int64_t ws_bytes);
/* rebuild the bf16 operand shadows after ANY change of params (load_state_dict, optimizer step) */
int masr_refresh(masr_model* m, void* stream);
void masr_set_seed(masr_model* m, uint64_t seed);      /* dropout stream */
/* hint: this model is one of `slots` task slots running concurrently on the GPU (pretrain.py --tasks_per_gpu).  NO result depends on it,
 * bit for bit: no launch partition that enters a summation order follows the slot count (the k-split below follows masr_set_ksplit only;
 * tests/test_hip_engine.py::test_task_slot_hint_never_changes_bits).  What follows it is the LDS footprint of some launches: with slots > 1
 * the encoder-row GEMMs keep a three-stage operand ring (72 KB) instead of four (96 KB), so that the other slots' workgroups still fit
 * beside them on a CU.  Changing it drops captured step graphs (masr_set_step_graphs). */
void masr_set_concurrency(masr_model* m, int slots);
/* the dropout stream's position: state[0] = seed, state[1] = batches run since masr_set_seed (every run_batch derives its masks
 * from both); set != 0 writes it.  For checkpoints: a resumed run continues the mask stream where the saved one stopped. */
void masr_dropout_state(masr_model* m, uint64_t state[2], int set);

/* TransformerTrainer.run_batch (src/transformer_torch_trainer.py:59-99) = MyTransformer.forward
 * (:178-208) + label-smoothed CE (:64-84) + (train) zero_grad/backward.  xs: device fp32 [B][T][idim];
 * ilens/olens/ys_flat: HOST int64 (ys_flat = concatenated labels, sum(olens) entries).  Gradients
 * are left in `grads`.  olens is NOT mutated (quirk Q6 is reproduced by the Python mirror). */
int masr_run_batch(masr_model* m, const float* xs, const int64_t* ilens, const int64_t* ys_flat,
                   const int64_t* olens, int B, int T, int flags, void* stream);
/* Opt-in: a batch shape (B, T, L, flags, xs pointer) that repeats on a non-null stream is captured into
 * a hipGraph on its second consecutive occurrence and replayed afterwards (one launch instead of ~150; tokens, lengths, dropout
 * seed and 1/n_total reach the kernels through the per-step upload, so replays are bit-identical to direct launches).  It cuts
 * the host's enqueue time 6x and leaves the step time unchanged -- the step is GPU-bound -- hence off by default.
 * counters: out[0] = steps launched kernel by kernel, out[1] = graphs captured, out[2] = steps replayed from a graph, out[3] = k-split GEMM
 * launches of the last step launched or captured (0 = whole reductions).  Captured graphs hold the launch geometry of the settings they were
 * captured under: masr_set_concurrency / masr_set_ksplit / masr_set_split_wgrad_launches / masr_set_specaug / masr_set_chunk drop them (after a device synchronisation). */
void masr_set_step_graphs(masr_model* m, int on);
/* The Linear weight gradients of a step are ONE launch (the decoder-row tiles fill the CUs the encoder-row tiles leave idle); on: two
 * launches, encoder rows then decoder rows (A/B; identical bits -- each element of dW is reduced by one workgroup either way). */
void masr_set_split_wgrad_launches(masr_model* m, int on);
/* The decoder's few-row GEMMs with a long reduction (FFN second layer, its first layer's dgrad, the packed q/k/v dgrad: <= 1024 rows, K >= 1024;
 * and the attention out-projections in two halves) run k-split over K / 512 x as many workgroups; the LayerNorm (backward) that follows sums the
 * fp32 partial products and applies the GEMM's epilogue (bias, dropout, residual) on its way in.  It shortens a lone task's launch chain (+1..3 %)
 * and costs throughput beside other task slots, and it changes the fp32 summation order of those GEMMs -- so it follows THIS call only, never
 * masr_set_concurrency.  Default OFF (whole reductions).  The one-task-per-stream loops turn it on (train.py: the mono / multi trainers); the
 * FOMAML interface leaves it off for every --tasks_per_gpu, so that K slots == the sequential run == N ranks, bit for bit.  Both schedules are
 * pinned to the reference at the headline shape (tests/test_hip_fullsize.py).  masr_step_counters out[3] reports which one ran. */
void masr_set_ksplit(masr_model* m, int on);
void masr_step_counters(const masr_model* m, int64_t out[4]);
/* out[0]=loss, out[1]=n_correct, out[2]=n_total, out[3]=last grad norm.  Synchronises the stream. */
int masr_read_stats(masr_model* m, float out[4], void* stream);
/* the same four floats WITHOUT waiting: masr_stats_post queues their copy into a page-locked block owned by the handle (a ring of
   64) and records an event behind it; it returns a ticket >= 0.  masr_stats_wait(ticket) waits for that event (completion and
   host visibility of the copy) and hands the floats out; a ticket may simply be dropped -- its block is only reused after its
   event has completed.  masr_stats_peek returns the block itself, whose four words hold MASR_STATS_PENDING until the copy lands:
   a host thread may poll them without entering the HIP runtime (the task threads are inside its launch path meanwhile) and call
   masr_stats_wait once they have changed.  Tickets EXPIRE after 64 newer posts on the same handle (masr_stats_wait / _peek then fail
   with "unknown or expired ticket"): a caller that keeps more than that outstanding must read the oldest first (the Python engine
   does so at 48).  Lets the host queue the next tasks while these
   run: the reference reads loss / accuracy / norm only for its log lines (fo_meta_interface.py:147-151). */
#define MASR_STATS_PENDING 0x7FC0DEADu            /* a quiet NaN with a payload no kernel produces */
int64_t masr_stats_post(masr_model* m, void* stream);
const float* masr_stats_peek(masr_model* m, int64_t ticket);
int masr_stats_wait(masr_model* m, int64_t ticket, float out[4]);
/* device view of the last forward's logits: fp32 [rows = B*L][ld], first odim columns valid; and gold */
int masr_last_logits(masr_model* m, const float** logits, const int32_t** gold, int* rows, int* L, int* ld);

/* Extension (the reference feeds every utterance as it sits in the shard): SpecAugment (Park et al. 2019) on the training batch, inside the step
 * (YAML asr_model.specaug).  xs fp32 [B][T][D] with raw frame lengths n_b -> out fp32 [B][T][D] in ANOTHER buffer; rows t >= n_b of
 * out are 0.0f whatever xs holds there (the padding of xs is never read); masked cells are 0.0f (the features are mean-normalised).
 * All draws are integers from the step's 32-bit seed: step_seed = (uint32)((seed * 0x9E3779B97F4A7C15) >> 32) + (uint32)step * 7919 (what
 * masr_run_batch forms from masr_dropout_state for its dropout masks), key = the dropout key of (step_seed, site 0x53504147),
 * word(b, j) = the dropout hash word of (key, b * 64 + j), uni(w, r) = (uint64(w) * r) >> 32 in [0, r).  Per utterance b of length n:
 *   warp        only if time_warp = W > 0 and n > 2W: c = W + uni(word(b, 0), n - 2W), c' = c + uni(word(b, 1), 2W - 1) - (W - 1), so 1 <= c' <= n - 2.
 *               Output row t reads source position i + r / den: t < c': num = t c, den = c', i = num / den; else num = (t - c')(n - 1 - c),
 *               den = n - 1 - c', i = c + num / den; r = num % den (integer division).  r == 0: x[i], copied bit for bit; else
 *               x[i] + (float(r) / float(den)) * (x[i + 1] - x[i]) in fp32.  Rows 0 and n - 1 stay; c' == c or no warp: a bit-exact copy.
 *   freq masks  for i < freq_masks: f = uni(word(b, 2 + 2i), min(freq_width, freq_bins) + 1), f0 = uni(word(b, 3 + 2i), freq_bins - f + 1);
 *               feature dims [f0, f0 + f) are zero.  Masks lie inside the first freq_bins dims (80 spares the 3 pitch dims of the 83-dim rows).
 *   time masks  for i < time_masks: cap = min(time_width, (int)floorf(time_ratio * (float)n)) (one fp32 product), tau = uni(word(b, 18 + 2i), cap + 1),
 *               t0 = uni(word(b, 19 + 2i), n - tau + 1); rows [t0, t0 + tau) are zero.  Masks apply after the warp.
 * A policy with time_warp = freq_masks = time_masks = 0 is "off": a plain copy with zeroed padding.
 * Bounds: time_warp >= 0, freq_masks in [0, 8], freq_width >= 0, freq_bins in [1, D], time_masks in [0, 8], time_width >= 0, time_ratio in [0, 1]. */
typedef struct masr_specaug_policy {
    int32_t time_warp, freq_masks, freq_width, freq_bins, time_masks, time_width;
    float time_ratio;
} masr_specaug_policy;
/* the stateless operator: one launch on `stream`; lens_dev int32 [B] on the device (each clamped to [0, T] by the kernel).  -1 with a message for
 * a policy out of bounds, a null pointer, out == xs, B outside [1, 65535], or T so large that T * T or T * D leaves an int. */
int masr_specaug(const float* xs, const int32_t* lens_dev, float* out, int B, int T, int D, const masr_specaug_policy* p, uint64_t seed,
                 uint64_t step, void* stream);
/* the model's policy (null or an all-zero policy: off, the default).  While one is set, every masr_run_batch(MASR_TRAIN) augments its batch as
 * its first launch -- masr_specaug at the (seed, step) masr_dropout_state reports before the call -- and both conv1's forward and conv1's weight
 * gradient read the augmented batch; MASR_EVAL and every masr_recog* never augment.  masr_workspace_bytes grows by B * T * D floats.  The step's seed
 * and the raw ilens travel in the per-step upload, so captured step graphs replay with the current ones.  Changing the policy drops captured step
 * graphs; a policy out of bounds (freq_bins against the model's idim) returns -1 and leaves the old one in place. */
int masr_set_specaug(masr_model* m, const masr_specaug_policy* p);
/* device view of the augmented batch of the last masr_run_batch(MASR_TRAIN) under a policy: fp32 [B][T][D].  -1 if that step did not augment. */
int masr_specaug_last(masr_model* m, const float** xa, int* B, int* T, int* D);

/* Extension (the reference's encoder always attends over the whole utterance): a chunk mask on the ENCODER's self-attention, WeNet's U2 recipe for a
 * first pass that does not depend on audio behind a bounded look-ahead (YAML asr_model.chunk).  Under a chunk of c >= 1 encoder frames
 * (an encoder frame is 4 input frames) query i sees key j iff
 *   j < klen_b (the key-padding mask, as without a chunk)  and  j < (i / c + 1) * c  and  (left < 0 or j >= (i / c - left) * c)
 * (integer division): its own chunk whole, `left` chunks before it (-1: all of them), nothing behind it.  c = 1, left = -1 is the causal mask;
 * c >= the encoder length with left = -1 masks nothing.  A query row without a visible key -- only with left >= 0, and only a padding row whose window
 * starts at or behind klen_b -- gives an attention output of exactly 0 and passes exactly 0 to every gradient (WeNet zeroes such rows behind its
 * softmax).  The decoder's self-attention stays causal and its cross-attention stays full: the attention decoder is the second pass.
 *   size     >= 0: the chunk in encoder frames; 0 = full context
 *   left     >= -1: earlier chunks a query may see; -1 = all
 *   dynamic  0 / 1: 1 = every TRAINING step draws its chunk (`size` then only serves the passes that do not train; `left` is not drawn)
 * Which chunk is in force: masr_run_batch(MASR_EVAL) and every masr_recog* (greedy, the beams, the CTC beams, rescoring, ctc_align: each runs one encoder
 * forward) always use `size`.  masr_run_batch(MASR_TRAIN) uses `size`, or with dynamic = 1 the draw of its step -- all integers, from the step's 32-bit
 * seed as masr_specaug forms it (step_seed, the dropout key and hash word, uni(w, r) = (uint64(w) * r) >> 32), with Tp = the batch's encoder frames:
 *   w = the dropout hash word of (the dropout key of (step_seed, site 0x43484E4B), 0);  r = 1 + uni(w, Tp - 1);
 *   Tp < 2 or r > Tp / 2 (integer division): full context (chunk 0);  otherwise c = r % 25 + 1, in [1, 25].
 * so about half of the steps train with full context and the others with a chunk of at most a second of audio (WeNet's rule), and a resumed run
 * draws what the uninterrupted one would have (masr_dropout_state).  The step's chunk travels in the per-step upload beside the seed, so a captured
 * step graph replays with the current one.  A model without a policy runs the kernels it ran before, bit for bit. */
typedef struct masr_chunk_policy {
    int32_t size, left, dynamic;
} masr_chunk_policy;
/* the model's policy (null or all-zero: off, the default).  Changing it drops captured step graphs; size < 0, left < -1 or dynamic outside {0, 1}
 * returns -1 with a message and leaves the old policy in place. */
int masr_set_chunk(masr_model* m, const masr_chunk_policy* p);
/* the stateless draw above on the host, at the (seed, step) masr_dropout_state reports before the step: 0 (full context) or the chunk in [1, 25] */
int masr_chunk_draw(uint64_t seed, uint64_t step, int Tp);
/* *size = the chunk the last masr_run_batch or masr_recog* ran its encoder with (0 = full context).  -1 before the first one. */
int masr_chunk_last(masr_model* m, int* size);

/* nn.utils.clip_grad_norm_(parameters, max_norm) (fo_meta_interface.py:148-149,242-243): norm only */
int masr_grad_norm(masr_model* m, void* stream);
/* ... followed by `if not isnan(norm): SGD(lr, momentum, nesterov).step()` (fo_meta_interface.py:228-248).
   first_step: bit 0 = the optimiser's first step (torch creates the momentum buffer as a copy of the gradient: the buffer is not
   read); bit 1 = its last step (run_task drops its SGD after k steps, :228-250: the buffer is not written).  With both bits set
   (meta_k = 1) momentum_buf is not touched and may be null. */
int masr_clip_sgd_step(masr_model* m, float* momentum_buf, float max_norm, float lr, float momentum, int nesterov,
                       int first_step, void* stream);
/* clip in place (multi_interface.py:108-109, mono fine-tune) */
int masr_clip_grads(masr_model* m, float max_norm, void* stream);
/* _partial_meta_update after the val-batch clip (fo_meta_interface.py:148-154,180-198): updates += clip(grads) */
int masr_clip_accumulate(masr_model* m, float* updates, float max_norm, void* stream);
/* Quirk Q5 of the reference (fo_meta_interface.py:151-154): a val-batch gradient whose norm is NaN is only warned about and still accumulated, so
   one bad batch turns the meta weights into NaNs.  Default (off) reproduces that.  On (pretrain.py --fix_nan_meta_grad): masr_clip_grads zeroes
   such a gradient and masr_clip_accumulate leaves `updates` alone -- decided on the device from the norm both already form, no host sync; the
   norm reported by masr_read_stats stays NaN, so the warning is still logged. */
void masr_set_drop_nan_grads(masr_model* m, int on);
/* buf[0..n) *= min(1, max_norm / (*norm + 1e-6)) with the norm read from device memory (what masr_allreduce applies chunk by chunk, as one
   pass: for transports that cannot pipeline it) */
int masr_clip_scale_flat(float* buf, int64_t n, const float* norm, float max_norm, void* stream);

/* flat helpers on arbitrary device buffers */
int masr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, int step, void* stream);
/* torch.optim.AdamW (decoupled != 0: p *= 1 - lr*weight_decay, then the Adam update) or torch.optim.Adam with its L2
 * weight_decay (decoupled == 0: g += weight_decay*p) -- config/transformer/adapt/hkust-adamw.yaml through
 * getattr(torch.optim, cls) (src/transformer_torch_trainer.py:44-46) */
/* Adam / AdamW step guarded ON THE DEVICE by the gradient norm of the model's stats block (masr_clip_grads leaves it there): a NaN
   norm skips the step, as `if math.isnan(grad_norm): warn else: step()` does (mono_interface.py:141-148, multi_interface.py:108-114),
   without the host having to read the norm first.  The host may be ONE step ahead: (lr_a, t_a) are learning rate and Adam step
   count if the previous guarded step was applied, (lr_b, t_b) if it was skipped -- the previous launch recorded which; pass the same
   pair twice when the previous outcome is known.  `slot` alternates 0 / 1 from step to step. */
int masr_adam_step_guarded(masr_model* m, float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr_a, int t_a,
                           float lr_b, int t_b, float b1, float b2, float eps, float weight_decay, int decoupled, int slot, void* stream);
/* the meta update of one meta-step in ONE pass: Adam on g = (((g_0 + g_1) + ...) + g_{n-1}) * gscale, the per-task gradients read
   straight from n <= 8 device buffers (`grads` is a HOST array of device pointers).  Replaces the accumulator of
   fo_meta_interface.py:180-202 (zero + n axpy passes + scale pass + Adam pass) with the same additions in the same order. */
int masr_adam_sum_step(float* p, const float* const* grads, int n_grads, float gscale, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float b1, float b2, float eps, int step, void* stream);
/* out = (((g_0 + g_1) + ...) + g_{n-1}) * scale over n <= 8 device buffers (`grads` is a HOST array of device pointers): the
   rank-local sum of the task gradients of one wave of concurrent tasks = the payload of that wave's ONE RCCL all-reduce
   (the `_updates[n] += p.grad` of fo_meta_interface.py:190-196 for the tasks this rank ran) */
int masr_sum_n(float* out, const float* const* grads, int n_grads, float scale, int64_t n, void* stream);
int masr_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int decoupled, int step, void* stream);
/* optimizer_cls 'RAdam' of set_model (src/transformer_torch_trainer.py:36-41).  The reference takes it from `torch_optimizer`, an
 * un-vendored third-party package absent from its tree.  variant 1 = that package's conventions (its authors' published
 * implementation: rectification once N_sma >= 5, denom = sqrt(v) + eps with sqrt(1 - b2^t) folded into the step size, weight decay
 * applied to the weight: p -= lr * wd * p) -- what FlatRAdam uses; pinned against a restatement of that algorithm in the oracle,
 * "parity unpinned" against the package itself.  variant 0 = torch.optim.RAdam's (rho_t > 5, bias-corrected denominator, L2 decay),
 * pinned against torch.optim.RAdam on the CPU (tests/test_hip_misc.py). */
int masr_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float b1, float b2,
                    float eps, float weight_decay, int step, int variant, void* stream);
/* torch.optim.SGD(momentum, nesterov) on arbitrary flat buffers */
int masr_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum,
                  int nesterov, int first_step, void* stream);
int masr_scale(float* x, int64_t n, float a, void* stream);                           /* _updates /= counter (:201-202) */
int masr_axpy(float* y, const float* x, int64_t n, float a, void* stream);
int masr_copy(float* dst, const float* src, int64_t n, void* stream);                 /* load_state_dict(_original) (:226) */

/* ---------------------------------------------------------------------------------------------------------------------
 * The exchange step of sharded meta-training: all-reduce(sum) of the flat meta-gradient over the ranks' GPUs with
 * RCCL over xGMI.  The reference is one process: its `_updates[n] += p.grad` over the tasks of a meta-step and `_updates[n] /=
 * counter` (src/fo_meta_interface.py:190-196,200-202) become, with the tasks sharded one per GPU, local gradient -> all-reduce(sum)
 * -> the same division and the same (replicated) Noam-Adam step on every rank.  librccl is bound with dlopen at init: libmasr has
 * no link-time dependency on it and single-GPU runs never load it.
 *   masr_allreduce_unique_id : rank 0 draws the communicator id (MASR_UNIQUE_ID_BYTES bytes); the caller ships it to the other
 *                              ranks over any side channel (torch.distributed's store, a file, MPI ...).
 *   masr_allreduce_init      : ncclCommInitRank on the CURRENT HIP device (one process per GPU); the communicator owns a
 *                              non-blocking side stream.  NULL + masr_last_error() on failure.
 *   masr_allreduce           : buf[0..n) (device fp32) is summed over all ranks IN PLACE, on the communicator's side stream,
 *                              ordered behind everything queued so far on `producer_stream` -- the caller goes on queueing the
 *                              next task's inner forward on `producer_stream` meanwhile and must not touch buf before
 *                              masr_allreduce_wait.  norm != NULL: buf is first scaled by clip_grad_norm_'s coefficient
 *                              min(1, max_norm / (*norm + 1e-6)) (`norm` = device float, e.g. masr_stats_device(m) + 3 after
 *                              masr_grad_norm; the reference clips every task's gradient before accumulating it, :148-149).  The
 *                              coefficient exists only once the whole backward is done, so the scale pass cannot be bucketed into
 *                              the backward: it is PIPELINED with the collective instead, chunk by chunk (chunk k+1 is scaled on
 *                              the producer stream while chunk k is on the wire).  nchunks (1..16): a few LARGE chunks -- xGMI is
 *                              point-to-point, a ring is bound by one ~153 GB/s link, small buckets only add launch latency.
 *   masr_allreduce_wait      : `stream` waits (on the device, no host sync) for every exchange issued so far.
 * Not thread-safe per communicator; calls on one communicator must come in the same order on every rank (RCCL's rule). */
#define MASR_UNIQUE_ID_BYTES 128
typedef struct masr_comm masr_comm;
int masr_allreduce_unique_id(char* id);
masr_comm* masr_allreduce_init(int rank, int world, const char* id);
void masr_allreduce_destroy(masr_comm* c);
int masr_allreduce(masr_comm* c, float* buf, int64_t n, const float* norm, float max_norm, int nchunks, void* producer_stream);
int masr_allreduce_wait(masr_comm* c, void* stream);
/* host-side health check of the exchange: 0 = the last exchange completed (or none is pending), 1 = still running (timeout_ms == 0: one
 * poll), -1 = RCCL reports an asynchronous error, or timeout_ms ran out -- the communicator is then aborted and the job must end. */
int masr_allreduce_check(masr_comm* c, int timeout_ms);
/* device view of the model's stats block: [0] loss, [1] n_correct, [2] n_total, [3] gradient norm (after masr_grad_norm / masr_clip_*) */
const float* masr_stats_device(masr_model* m);

/* MyTransformer.recog (mono_transformer_torch.py:143-176): greedy decode, out int32 [Ldec][B] (device),
 * Ldec = max(floor(ilens/4)).  Needs workspace for L = Ldec.
 * masr_recog      : KV-cached incremental decode (one new position per step, the step replayed as a hipGraph);
 * masr_recog_full : the reference's literal schedule (the whole prefix is decoded again at every step).
 * Both emit the same token sequences (the target mask is causal). */
int masr_recog(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int32_t* out, void* stream);
int masr_recog_full(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int32_t* out, void* stream);

/* Beam search over the KV-cached decoder step (no LM -- see masr_recog_beam_lm --, no CTC -- see masr_recog_beam_ctc: the scores are sums of fp32
 * log_softmax of the decoder's logits).
 * Per utterance b: enc_len = floor(ilens[b] / 4); maxlen = enc_len if max_step_ratio <= 0, else max(1, floor(max_step_ratio * enc_len)),
 * capped at the 3000 rows of pe; minlen = floor(min_step_ratio * enc_len); Lmax = max over b of maxlen.  1 <= K <= 64.
 * At every step the K best extensions (score descending, parent rank ascending, token ascending) of the live hypotheses are kept;
 * those that end in <eos> (excluded while a hypothesis has fewer than minlen tokens) are set aside as ended; an utterance stops when
 * nothing runs any more or its best ended score is >= its best running one; after maxlen steps the running ones end as they are.
 * Result (device): tokens int32 [B][Lmax] (the best ended hypothesis without sos / eos, -1 behind it), lens int32 [B], scores fp32 [B].
 * K = 1 is the greedy decode of masr_recog trimmed at its first <eos>.  Needs a workspace of masr_beam_workspace_bytes(B, T, K, Lmax)
 * bound with masr_bind; the decode step is captured as its own hipGraph (the cache of masr_recog is not touched). */
int64_t masr_beam_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax);
int masr_recog_beam(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio, float max_step_ratio,
                    int32_t* tokens, int32_t* lens, float* scores, void* stream);

/* Joint CTC/attention beam search (hybrid models of masr_create_ctc; ESPnet's ctc_weight decoding, Watanabe et al. 2017).  The search of
 * masr_recog_beam with the CTC head's one-pass prefix score psi over the encoder memory (log_softmax of the head, blank 0, T_b = enc_len frames):
 * each live hypothesis keeps its P = min(floor(3K/2), eligible) best tokens by attention logit (blank never, eos from minlen tokens on), and a
 * candidate scores s(h+c) = s(h) + att_w * lp_att(c | h) + ctc_w * (psi(h+c) - psi(h)) in fp32; psi(h+eos) is the full CTC log-probability
 * of h.  The K best candidates (joint score descending, parent rank ascending, logit descending, token ascending) are kept; a candidate
 * scoring -inf is never kept nor ended.  Stop rule, minlen / maxlen and the result layout as masr_recog_beam; scores are joint scores, and an
 * utterance where nothing ended gets the empty hypothesis with score -inf.  Needs ctc_w > 0 and att_w >= 0 (both finite), a CTC head, the
 * bounds of masr_recog_beam and a workspace of masr_beam_ctc_workspace_bytes(B, T, K, Lmax) (it holds [2][B*K][T/4][P] CTC states of
 * 8 bytes).  The step is captured as its own hipGraph. */
int64_t masr_beam_ctc_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax);
int masr_recog_beam_ctc(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio, float max_step_ratio,
                        float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, void* stream);

/* Shallow fusion of a backoff n-gram language model into the attention beam.
 * The LM: order N in [1, 4] over the model's C <= 65535 output units with the model's ids (<s> = sos = 0, </s> = eos = C - 1, units 1 .. C - 2).
 * An n-gram of order n has ids (w_1 .. w_n), a natural-log probability logp and a natural-log backoff weight bo (0 for the highest order), both
 * finite fp32 and <= 0: every LM term is <= 0 and the beam's stop rule stays exact.  Order 1 is dense (every class 0 .. C - 1 has a unigram).
 * masr_lm_create: per order n, grams[n - 1] is int32 [counts[n - 1]][n], logp[n - 1] / backoff[n - 1] fp32 [counts[n - 1]] (host arrays;
 * backoff[order - 1] may be null).  Builds the device tables (dense unigrams; per order >= 2 one open-addressing table of 16-byte slots, capacity a
 * power of two >= 2 x the count, n-grams inserted in input order) on the current device and returns the handle; NULL + masr_last_error() for
 * a duplicate n-gram, an id outside [0, C - 1], </s> anywhere but last or <s> anywhere but first in an n-gram, a non-finite or positive value
 * or a missing unigram -- all found on the host, before anything touches the device.  masr_lm_bytes: device bytes held.
 * lm(c | h), the LM score of class c after hypothesis h: ctx = the last min(N - 1, |h| + 1) tokens of [sos] + h; acc = 0.f; for k = |ctx| down to 0,
 * with g = the last k tokens of ctx: if (g, c) is an n-gram of order k + 1, lm = fl(acc + logp(g, c)) and stop; else if k >= 1 and g is an n-gram
 * of order k, acc = fl(acc + bo(g)).  k = 0 always hits.  fp32 additions in this order.
 * masr_recog_beam_lm: the search of masr_recog_beam (attention decoder alone, also on a hybrid model) with the per-step increment
 *   f(c) = fl(lp(c) + fl(lm_w * lm(c | h))), lp(c) = (z_c - mx) - log_s as masr_recog_beam composes it (no fused multiply-add),
 * over all C classes (no pre-beam).  A hypothesis's list is its K best classes by (f descending, class ascending), eos excluded below minlen;
 * a candidate scores fl(s(h) + f(c)); candidates are kept by score descending, parent rank ascending, f descending, class ascending.  Selection,
 * ended / running bookkeeping, the stop rule, minlen / maxlen and the result layout are masr_recog_beam's; K = 1 is greedy on the fused score;
 * lm_w = 0 gives masr_recog_beam's scores bit for bit.  Same bounds and messages as masr_recog_beam; lm_w finite and >= 0; the LM's C must equal
 * the model's odim.  Needs a workspace of masr_beam_lm_workspace_bytes(B, T, K, Lmax) = the beam's plus the fp32 fused rows [B*K][odim padded
 * to 128].  The step is captured as its own hipGraph, keyed on the LM and lm_w as well: a call with another LM or weight captures anew. */
typedef struct masr_lm masr_lm;
masr_lm* masr_lm_create(int order, int C, const int64_t* counts, const int32_t* const* grams, const float* const* logp, const float* const* backoff);
void masr_lm_destroy(masr_lm* lm);
int64_t masr_lm_bytes(const masr_lm* lm);
int64_t masr_beam_lm_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax);
int masr_recog_beam_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio,
                       float max_step_ratio, float lm_w, int32_t* tokens, int32_t* lens, float* scores, void* stream);

/* Shallow fusion of an LSTM language model into the attention beam.
 * The LM is torch.nn.Embedding(C, E) -> torch.nn.LSTM(E, H, L) -> torch.nn.Linear(H, C) over the model's C output units with the model's ids;
 * gate order i, f, g, o; no dropout.  1 <= E, H <= 2048, L in [1, 4], C in [2, 65535].  The start token is start_id in [0, C): 0 is this model's
 * sos, C - 1 serves LMs trained with sos = eos.
 * masr_nlm_create takes host arrays: embed fp32 [C][E]; per layer l, w_ih[l] [4H][in_l] (in_0 = E, else H), w_hh[l] [4H][H], b_ih[l] and b_hh[l]
 * [4H]; lo_w [C][H], lo_b [C].  It builds the device weights on the current device and returns the handle; NULL + the masr_last_error text for a
 * null array, a non-finite weight, a size out of range or start_id outside [0, C) -- all found on the host, before anything touches the device.
 * Device layout and precision: bf16 operands (embedding rows, h, every weight matrix; per layer one matrix [4 Hp][INp + Hp] = W_ih | W_hh, with
 * E and H padded up to multiples of 32 by zeros) with fp32 accumulation; fp32 gates, cell state c, bias fl(b_ih + b_hh), output bias and LM
 * logits.  h is stored as bf16, the only form any consumer reads.  A padded unit's pre-activations are exactly 0, so its c and h stay exactly 0.
 * masr_nlm_bytes: device bytes held.
 * lm(c | h), the LM score of class c after hypothesis h: feed [start] + h from the zero state; y = the fp32 output row behind the last token;
 * lm = (y_c - mx) - log_s with mx = max y and log_s = log sum exp(y - mx), composed as masr_recog_beam composes lp.  Every LM term is <= 0 and
 * the beam's stop rule stays exact.
 * masr_recog_beam_nlm: the search of masr_recog_beam (attention decoder alone, also on a hybrid model) with the per-step increment
 *   f(c) = fl(lp(c) + fl(lm_w * lm(c | h))), no fused multiply-add,
 * and everything else as masr_recog_beam_lm states it: the row lists by (f descending, class ascending), the selection, the stop rule, minlen /
 * maxlen, the result layout, the bounds and messages; lm_w finite and >= 0; the LM's C must equal the model's odim; lm_w = 0 gives
 * masr_recog_beam's scores bit for bit.  Every hypothesis row carries the LM's state (h, c) per layer, double-buffered by step parity: a row
 * reads its parent's state of the step before and writes its own, so the state follows the beam's re-parenting without a copy.
 * Needs a workspace of masr_beam_nlm_workspace_bytes(m, nlm, B, T, K, Lmax) = the beam's plus, with R = B * K, Cp = odim padded to 128, Hp = H
 * padded to 32 and each entry rounded up to 256 bytes:
 *   R * Cp * 4  (the fused rows)  +  R * Cp * 4  (the LM logits)  +  2 * L * R * Hp * 2  (h)  +  2 * L * R * Hp * 4  (c)
 *   +  R * Hp * 2  (the top layer's new h once more, the output projection's operand at an address that does not depend on the step).
 * The step is captured as its own hipGraph, keyed on the LM and lm_w as well: a call with another LM or weight captures anew.
 * masr_nlm_score, model-free: the teacher-forced log-probability of R token sequences, tokens int32 [R][ld] and lens int32 [R] (device; every
 * length in [0, ld], every token in [0, C - 1], vetted on the host after one synchronisation): logp_out[r] = the sum over i = 0 .. lens[r], in
 * that order in fp32, of lm(target_i | tokens[r][0 .. i)), target_i = tokens[r][i] and, behind the last token, eos = C - 1.  It runs the beam's
 * step kernels position by position with every row its own parent.  work: 256-byte aligned device memory of at least
 * masr_nlm_score_work_bytes(nlm, R, ld) bytes (1 <= R <= 2^20, 0 <= ld <= 4096). */
typedef struct masr_nlm masr_nlm;
masr_nlm* masr_nlm_create(int C, int E, int H, int L, int start_id, const float* embed, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, const float* lo_w, const float* lo_b);
void masr_nlm_destroy(masr_nlm* nlm);
int64_t masr_nlm_bytes(const masr_nlm* nlm);
int64_t masr_beam_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int Lmax);
int masr_recog_beam_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio,
                        float max_step_ratio, float lm_w, int32_t* tokens, int32_t* lens, float* scores, void* stream);
int64_t masr_nlm_score_work_bytes(const masr_nlm* nlm, int R, int ld);
int masr_nlm_score(const masr_nlm* nlm, const int32_t* tokens, const int32_t* lens, int R, int ld, float* logp_out, void* work, int64_t work_bytes,
                   void* stream);

/* One-pass joint CTC/attention beam search with the n-gram LM, a length bonus and an N-best list (what ESPnet-style recipes decode
 * with).  It is masr_recog_beam_ctc with these differences; everything else (P = floor(3K/2), blank never, eos from minlen tokens on, -inf never
 * kept nor ended, minlen / maxlen, dead rows) is that search's:
 *   pre-beam   a hypothesis's P candidates are its best classes by g(c) = fl(lp(c) + fl(lm_w * lm(c | h))), masr_recog_beam_lm's fused increment
 *              composed the same way, in the order (g descending, class ascending): the LM takes part in the pre-beam
 *   score      s(h+c) = fl(fl(fl(fl(s(h) + fl(att_w * lp(c))) + fl(ctc_w * fl(psi(h+c) - psi(h)))) + fl(lm_w * lm(c | h))) + b), b = len_bonus
 *              for a token and 0 for eos (the bonus counts emitted tokens); every product and sum is rounded on its own
 *   N-best     an utterance keeps its N best ended hypotheses, 1 <= N <= K, ordered by score descending and, on equal scores, the one that ended
 *              first (the earlier step, then the lower rank); at st >= maxlen the running hypotheses end as they are and compete too.  The
 *              entries are distinct token sequences
 *   stop rule  an utterance is finished when nothing runs, st >= maxlen, or the list is full and its N-th score is
 *              >= fl(run_best + fl((maxlen - st) * max(len_bonus, 0))): every other increment is <= 0 (up to the few-ulp caveat on psi of
 *              DESIGN 5.2) and a running hypothesis of st tokens collects at most maxlen - st more bonuses, so the result is what the same
 *              beam gives when it runs to maxlen with no stop rule.  At len_bonus <= 0 and N = 1 it is masr_recog_beam's rule
 * Result (device): tokens int32 [B][N][Lmax] (-1 behind each hypothesis), lens int32 [B][N], scores fp32 [B][N]; a slot without a hypothesis
 * holds lens -1, scores -inf, tokens -1.  lm_w = 0, len_bonus = 0, N = 1 gives masr_recog_beam_ctc's scores (its pre-beam orders by logit, this
 * one by lp: the two differ only where rounding ties two logits' lp).
 * -1 with a message, before any launch: masr_recog_beam_ctc's refusals (a CTC head, ctc_w finite and > 0, att_w finite and >= 0, its bounds), a
 * null LM, an LM whose C is not the model's odim, lm_w negative or not finite, len_bonus not finite, N outside [1, K]; -2: a workspace below
 * masr_beam_ctc_lm_workspace_bytes(B, T, K, N, Lmax) = the joint beam's plus the fused rows [B*K][odim padded to 128], the LM terms [B*K][P] and the
 * list.  The step is captured as its own hipGraph, keyed on the LM and N; the four weights are device values written before the replays, so a call
 * with other weights replays the same graph and never an old value. */
int64_t masr_beam_ctc_lm_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax);
int masr_recog_beam_ctc_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float min_step_ratio,
                           float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, int32_t* tokens, int32_t* lens, float* scores,
                           void* stream);

/* The same one-pass joint CTC/attention beam with the LSTM LM in place of the n-gram.  It is masr_recog_beam_ctc_lm word for word
 * with one substitution: lm(c | h) is the LSTM LM's, as masr_recog_beam_nlm defines it (feed [start] + h from the zero state; lm = (y_c - mx) -
 * log_s over the fp32 LM logits; every hypothesis row carries (h, c) per layer, double-buffered by step parity; a row reads its parent's state of
 * the step before).  The pre-beam by g(c) = fl(lp(c) + fl(lm_w * lm(c | h))), P = floor(3K/2), blank never, eos from minlen tokens on, the
 * five-rounding score, the N-best list, the bound stop rule and the result layout [B][N][Lmax] / [B][N] / [B][N] are that entry's.  Every LM term
 * is <= 0, so the stop-rule argument of DESIGN 5.7 carries over.  lm_w = 0 gives masr_recog_beam_ctc_lm's result at lm_w = 0 bit for bit.
 * -1 with a message, before any launch: everything masr_recog_beam_ctc_lm refuses, a null LSTM LM, an LM whose C is not the model's odim, lm_w
 * negative or not finite, len_bonus not finite, N outside [1, K]; -2: a workspace below
 * masr_beam_ctc_nlm_workspace_bytes(m, nlm, B, T, K, N, Lmax) = masr_beam_ctc_lm_workspace_bytes(B, T, K, N, Lmax) (its fused rows are shared)
 * plus, with R = B * K, Cp = odim padded to 128, Hp = H padded to 32 and each entry rounded up to 256 bytes:
 *   R * Cp * 4  (the LM logits)  +  2 * L * R * Hp * 2  (h)  +  2 * L * R * Hp * 4  (c)  +  R * Hp * 2  (the top layer's new h).
 * The step is captured as its own hipGraph, keyed on (B, T, K, Lmax, N, the LM); the four weights are device values written before the replays,
 * so a call with other weights replays the same graph and never an old value. */
int64_t masr_beam_ctc_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int N, int Lmax);
int masr_recog_beam_ctc_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int N,
                            float min_step_ratio, float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, int32_t* tokens,
                            int32_t* lens, float* scores, void* stream);

/* CTC prefix beam search on the CTC head alone (hybrid models of masr_create_ctc): the encoder and the head GEMM of
 * masr_recog_beam_ctc, then masr_ctc_beam_search (below) on the head's fp32 logits with blank 0, eos = odim - 1, Tp = T / 4 and
 * enc_len = floor(ilens[b] / 4).  Result (device): tokens int32 [B][nbest][T/4], lens int32 [B][nbest], scores fp32 [B][nbest].  A model
 * without a CTC head returns -1.  Needs a workspace of masr_ctc_beam_workspace_bytes(B, T, K) bound with masr_bind. */
int64_t masr_ctc_beam_workspace_bytes(const masr_model* m, int B, int T, int K);
int masr_recog_ctc_beam(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, int32_t* tokens, int32_t* lens,
                        float* scores, void* stream);
/* Streaming first pass on the CTC head (hybrid models under a chunk policy with size c > 0).  The batch's audio arrives in pieces;
 * the encoder runs incrementally -- the front-end on input windows, every layer on a chunk's rows against a per-layer K|V cache -- and produces,
 * chunk by chunk, the head logits that one chunk-masked full pass (masr_recog_ctc_beam's encoder and head GEMM) produces on the zero-padded
 * batch, for every frame t < ilens[b] / 4 (equal in exact arithmetic; the summation order differs).  A greedy (best-path) CTC decode follows
 * the chunks; after the last piece the full-utterance prefix beam runs on the accumulated logits.  Chunk n = encoder frames [n c, (n + 1) c)
 * runs once the input frames up to 4 (n + 1) c + 8 are buffered, so what is emitted does not depend on how the audio was cut into pieces.
 *   masr_stream_workspace_bytes  the workspace an open stream of B utterances of at most max_frames input frames needs under the model's
 *                  current chunk size (bind one at least that large); -1: no CTC head, no chunk size, B < 1, max_frames outside [4, 12000].
 *   masr_stream_begin   opens a stream (an open one is dropped).  -1 for the same reasons or an unbound model, -2 for a workspace that is too
 *                  small.  The policy's `dynamic` is ignored; `size` and `left` are those of the moment of the call.
 *   masr_stream_feed    the next n input frames of every utterance, xs device fp32 [B][n][idim].  valid (host int32 [B], null = all n):
 *                  valid[b] < n ends utterance b behind its first valid[b] frames, and every later piece must give it 0 (otherwise -1); the
 *                  engine zero-fills behind an utterance's end itself.  Runs every chunk whose window is complete; with last != 0 all that
 *                  remain (a final partial chunk; the trailing T % 4 input frames make no encoder frame, as in the full pass).  *frames_out
 *                  (may be null) = the encoder frames emitted so far.  -1: no open stream, a piece after the last, more than max_frames.
 *   masr_stream_partial device views of the greedy result so far: tokens / frames int32 [B][*ld] (a token and the encoder frame that emitted
 *                  it; -1 behind the list), lens int32 [B].
 *   masr_stream_logits  the accumulated head logits in the layout masr_ctc_beam_search reads (row of utterance b, frame t at logits +
 *                  (b * (max_frames / 4) + t) * *ld), enc_lens int32 [B] = (frames of b received) / 4, *frames = frames emitted so far.
 *   masr_stream_ctc_beam  after the last piece: masr_ctc_beam_search on those logits and lengths with blank 0, eos = odim - 1; tokens int32
 *                  [B][nbest][max_frames / 4], lens int32 [B][nbest], scores fp32 [B][nbest] (device).  Refuses what masr_recog_ctc_beam does.
 * Any other call that plans the workspace (masr_run_batch, masr_recog*, masr_bind, masr_set_chunk) ends an open stream: the next feed returns
 * -1 with "no open stream".  Every refusal sets masr_last_error and launches nothing. */
int64_t masr_stream_workspace_bytes(const masr_model* m, int B, int max_frames);
int masr_stream_begin(masr_model* m, int B, int max_frames, void* stream);
int masr_stream_feed(masr_model* m, const float* xs, int n, const int32_t* valid, int last, int* frames_out, void* stream);
int masr_stream_partial(masr_model* m, const int32_t** tokens, const int32_t** frames, const int32_t** lens, int* ld);
int masr_stream_logits(masr_model* m, const float** logits, int64_t* ld, const int32_t** enc_lens, int* frames);
int masr_stream_ctc_beam(masr_model* m, int K, int nbest, int32_t* tokens, int32_t* lens, float* scores, void* stream);

/* masr_recog_ctc_beam with the n-gram LM fused into the search: the same encoder pass, head GEMM and workspace, then
 * masr_ctc_beam_search_lm (below) with blank 0 and eos = odim - 1.  scores fp32 [B][nbest] are the fused finals, am fp32 [B][nbest] the acoustic
 * totals.  -1 besides masr_recog_ctc_beam's refusals: a null LM, an LM whose C is not the model's odim, lm_w negative or not finite, len_bonus
 * not finite. */
int masr_recog_ctc_beam_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, float lm_w,
                           float len_bonus, int32_t* tokens, int32_t* lens, float* scores, float* am, void* stream);

/* masr_recog_ctc_beam with the LSTM LM fused into the search: the same encoder pass and head GEMM, then masr_ctc_beam_search_nlm
 * (below) with blank 0 and eos = odim - 1; scores and am as masr_recog_ctc_beam_lm gives them.  One frame of the search is captured as a
 * hipGraph of its own, keyed on (B, T, K, the LM) and replayed T / 4 times; lm_w and len_bonus are device values written before the replays,
 * so a call with other weights replays the same graph and never an old value.  -1 with a message, before any launch: everything
 * masr_recog_ctc_beam_lm refuses, a null LSTM LM, an LM whose C is not the model's odim; -2: a workspace below
 * masr_ctc_beam_nlm_workspace_bytes(m, nlm, B, T, K) = masr_ctc_beam_workspace_bytes(B, T, K) with masr_ctc_beam_nlm_work_bytes(nlm, B, T / 4,
 * odim, K) in the place of the plain search's work buffer. */
int64_t masr_ctc_beam_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K);
int masr_recog_ctc_beam_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, float lm_w,
                            float len_bonus, int32_t* tokens, int32_t* lens, float* scores, float* am, void* stream);

/* CTC forced alignment of each utterance's transcript on the CTC head (hybrid models of masr_create_ctc): the encoder and the head
 * GEMM of masr_recog_ctc_beam, then masr_ctc_align (below) on the head's fp32 logits with blank 0, Tp = T / 4 and enc_len = floor(ilens[b] / 4)
 * -- frames, start and end count ENCODER frames, one per 4 input frames.  ys_flat / olens are host int64 as masr_run_batch takes them: the
 * tokens of all utterances one after the other, without sos / eos, olens[b] of them for utterance b.  A length or token the operator refuses
 * on the device (below) is passed on and refused there: that utterance's score is NaN.  Result (device): frames int32 [B][T/4], start / end int32
 * [B][maxL], score fp32 [B].  -1 with a message, before any launch: a null model or pointer, a model without a CTC head, B < 1, T < 4,
 * maxL < 0 or 2 * maxL + 1 > 2048, ilens outside [4, T], B * (maxL + 2) above the model's staging buffer (65536 ints, more once a training batch has grown it); -2: a workspace below masr_ctc_align_workspace_bytes(B, T, maxL). */
int64_t masr_ctc_align_workspace_bytes(const masr_model* m, int B, int T, int maxL);
int masr_recog_ctc_align(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, const int64_t* ys_flat, const int64_t* olens, int maxL,
                         int32_t* frames, int32_t* start, int32_t* end, float* score, void* stream);

/* Attention rescoring of an N-best list (hybrid models of masr_create_ctc; the two-pass decode WeNet calls "attention
 * rescoring").  For utterance b and list entry n with tokens h (length l >= 0, no sos / eos) and first-pass score c(b, n):
 *   decoder input  [sos, h_0 .. h_{l-1}] padded with eos, targets [h_0 .. h_{l-1}, eos] padded with -1; L = 1 + the longest live l of the
 *                  call.  The decoder runs ONCE, teacher-forced, over all B * N entries (the pass of masr_run_batch(MASR_EVAL): bf16-operand
 *                  logits GEMM, fp32 logits);
 *   att(b, n)      = sum_{i = 0 .. l} log_softmax(z_i)[target_i], l + 1 terms; the log-softmax in fp32 over the odim classes, the sum in
 *                  fp32, position ascending, by one thread: a result does not depend on the launch geometry;
 *   score          = att_w * att + ctc_w * c in fp32 (two rounded products, one rounded sum; the ctc term is left out when ctc_w == 0);
 *   output order   score descending, then first-pass rank ascending.  Entries without a list (lens -1) stay last, in their first-pass
 *                  order, with lens -1 and score = att = -inf.
 * Results (device): tokens int32 [B][N][ld] (rows copied from the first pass), lens int32 [B][N], scores / att / ctc fp32 [B][N] (ctc:
 * the first-pass scores, copied bit for bit), order int32 [B][N] = the first-pass rank of output entry j.  Needs a CTC head, att_w > 0,
 * ctc_w >= 0 (both finite) and 1 <= N <= K <= 64; otherwise -1.
 *   masr_recog_rescore  the first pass is the CTC prefix beam of masr_recog_ctc_beam(K, nbest = N) on the same encoder pass; ld = T / 4.
 *   masr_rescore_nbest  the first pass is the caller's: tokens_in int32 [B][N][ld_tok], lens_in int32 [B][N] (-1 = no entry, else in
 *                       [0, ld_tok]), ctc_in fp32 [B][N], device arrays that the outputs may not overlap; ld = ld_tok < 3000.  Every token
 *                       of a live list must lie in [1, odim - 2]; a list with another token is refused with -1.  Runs the encoder and the
 *                       second pass.
 * Both copy the list lengths (masr_rescore_nbest: the lists) to the host between the passes and wait for the stream there -- the ONE
 * host synchronisation of the call: the decoder pass is launched for L positions, not for the Lmax planned.
 * Workspace: masr_rescore_workspace_bytes(B, T, K, N, Lmax) bound with masr_bind, Lmax = the longest hypothesis planned for (the decoder is
 * planned for N * (Lmax + 1) positions per utterance).  masr_recog_rescore needs Lmax >= max(floor(ilens / 4)) (T / 4 always suffices: a
 * CTC hypothesis is no longer than its frames); masr_rescore_nbest (pass K = N) needs Lmax >= its longest live list.  A call whose plan
 * does not fit the bound workspace returns -2, as the other decoders do. */
int64_t masr_rescore_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax);
int masr_recog_rescore(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float att_w, float ctc_w, int32_t* tokens,
                       int32_t* lens, float* scores, float* att, float* ctc, int32_t* order, void* stream);
/* masr_recog_rescore whose first pass is the LM-fused search of masr_recog_ctc_beam_lm(K, nbest = N, lm_w, len_bonus): c(b, n) is that pass's
 * fused score, copied bit for bit into `ctc`; everything else, the single host synchronisation and the workspace included, is
 * masr_recog_rescore's.  The full two-pass pipeline: LM-fused CTC first pass, attention rescoring. */
int masr_recog_rescore_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float lm_w,
                          float len_bonus, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc,
                          int32_t* order, void* stream);
/* masr_recog_rescore_lm with the LSTM LM search of masr_recog_ctc_beam_nlm(K, nbest = N, lm_w, len_bonus) as its first pass: c(b, n)
 * is that pass's fused score, copied bit for bit into `ctc`; the second pass and the single host synchronisation are masr_recog_rescore's.
 * -1 with a message, before any launch: everything masr_recog_rescore_lm refuses, a null LSTM LM, an LM whose C is not the model's odim;
 * -2: a workspace below masr_rescore_nlm_workspace_bytes(m, nlm, B, T, K, N, Lmax) = masr_rescore_workspace_bytes(B, T, K, N, Lmax) with
 * masr_ctc_beam_nlm_work_bytes(nlm, B, T / 4, odim, K) in the place of the first pass's work buffer. */
int64_t masr_rescore_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int N, int Lmax);
int masr_recog_rescore_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float lm_w,
                           float len_bonus, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc,
                           int32_t* order, void* stream);
int masr_rescore_nbest(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int N, const int32_t* tokens_in, int64_t ld_tok,
                       const int32_t* lens_in, const float* ctc_in, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att,
                       float* ctc, int32_t* order, void* stream);

/* Levenshtein distance of two id sequences (host-side; replaces the `editdistance` extension the reference's metric
 * imports, src/monitor/metric.py:4,66,87).  Returns the distance, < 0 on bad arguments. */
int64_t masr_edit_distance(const int32_t* a, int na, const int32_t* b, int nb);

/* ---------------------------------------------------------------------------------------------------------------------
 * BLSTM-CTC model of config/blstm: MonoBLSTM.forward (src/model/blstm/mono_blstm.py:77-92) =
 * BlstmEncoder (src/modules/encoder.py:215-298: VGG 1->128->128 pool(ceil) ->256->256 pool(ceil), RNNP = nlayers x
 * {packed bidirectional LSTM(enc_dim), Linear(2 enc_dim -> proj_dim | enc_odim), tanh}, pad frames zeroed) + Linear head,
 * with BLSTMTrainer.run_batch's loss (src/blstm_trainer.py:55-85): targets [sos] + y + [eos] (sos = eos = odim - 1),
 * log_softmax + CTCLoss(blank 0, mean, zero_infinity).  sample_rate 1 / dropout 0 per layer (the shipped settings).
 * Same conventions as the masr_* calls above: flat fp32 params / grads in the reference's state_dict order (each tensor
 * starts on a 4-float boundary), caller-owned workspace, stream-ordered, int return codes. */
typedef struct masr_blstm masr_blstm;
typedef struct masr_blstm_config {
    int32_t idim, odim;          /* feature width (83), vocabulary incl. <blank> and <eos> (367) */
    int32_t enc_dim, proj_dim;   /* LSTM hidden size per direction, projection width between layers */
    int32_t enc_odim;            /* projection width of the last layer (encoder.odim) */
    int32_t nlayers;             /* <= 8 */
    int32_t sample_rate[8];      /* time sub-sampling behind BLSTM layer i (encoder.sample_rate, e.g. 1_2_2): the layer's output keeps every
                                  * sample_rate[i]-th frame, enc_lens -> (enc_lens + 1) / sample_rate[i] (src/modules/encoder.py:118-121); 0 = 1 */
} masr_blstm_config;
masr_blstm* masr_blstm_create(const masr_blstm_config* cfg);
void masr_blstm_destroy(masr_blstm* m);
int64_t masr_blstm_param_numel(const masr_blstm* m);
int masr_blstm_param_count(const masr_blstm* m);
int masr_blstm_param_info(const masr_blstm* m, int idx, char* name, int name_cap, int64_t shape[4], int* ndim, int64_t* offset);
int64_t masr_blstm_workspace_bytes(const masr_blstm* m, int B, int T, int max_target_len);
int masr_blstm_bind(masr_blstm* m, float* params, float* grads, void* workspace, int64_t ws_bytes);
int masr_blstm_refresh(masr_blstm* m, void* stream);
/* xs: device fp32 [B][T][idim]; ilens / olens: host int64 [B]; ys_flat: host int64 (labels without sos/eos, concatenated).
 * MASR_TRAIN leaves d loss / d params in the bound gradient buffer. */
int masr_blstm_run_batch(masr_blstm* m, const float* xs, const int64_t* ilens, const int64_t* ys_flat, const int64_t* olens,
                         int B, int T, int flags, void* stream);
/* forward only (MonoBLSTM.forward / greedy_decode, mono_blstm.py:63-92): head output readable through masr_blstm_last_logits */
int masr_blstm_forward(masr_blstm* m, const float* xs, const int64_t* ilens, int B, int T, void* stream);
int masr_blstm_read_stats(masr_blstm* m, float out[4], void* stream);            /* out[0] = CTC loss, out[3] = grad norm */
/* The LSTM recurrence of a layer as ONE launch per pass (workgroups resident for the whole sequence, W_hh slices in registers, h_t / dz_t
 * exchanged as self-flagging granules: csrc/lstm_rec.hip) instead of one launch per timestep.  Default ON for the shapes it covers (B <= 32,
 * enc_dim <= 384); off = per-timestep launches (A/B + test; same results to fp32 rounding).  A timed-out exchange is reported by
 * masr_blstm_read_stats. */
void masr_blstm_set_resident_recurrence(masr_blstm* m, int on);
/* forward-only callers (masr_blstm_forward + masr_blstm_last_logits, i.e. the Tester's greedy CTC decode) never read the stats block:
 * this is their check.  Synchronises the stream; -1 (text in masr_last_error(), mark cleared) when the resident recurrence of a launch
 * since the last check timed out -- the logits are then invalid.  After a time-out the remaining resident launches of the step return
 * at once (one bounded wait per step, not one per layer and pass). */
int masr_blstm_check(masr_blstm* m, void* stream);
/* head output (pre-softmax) [B][Tp][odim] fp32 and enc_lens int32 [B] on the device, Tp = ceil(ceil(T/2)/2) */
int masr_blstm_last_logits(masr_blstm* m, float** logits, int32_t** enc_lens, int* B, int* Tp, int* C);
/* nn.utils.clip_grad_norm_(parameters, max_norm) on the flat gradient; the norm is read with masr_blstm_read_stats */
int masr_blstm_clip_grads(masr_blstm* m, float max_norm, void* stream);
/* clip_grad_norm_(max_norm) + SGD(momentum, nesterov) step + shadow refresh (mono_interface.py:141-148) */
int masr_blstm_clip_sgd_step(masr_blstm* m, float* momentum_buf, float max_norm, float lr, float momentum, int nesterov,
                             int first_step, void* stream);

/* Log-mel filterbank features on the GPU, written in the layout of the reference's feat.dat shards
 * (src/io/dataset.py:123-139: one [sum T_b][idim] float matrix per split).  The reference has no extraction code; the
 * algorithm is Kaldi's compute-fbank-feats with the recipe's options (16 kHz, 25 ms / 10 ms, povey window, 512-point FFT,
 * mel bins over 20 Hz - 8 kHz, log) -- oracle/fbank_np.py.  wav: device fp32 on the 16-bit PCM scale, utterances
 * concatenated; wav_off: device int64 [B+1]; row_off: device int64 [B] first output row of each utterance;
 * frames of utterance b: T_b = 1 + (n_b - 400) / 160 (0 if n_b < 400); max_frames >= max T_b; feat: device [sum T_b][n_mel]. */
int masr_fbank(const float* wav, const int64_t* wav_off, const int64_t* row_off, int B, int max_frames, int n_mel,
               float* feat, void* stream);

/* The shipped 83-dim rows: n_mel log-mel bins | 3 Kaldi pitch dims (config/transformer/pretrain/fometa-hkust.yaml:13 `idim: 83`,
 * README.md:24).  The pitch dims follow ESPnet's make_fbank_pitch.sh = compute-kaldi-pitch-feats | process-kaldi-pitch-feats
 * with Kaldi's default options (4 kHz resampling, NCCF at 417 log-spaced lags between 1/400 s and 1/50 s, Viterbi, then
 * [2 * pov feature, 2 * POV-normalised log pitch, 10 * delta log pitch]; oracle/pitch_np.py; the dithering noise Kaldi adds to the
 * delta is omitted).  feat: device [sum T_b][n_mel + 3] with T_b = min(fbank frames, pitch frames of utterance b) -- the pitch
 * tracker needs (ceil(n_b / 4) - 182) / 40 + 1 frames' worth of samples -- as `paste-feats --length-tolerance=2` truncates them;
 * row_off from those T_b; max_frames >= max T_b; total_samples = wav_off[B], max_samples = max n_b (host values);
 * work: masr_fbank_pitch_work_bytes(total_samples, B, max_frames) bytes of device memory. */
int64_t masr_fbank_pitch_work_bytes(int64_t total_samples, int B, int max_frames);
int masr_fbank_pitch(const float* wav, const int64_t* wav_off, const int64_t* row_off, int64_t total_samples, int64_t max_samples, int B, int max_frames,
                     int n_mel, float* feat, void* work, int64_t work_bytes, void* stream);

/* collate_fn zero-padding of CommonVoiceDataset rows (src/io/dataset.py:21-33,147-153) done on the GPU:
 * feat fp32 [sum T_i][D] resident in HBM, row_start int64 [B] (device), lens int32 [B] (device). */
int masr_gather_pad(const float* feat, const int64_t* row_start, const int32_t* lens, float* xs, int B, int Tmax, int D, void* stream);

/* nn.CTCLoss(blank, reduction='mean', zero_infinity=True) on log_softmax(logits) with its gradient wrt the
 * logits (src/blstm_trainer.py:22,62-70).  logits fp32 [T][B][C] device; targets/tgt_off/in_len/tgt_len int32 device.
 * nll [B], loss [1], grad [T][B][C] device outputs; work: masr_ctc_work_floats(T,B,maxS) floats. */
int64_t masr_ctc_work_floats(int T, int B, int maxS);
/* The lengths are DEVICE arrays, so they are vetted by the kernel: an utterance with in_len < 0 or > T, tgt_len < 0 or
 * 2 tgt_len + 1 > maxS is not run -- its nll (hence the mean loss) is NaN, its gradient rows are zero.  in_len == 0 is torch's
 * "no path" case: nll 0, zero gradient (zero_infinity).  masr_ctc_status synchronises and returns 0, or (index + 1) of the last
 * utterance the most recent masr_ctc_loss call ON THIS work buffer (same T, B, maxS) refused, with the text in masr_last_error().  The mark
 * lives in the call's own work buffer (re-armed by every masr_ctc_loss on it): calls on different buffers / streams do not mix. */
int masr_ctc_status(const float* work, int T, int B, int maxS, void* stream);
int masr_ctc_loss(const float* logits, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len,
                  const int32_t* tgt_len, int T, int B, int C, int blank, float* nll, float* loss, float* grad,
                  float* work, int maxS, void* stream);

/* CTC prefix beam search with merging (Hannun et al. 2014) over a CTC output layer, model-free like masr_ctc_loss.
 * logits: device fp32, the row of utterance b, frame t at logits + (b * Tp + t) * ld (ld >= C); enc_lens: device int32 [B], each clamped to
 * [0, Tp] by the kernels; frames past it are never read.  x_t = fp32 log_softmax of the row.  Classes `blank` and `eos` (-1 = none) are
 * never emitted.  The beam holds at most K distinct prefixes with (p_b, p_nb) in log space, from the empty prefix (0, -inf).  Per frame, with
 * S_t the P = min(K, emittable classes) best emittable classes by (x_t descending, class ascending), every entry h in rank order gives
 *   stay:      p_b' = logaddexp(p_b, p_nb) + x_t(blank),  p_nb' = p_nb + x_t(last(h))  (-inf for the empty prefix)
 *   h + c:     p_b' = -inf,  p_nb' = (c == last(h) ? p_b : logaddexp(p_b, p_nb)) + x_t(c)        for c in S_t
 * and an extension h + c that is itself an entry h' of the beam is no candidate: its p_nb' is log-added to p_nb' of stay(h').  A candidate
 * scores logaddexp(p_b', p_nb'); the K best by (score descending, parent rank ascending, stay before extensions, position in S_t
 * ascending) are kept, -inf candidates never.  All of it fp32 in this order.  Prefix identity is (length, 64-bit hash), see DESIGN 5.3.
 * Result (device): the final beam in rank order, tokens int32 [B][nbest][Tp] (-1 behind each list), lens int32 [B][nbest], scores fp32
 * [B][nbest]; slots beyond the live entries have lens -1 and score -inf; enc_len 0 gives the empty prefix with score 0.
 * -1 (text in masr_last_error()) unless 1 <= K <= 64, 1 <= nbest <= K, 2 <= C <= 4096, 0 <= blank < C, eos in {-1} or [0, C) and != blank,
 * B >= 1, Tp >= 1, work_bytes >= masr_ctc_beam_work_bytes(B, Tp, C, K), and no pointer is null. */
int64_t masr_ctc_beam_work_bytes(int B, int Tp, int C, int K);
int masr_ctc_beam_search(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                         void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens, float* scores, void* stream);

/* masr_ctc_beam_search with a backoff n-gram LM (masr_lm_create) and a per-token bonus fused into the ranking (Hannun et al. 2014).
 * Model-free.  Everything is the search above unless stated.  Needs blank == 0, eos == C - 1 and lm->C == C <= 4096: the LM's ids are <s> = 0 --
 * the blank's slot, which is never emitted -- and </s> = C - 1.  lm_w finite and >= 0; len_bonus finite, of any sign (no stop rule depends on it).
 *   LM state   each entry keeps, besides the purely acoustic (p_b, p_nb), an fp32 lmacc(h): lmacc(()) = 0.f,
 *              lmacc(h + c) = fl(lmacc(h) + fl(fl(lm_w * lm(c | h)) + len_bonus)), lm(c | h) the rule of masr_recog_beam_lm; every product
 *              and sum rounded on its own (no fused multiply-add).  lmacc is a function of the token sequence alone: a prefix that is
 *              merged into, or leaves the beam and is created again, has the same bits whichever parent produced it.
 *   acoustics  the stay / extension recursion, S_t (by acoustic logit: no LM in the pre-beam), the merge test and the prefix identity are
 *              unchanged; p_b and p_nb never contain an LM term.
 *   ranking    a candidate scores fl(logaddexp(p_b', p_nb') + lmacc(prefix)): a stay uses lmacc(h), an extension lmacc(h + c).  Selection
 *              order as above (score descending, parent rank ascending, stay first, position in S_t ascending); -inf is never kept.
 *   the end    final(h) = fl(fl(am(h) + lmacc(h)) + fl(lm_w * lm(eos | h))), am = logaddexp(p_b, p_nb); the whole final beam is re-ranked by
 *              (final descending, beam rank ascending) and its first nbest entries are returned.
 * Result (device): tokens / lens as above, scores fp32 [B][nbest] = final, am fp32 [B][nbest] = the acoustic total; slots that are not live
 * hold lens -1 and scores = am = -inf; enc_len 0 gives the empty prefix with am 0 and score fl(lm_w * lm(eos | ())).
 * With lm_w == 0 and len_bonus == 0, tokens, lens and scores equal masr_ctc_beam_search's bit for bit and am == scores (DESIGN 5.6 has the
 * argument).  Every refusal returns -1 with its text in masr_last_error() before anything is launched.  The work buffer is
 * masr_ctc_beam_lm_work_bytes(B, Tp, C, K) bytes (today the plain search's size: the LM state lives on chip). */
int64_t masr_ctc_beam_lm_work_bytes(int B, int Tp, int C, int K);
int masr_ctc_beam_search_lm(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                            const masr_lm* lm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens,
                            float* scores, float* am, void* stream);

/* masr_ctc_beam_search_lm with the LSTM LM (masr_nlm_create) in the n-gram's place.  Model-free.  It is that search word for word
 * with one substitution: lm(c | h) is the LSTM LM's, as masr_recog_beam_nlm defines it -- feed [start] + h from the zero state; lm = (y_c - mx) -
 * log_s over the fp32 LM logits.  lmacc, the purely acoustic p_b / p_nb, S_t by acoustic logit alone, the merge test and the prefix hash, the
 * ranking, the selection order, the end-of-utterance term, the final re-rank and the result layout (am included; enc_len 0: the empty prefix
 * with am 0 and score fl(lm_w * lm(eos | ()))) are masr_ctc_beam_search_lm's.  Needs blank == 0, eos == C - 1, nlm->C == C <= 4096, lm_w finite
 * and >= 0, len_bonus finite.
 *   LM state   lmacc AND the LM's recurrent state of a prefix are functions of its token sequence alone: a prefix that is merged into keeps its
 *              state and takes no LM step; one that leaves the beam and is created again gets the same bits from whichever parent produced
 *              it (an LM step's result for a row depends neither on the row's index nor on the rows around it).
 *   the search is frame-synchronous across launches: per frame one kernel runs every utterance's frame (the beam lives in the work buffer, by
 *              parity), then the LM advances on the B * K rows -- a row that took a token steps from its parent's state, a row that stayed
 *              copies its parent's state and log-softmax row.  All Tp frames are launched; an utterance past its enc_len idles.
 * With lm_w == 0, tokens, lens, scores and am equal masr_ctc_beam_search_lm's at lm_w == 0 and the same len_bonus bit for bit (every LSTM lm is
 * finite and <= 0, so DESIGN 5.6's signed-zero argument carries over); with len_bonus == 0 as well, masr_ctc_beam_search's.
 * Every refusal returns -1 with its text in masr_last_error() before anything is launched: what masr_ctc_beam_search_lm refuses, a null LSTM LM,
 * a work buffer that is not 256-byte aligned or below masr_ctc_beam_nlm_work_bytes(nlm, B, Tp, C, K) = masr_ctc_beam_work_bytes(B, Tp, C, K)
 * plus, with R = B * K, Cp = C padded to 128, Hp = H padded to 32 and each entry rounded up to 256 bytes:
 *   8 + 8  (the step word, the two weights)  +  5 * (2 * R * 4) + 2 * (2 * R * 8)  (the beam by parity: p_b, p_nb, lmacc, last, len; hash, parent
 *   hash)  +  2 * B * 4  (live counts)  +  2 * (R * 4)  (the frame's token and parent row)  +  2 * L * R * Hp * 2  (h)  +  2 * L * R * Hp * 4  (c)
 *   +  R * Hp * 2  (the top layer's new h)  +  R * Cp * 4  (the LM logits)  +  2 * R * Cp * 4  (the log-softmax rows by parity). */
int64_t masr_ctc_beam_nlm_work_bytes(const masr_nlm* nlm, int B, int Tp, int C, int K);
int masr_ctc_beam_search_nlm(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                             const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens,
                             float* scores, float* am, void* stream);

/* Contextual phrase biasing of the CTC prefix beam (the context graph of WeNet's CTC prefix beam search).
 * The phrase list: P in [1, 65536] phrases of 1 .. 64 tokens each over the model's C in [3, 65535] classes, tokens in [1, C - 2] (no blank / sos, no
 * eos).  masr_bias_create takes host arrays, phrase i = tokens[off[i] .. off[i + 1]); it builds a trie whose nodes are the distinct prefixes of
 * the phrases (root = node 0, at most 2^20 nodes), as one open-addressing table of 16-byte slots (node, token) -> child with the n-gram tables'
 * capacity, hash and probing, plus one byte revoke(u) per node, on the current device.  NULL + masr_last_error() for a null array, C or P out of
 * range, a phrase of length 0 or above 64, a token outside [1, C - 2], a duplicate phrase or more than 2^20 nodes -- all found on the host, before
 * anything touches the device.  masr_bias_bytes: device bytes held; masr_bias_nodes: the trie's nodes, the root included.
 *   d(u) the depth of node u, e(u) the length of the longest phrase that is a prefix of, or equal to, u's string (0: none), revoke(u) = d(u) - e(u).
 *   The state of a hypothesis is (u, n), n the credited tokens; () has (root, 0), and token c advances it:
 *     v = child(u, c);  if v exists: (v, n + 1)
 *     n = n - revoke(u);  v = child(root, c);  if v exists: (v, n + 1);  else (root, n)
 *   and n_final(h) = n - revoke(u) at the end of the utterance.  n >= 0 always.  A phrase that is a proper prefix of a longer one keeps its tokens
 *   when the longer match breaks.  There are no failure links: a broken match restarts at the root with the current token, so an overlapping
 *   restart is missed on purpose (the phrase `a a b` is not found in `a a a b`).
 * masr_ctc_beam_search_bias is masr_ctc_beam_search_lm word for word when lm is given and masr_ctc_beam_search when lm is null (lm_w and len_bonus
 * are then ignored and no lmacc exists), except:
 *   state      each entry also carries (u, n) of its prefix: an extension that is a candidate gets step(parent's state, c), a stay keeps its own,
 *              a merged extension needs none.  The state is a function of the token sequence alone, so a prefix that is merged into, or leaves
 *              the beam and is created again, has the same state whichever parent produced it.  p_b, p_nb, lmacc, S_t (by acoustic logit alone),
 *              the merge test and the prefix hash are untouched.
 *   ranking    a candidate scores fl(x + fl(bias_w * (float)n(prefix))), x = fl(acoustic + lmacc(prefix)) with the LM, the acoustic score without.
 *              The count is provisional: a half-matched phrase is already boosted.  Every product and sum rounded on its own; selection order
 *              unchanged.
 *   the end    final(h) = fl(y + fl(bias_w * (float)n_final(h))), y = fl(fl(am + lmacc) + fl(lm_w * lm(eos | h))) with the LM, y = am without;
 *              the final beam is re-ranked by (final descending, beam rank ascending) in both cases.
 * Result (device): tokens, lens, scores (= final) and am as masr_ctc_beam_search_lm gives them (am also without an LM); nbias int32 [B][nbest] =
 * n_final, -1 in slots that are not live; enc_len 0 gives the empty prefix with am 0 and nbias 0.
 * Needs blank == 0 and eos == C - 1 with or without an LM, bias->C == C <= 4096, bias_w finite and >= 0.  -1 with a message before any launch:
 * a null phrase list and everything the underlying search refuses.  The work buffer is masr_ctc_beam_bias_work_bytes(B, Tp, C, K) bytes (the
 * plain search's size: the state lives on chip).  The LSTM LM search has no biasing. */
typedef struct masr_bias masr_bias;
masr_bias* masr_bias_create(int C, int P, const int32_t* tokens, const int64_t* off);
void masr_bias_destroy(masr_bias* bias);
int64_t masr_bias_bytes(const masr_bias* bias);
int masr_bias_nodes(const masr_bias* bias);
int64_t masr_ctc_beam_bias_work_bytes(int B, int Tp, int C, int K);
int masr_ctc_beam_search_bias(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                              const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work, int64_t work_bytes,
                              int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias, void* stream);
/* Through the transformer (hybrid models): masr_recog_ctc_beam_bias runs the encoder pass and head GEMM of masr_recog_ctc_beam, then
 * masr_ctc_beam_search_bias with blank 0 and eos = odim - 1 (lm may be null) in the workspace of masr_ctc_beam_workspace_bytes(B, T, K).
 * masr_recog_rescore_bias is masr_recog_rescore_lm with that search as its first pass: c(b, n) is its final score, copied bit for bit into
 * `ctc`; the second pass (not biased), the single host synchronisation and the workspace are masr_recog_rescore's.  -1 besides what
 * masr_recog_ctc_beam / masr_recog_rescore refuse: a null phrase list, one whose C is not the model's odim, bias_w negative or not finite and,
 * with an LM, what masr_recog_ctc_beam_lm refuses. */
int masr_recog_ctc_beam_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K,
                             int nbest, float lm_w, float len_bonus, float bias_w, int32_t* tokens, int32_t* lens, float* scores, float* am,
                             int32_t* nbias, void* stream);
int masr_recog_rescore_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K, int N,
                            float lm_w, float len_bonus, float bias_w, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores,
                            float* att, float* ctc, int32_t* order, void* stream);

/* The resumable CTC prefix beam.  Model-free.  masr_ctc_beam_search (lm and bias null), masr_ctc_beam_search_lm (lm given) or
 * masr_ctc_beam_search_bias (bias given, lm or not) run over frame ranges: the beam is kept in a state block of the work buffer between calls,
 * so the search can follow logits that arrive piece by piece, and a result can be read at any point.  The run object is host memory only; it
 * owns no GPU memory and holds the pointers it was opened with (logits, enc_lens, the LM's and the phrase list's tables, the work buffer),
 * which must stay valid until masr_ctc_beam_run_close.  The LSTM LM search has no resumable form.
 *   masr_ctc_beam_run_work_bytes  masr_ctc_beam_work_bytes(B, Tp, C, K) + the state block (per entry p_b, p_nb, last, len, hash, parent hash,
 *                  lmacc, the packed LM context, the automaton's node and credit; per utterance the live count and the frame cursor).
 *   masr_ctc_beam_run_open     checks the arguments, launches the initial state (the empty prefix, cursor 0).  NULL on a refusal.
 *   masr_ctc_beam_run_advance  runs the frames [t_done, t_end) of every utterance, t_done the largest t_end so far (0 after open): the frame
 *                  statistics of those rows, then for utterance b the frames [cursor_b, min(t_end, clamp(enc_lens[b]))).  Two launches; none
 *                  when t_end == t_done.
 *   masr_ctc_beam_run_result   the tail on the beam as it stands: outputs as the matching one-shot search writes them (am may be null without
 *                  an LM and a phrase list, nbias without a phrase list).  Stores nothing into the state: the search continues afterwards.
 *   masr_ctc_beam_run_close    frees the run object (null is allowed).
 * Final result: after advance(Tp) the result equals the matching one-shot search on the same arguments bit for bit, however [0, Tp) was cut
 * into calls.  Partial result: after advance(t) the result equals what the matching one-shot search returns with enc_lens[b] replaced by
 * min(enc_lens[b], t), bit for bit -- the search is causal, so this is the definition of a partial result.  Causality: advance(t_end) reads no
 * logits row at t >= t_end.  enc_lens is read on the device at every call; the caller may change enc_lens[b] between calls only among values
 * >= the largest t_end passed so far (a stream's lengths: frames received / 4 until the utterance ends).  Otherwise results are unspecified,
 * but every access stays inside the planned buffers: an utterance that stopped in front of a call's t_end, because its length said so then,
 * stays stopped there whatever its length says later (a call runs an utterance only from the frame where the call's own rows begin), and
 * one whose length fell below its cursor runs nothing.
 * Refusals return -1 (open: NULL) with their text in masr_last_error() before any launch and leave the state unwritten: what the matching
 * one-shot search refuses of these arguments, a work buffer below masr_ctc_beam_run_work_bytes or not 8-byte aligned, t_end < t_done or
 * t_end > Tp, nbest outside [1, K], a null output that the search writes, a null run. */
typedef struct masr_ctc_beam_run masr_ctc_beam_run;
int64_t masr_ctc_beam_run_work_bytes(int B, int Tp, int C, int K);
masr_ctc_beam_run* masr_ctc_beam_run_open(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int blank, int eos,
                                          const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work,
                                          int64_t work_bytes, void* stream);
int masr_ctc_beam_run_advance(masr_ctc_beam_run* run, int t_end, void* stream);
int masr_ctc_beam_run_result(const masr_ctc_beam_run* run, int nbest, int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias,
                             void* stream);
void masr_ctc_beam_run_close(masr_ctc_beam_run* run);
/* The resumable beam inside a stream: the prefix beam follows the chunks, with the n-gram LM and the phrase list if given.
 *   masr_stream_beam_open    on an open stream at any time (an open beam is replaced): a masr_ctc_beam_run on the stream's logits and
 *                  lengths with blank 0, eos = odim - 1, in a work buffer and state block of its own behind the stream's other buffers
 *                  (masr_stream_workspace_bytes includes them: masr_ctc_beam_run_work_bytes(B, max_frames / 4, odim, 64) more than before).
 *                  Opened after some chunks have run, it runs the frames emitted so far at once (also after the last piece, when its result
 *                  is then the final one).  Refuses what masr_recog_ctc_beam, _lm and _bias do.
 *   masr_stream_feed         with a beam open, advances it once to the frames emitted, after the feed's chunk steps: two launches per feed.
 *   masr_stream_beam_result  at any time: the partial result as defined above (before the first chunk: the empty prefix); after the last
 *                  piece the final one, which without an LM and a phrase list equals masr_stream_ctc_beam(K, nbest) bit for bit.
 *                  tokens int32 [B][nbest][max_frames / 4], lens, scores, am, nbias [B][nbest] (device).
 * Whatever ends the stream ends its beam.  A stream without an open beam runs exactly the launches it ran before; masr_stream_ctc_beam is
 * unchanged and may be called beside an open beam. */
int masr_stream_beam_open(masr_model* m, int K, const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* stream);
int masr_stream_beam_result(masr_model* m, int nbest, int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias, void* stream);

/* Contextual phrase biasing of the attention beam and the joint beam.  A hypothesis of these searches is one token sequence on one
 * path (prefixes are never merged), so each live row carries the state (u, n) of its hypothesis, starting at (root, 0).  For a hypothesis h of
 * st - 1 tokens in state (u, n) and a class c at step st:
 *     (u', n') = the state behind token c (above; classes 0 and eos have no child, so they yield (root, n - revoke(u)))
 *     dn(h, c) = n' - n, an integer in [-63, 1];  if c != eos and st >= maxlen: dn -= revoke(u')   (the hypothesis ends as it is at this step)
 *     b(h, c)  = fl(bias_w * (float)dn(h, c))                                                       (one rounding)
 * The credit is provisional: a half-matched phrase is already boosted, a broken match gives its unearned tokens back, and so does the end of the
 * hypothesis (eos or maxlen).  lm may be NULL in both entries (lm_w is then ignored).
 * masr_recog_beam_bias is masr_recog_beam_lm with the row increment g(c) = fl(f(c) + b(h, c)); f is that entry's fused increment, or lp(c)
 * without an LM.  A row's list is its K best by (g descending, class ascending), eos skipped below minlen; a candidate scores fl(s(h) + g(c)); the
 * merge, the ended / running bookkeeping and the result layout are masr_recog_beam's.  Stop: nothing runs, st >= maxlen, or best_ended >=
 * fl(run_best + fl((float)(maxlen - st) * bias_w)) -- a running hypothesis gains at most bias_w per further token and every other term is <= 0.
 * nbias int32 [B] (device) = n_final of the returned hypothesis.  At bias_w = 0 with an LM tokens and scores equal masr_recog_beam_lm's at the
 * same lm_w bit for bit; with lm NULL they equal masr_recog_beam's except where rounding ties the lp of two different logits of one row: the
 * plain beam ranks a row by the logit, this one by lp (class ascending among equal lp), as masr_recog_beam_lm does at lm_w = 0.  The step graph
 * is keyed on the LM, lm_w, the list and bias_w.
 * masr_recog_beam_ctc_bias is masr_recog_beam_ctc_lm with these differences: the pre-beam ranks the P candidates by g(c) as above (so a phrase
 * token is rescued into the pre-beam); the score is that entry's five-rounding sum followed by + b(h, c) as a sixth rounding (with lm NULL the LM
 * term is the constant +0.f, added in the same place); the stop bound is fl(run_best + fl((float)(maxlen - st) * fl(max(len_bonus, 0) + bias_w))).
 * nbias int32 [B][N], -1 in an empty slot.  bias_w is a device value next to the four weights: the graph is keyed on the LM, N and the list, and
 * a call with another bias_w replays it and never an old value.  At bias_w = 0 with an LM the result equals masr_recog_beam_ctc_lm's bit for bit.
 * -1 with a message, before any launch, outputs unwritten: everything masr_recog_beam_lm / masr_recog_beam_ctc_lm refuse except a null LM, a null
 * list, a list whose C is not the model's odim, bias_w negative or not finite, a null nbias; -2: a workspace below
 * masr_beam_bias_workspace_bytes(B, T, K, Lmax) = masr_beam_lm_workspace_bytes plus the states [2][B*K] (8 bytes each), or below
 * masr_beam_ctc_bias_workspace_bytes(B, T, K, N, Lmax) = masr_beam_ctc_lm_workspace_bytes plus the states and the bias terms [B*K][P] (each
 * entry rounded up to 256 bytes).  The LSTM-LM beams (masr_recog_beam_nlm, masr_recog_beam_ctc_nlm, masr_recog_ctc_beam_nlm) have no biasing. */
int64_t masr_beam_bias_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax);
int masr_recog_beam_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K,
                         float min_step_ratio, float max_step_ratio, float lm_w, float bias_w, int32_t* tokens, int32_t* lens, float* scores,
                         int32_t* nbias, void* stream);
int64_t masr_beam_ctc_bias_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax);
int masr_recog_beam_ctc_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K, int N,
                             float min_step_ratio, float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, float bias_w,
                             int32_t* tokens, int32_t* lens, float* scores, int32_t* nbias, void* stream);

/* CTC forced alignment: the single best alignment (Viterbi path) of a known transcript to the frames of a CTC output layer, model-free like
 * masr_ctc_loss and masr_ctc_beam_search.  logits and enc_lens as for masr_ctc_beam_search (row of utterance b, frame t at
 * logits + (b * Tp + t) * ld, ld >= C; enc_lens device int32 [B], each clamped to [0, Tp]; frames past it and columns >= C are never read);
 * targets as for masr_ctc_loss (device int32: utterance b's tokens are targets[tgt_off[b] .. + tgt_len[b])).  With n = enc_len, L = tgt_len,
 * S = 2L + 1 and label(s) = blank for even s, y[(s - 1) / 2] for odd s:
 *   emissions  u_t(c) = fl(z_t(c) - max_t), max_t the maximum of the row's C classes (exact, whatever the order): one fp32 subtraction.  The path
 *              is decided on these raw, max-shifted logits, not on log_softmax: the normaliser is the same for every state of a frame and
 *              cannot change an arg-max, and without it the path is a function of fp32 additions and comparisons only -- no exp / log.
 *   start      v_0(0) = u_0(blank), v_0(1) = u_0(y[0]) if L > 0, every other state -inf.
 *   recursion  v_t(s) = fl(m + u_t(label(s))), m the largest of v_{t-1}(s) (back-pointer 0), v_{t-1}(s - 1) (1; s >= 1) and v_{t-1}(s - 2)
 *              (2; s odd, s >= 3, label(s) != label(s - 2)).  A tie goes to the smaller back-pointer.  m = -inf: the state is -inf, back-pointer 0.
 *   end        the final state is S - 1, or S - 2 if L > 0 and v_{n-1}(S - 2) > v_{n-1}(S - 1) (a tie: S - 1); the back-pointers are walked from it.
 *   score      the path's log-probability under the frame-wise softmax: acc = 0.f; for t = 0 .. n - 1 in this order acc = fl(acc + lsum_t), with
 *              lsum_t = log(sum_c exp(u_t(c))) in fp32 (strided sum of __expf over the lanes of one wave, wave sum, __logf); then
 *              score = fl(v_{n-1}(final) - acc).
 * Result (device): frames int32 [B][Tp] -- at t < n the target index i in [0, L) while the path is in state 2i + 1, -1 in a blank state, and -2 at
 * t >= n; start / end int32 [B][maxL] -- the first frame of token i and one past its last, -1 for i >= L (every token of a feasible alignment
 * has end > start); score fp32 [B].  L = 0 gives the all-blank path, n = 0 with L = 0 score 0.  Infeasible (both final states -inf: n below L
 * plus the number of adjacent equal tokens, or n = 0 with L > 0): score -inf, frames -2 throughout, start / end -1.  Refused on the device, the
 * targets being device arrays (tgt_len < 0 or > maxL, a token outside [0, C) or equal to blank): score NaN, the rest as for infeasible; no
 * status word, no synchronisation.  Non-finite logits give an unspecified path, but no access outside the arrays.
 * -1 (text in masr_last_error()), before any launch, unless B >= 1, Tp >= 1, 2 <= C <= 4096, ld >= C, 0 <= blank < C, maxL >= 0,
 * 2 * maxL + 1 <= 2048 (the lattice width of masr_ctc_loss), work_bytes >= masr_ctc_align_work_bytes(B, Tp, maxL), and no pointer is null. */
int64_t masr_ctc_align_work_bytes(int B, int Tp, int maxL);
int masr_ctc_align(const float* logits, int64_t ld, const int32_t* enc_lens, const int32_t* targets, const int32_t* tgt_off, const int32_t* tgt_len,
                   int B, int Tp, int C, int blank, int maxL, void* work, int64_t work_bytes, int32_t* frames, int32_t* start, int32_t* end,
                   float* score, void* stream);

/* device timing (HIP events on the launch stream) for bench.py's roofline block: one slot per conv launch of the VGG
 * front-end (each is ONE launch per step, so slot time / launches = that kernel's average duration) and one per kernel
 * class for the rest.  bench.py::PROF_NAMES mirrors this list. */
#define MASR_PROF_CONV1_FWD 0     /* 1 -> 64, direct fp32 (HBM-bound) */
#define MASR_PROF_CONV2_FWD 1     /* 64 -> 64 on the full-resolution map + fused 2x2 max-pool */
#define MASR_PROF_CONV3_FWD 2     /* 64 -> 128 */
#define MASR_PROF_CONV4_FWD 3     /* 128 -> 128 + fused 2x2 max-pool */
#define MASR_PROF_CONV2_DGRAD 4   /* 64 <- 64 with conv1's weight gradient fused into the epilogue */
#define MASR_PROF_CONV3_DGRAD 5
#define MASR_PROF_CONV4_DGRAD 6
#define MASR_PROF_CONV2_WGRAD 7
#define MASR_PROF_CONV3_WGRAD 8
#define MASR_PROF_CONV4_WGRAD 9
#define MASR_PROF_CONV1_WGRAD 10  /* folds of the per-workgroup weight-gradient partials: conv1's fused sums and the slab reduces of conv2..4 */
#define MASR_PROF_GEMM_ENC 11     /* Linear forward / dgrad over the B*T' encoder rows (incl. vgg2enc, grouped cross-attention K/V) */
#define MASR_PROF_GEMM_DEC 12     /* ... over the B*L decoder rows */
#define MASR_PROF_WGRAD_ENC 13    /* Linear weight gradients reducing over encoder rows (split-K) */
#define MASR_PROF_WGRAD_DEC 14    /* grouped launch of the decoder-row weight gradients */
#define MASR_PROF_ATTN_ENC 15
#define MASR_PROF_ATTN_DEC 16
#define MASR_PROF_LAYERNORM 17
#define MASR_PROF_POOL 18         /* max-pool/ReLU backward */
#define MASR_PROF_OPTIM 19        /* grad norm, clip + SGD */
#define MASR_PROF_SHADOWS 20      /* bf16 operand shadows after a parameter update */
#define MASR_PROF_MISC 21         /* loss, embedding, casts, split-K combine */
#define MASR_PROF_N 22
int masr_profile_enable(masr_model* m, int on);
/* sums since the last call: ms[MASR_PROF_N], launches[MASR_PROF_N]; synchronises */
int masr_profile_read(masr_model* m, float* ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif
