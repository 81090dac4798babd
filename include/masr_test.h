/* libmasr -- test-only entry points (exported by libmasr.so, NOT part of the operator API of include/masr.h).
 *
 * Standalone launches of single kernels for the parity tests (tests/test_hip_kernels.py, tools/), bf16 passed as uint16_t bit patterns,
 * and one fault-injection hook.  Same conventions as masr.h: plain pointers and sizes, device memory owned by the caller, stream-ordered,
 * 0 on success / < 0 on error (text: the masr_last_error function of masr.h).
 */
#ifndef MASR_TEST_H
#define MASR_TEST_H
#include "masr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fault injection for the time-out test of the resident LSTM recurrence: while on, the resident forward launches of THIS handle lose one
 * workgroup at start, so that its peers run into the bound of their wait and the step is reported as failed by masr_blstm_read_stats /
 * masr_blstm_check instead of hanging (tests/test_hip_blstm.py) */
void masr_test_blstm_stall(masr_blstm* m, int on);

/* standalone kernel entry points used by the parity tests (bf16 passed as uint16_t bit patterns) */
int masr_test_gemm(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, int reduction_major,
                   const float* bias, int relu, float* C32, int64_t ldc, void* stream);
/* dropout (torch nn.Dropout inside nn.Transformer*Layer / PositionalEncoding, mono_transformer_torch.py:30-32,74-98): the keep-scale
 * (0 or 1/(1-p)) of element i at a site; the GEMM epilogue and the attention-probability sites with their dropout switched on */
int masr_test_dropout_mask(uint32_t seed, uint32_t site, int64_t n, float p, float* out, void* stream);
int masr_test_gemm_dropout(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, float drop_p,
                           uint32_t seed, uint32_t site, float* C32, int64_t ldc, void* stream);
int masr_test_attention_dropout(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, float* lse, int B, int H,
                                int Tq, int Tk, int hd, float drop_p, uint32_t seed, uint32_t site, void* stream);
/* the NT GEMM with any combination of its fused epilogue stages (tools/bench_gemm_epi.py: what each stage costs per launch) */
int masr_test_gemm_epi(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, const float* bias, int relu,
                       float drop_p, const float* residual, const uint16_t* mask, float* C32, uint16_t* C16, void* stream);
/* ... with the two stages the entry above does not pass: the positional encoding pe fp32 [pe_period][N] added to row m as pe[m % pe_period]
 * (null: none; the vgg2enc launch: bias + pe, fp32 and bf16 output) and accumulation into the fp32 output (C32 += result; the memory gradient
 * summed over decoder layers); C32 with row pitch ldc and/or C16 with row pitch ldc16 */
int masr_test_gemm_pe_acc(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, const float* bias,
                          const float* pe, int pe_period, int accumulate, float* C32, int64_t ldc, uint16_t* C16, int64_t ldc16, void* stream);
/* the decode's few-row GEMM (decode.hip skinny_gemm_kernel, the launch of every decoder Linear of masr_recog / masr_recog_beam):
 * C[M][N] = epi(A[M][K] W[N][K]^T) with bias, ReLU, fp32 residual [M][N], fp32 and/or bf16 output (tools/bench_beam.py: against the NT GEMM) */
int masr_test_skinny_gemm(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, int M, int N, int K, const float* bias, int relu,
                          const float* residual, float* C32, uint16_t* C16, void* stream);
/* the joint beam's CTC prefix-score kernel (beam.hip beam_ctc_prefix_kernel, the per-step launch of masr_recog_beam_ctc) alone, on one
 * hypothesis row over T frames: lp fp32 [C][T] (x_t(c), frame-contiguous per class; blank 0, eos C - 1); the parent as (last, parent, psi_par,
 * score): last = -1 for the empty hypothesis (its state and psi 0 come from the decode's init kernel; parent / psi_par are ignored), else its
 * last token, with its state parent fp32 [T][2] (r^n_t, r^b_t) and prefix score psi_par; n (1..96) pre-beam candidates cand int32 [n]
 * (1 .. C-1, or -1 = none) with their attention log-probs att_lp fp32 [n].  Out: the row's list as the decode step leaves it -- list_tok /
 * list_score / list_psi / list_slot [n] sorted by joint score s + att_w lp + ctc_w (psi - psi_par) (descending, then candidate index), -1 /
 * -inf behind the finite ones -- and the candidates' states out_state fp32 [T][n][2] (columns of eos and of -1: zero).  All arrays on
 * the device; synchronises the stream. */
int masr_test_ctc_prefix(const float* lp, int C, int T, int last, const float* parent, float psi_par, float score, const int32_t* cand,
                         const float* att_lp, int n, float att_w, float ctc_w, int32_t* list_tok, float* list_score, float* list_psi,
                         int32_t* list_slot, float* out_state, void* stream);
/* the decode's one-query attention (decode.hip attn_decode_kernel, every self- and cross-attention of masr_recog / masr_recog_beam) with
 * every field of its launch: q [B][ldq], head h at column h*hd; cache k / v + b*kv_batch_stride + j*ldk + h*hd; the key count is the
 * device scalar *step (self-attention: knew / vnew [B][ldnew] are the newest row, appended to the cache at slot *step - 1) or klens [B]
 * (cross-attention; rows_per_utt > 1: row b reads cache row / klens entry b / rows_per_utt); src (with step only): key j of row b lives in
 * cache row src[(klen & 1) * src_flip + b * ld_src + j].  o bf16 [B][ldo].  Reads the key counts and the src entries back first and
 * refuses a key count outside [1, Tk_cap] or a src entry outside the cache rows; synchronises the stream. */
int masr_test_attn_decode(const uint16_t* q, int64_t ldq, const uint16_t* k, const uint16_t* v, int64_t ldk, int64_t kv_batch_stride,
                          const uint16_t* knew, const uint16_t* vnew, int64_t ldnew, const int32_t* step, const int32_t* klens, uint16_t* o,
                          int64_t ldo, int B, int H, int hd, int Tk_cap, int rows_per_utt, const int32_t* src, int64_t ld_src, int64_t src_flip,
                          void* stream);
/* the greedy decode's fp32 last projection (decode.hip logits_f32_kernel): z [rows][ld] = bias [C] + y32 [rows][E] W32 [C][E]^T; 16-byte
 * loads when y32 and W32 are both 16-byte aligned, 4-byte loads otherwise */
int masr_test_logits_f32(const float* y32, const float* W32, const float* bias, float* z, int64_t ld, int rows, int C, int E, void* stream);
/* the greedy decode's arg-max (decode.hip recog_argmax_step_kernel): out[(step[0] - 1) * B + b] = first maximal index of logits [b][:C]
 * (0 when no value is above -inf); the last row to finish sets step = {step[0] + 1, 0}.  step int32 [2] on the device */
int masr_test_recog_argmax_step(int32_t* step, const float* logits, int64_t ld, int32_t* out, int B, int C, void* stream);
/* one step t of the beam search's glue (beam.hip beam_rows_kernel without an LM + beam_select_kernel<false>) on R = B*K rows of caller-given fp32
 * logits [R][ld].  In: minlen / maxlen [B].  In and out: score [R], fin [B], best_score / best_len / best_row [B], and row t-1 of the
 * token / parent history tok_hist_row / par_hist_row [R] (the entries the step does not write keep the caller's values).  Out: the rows'
 * lists list_tok / list_score [R][K] and the step pair step_out int32 [2].  All arrays on the device; synchronises the stream. */
int masr_test_beam_step(int B, int K, int C, int sos, int eos, int t, const int32_t* minlen, const int32_t* maxlen, const float* logits,
                        int64_t ld, float* score, int32_t* fin, float* best_score, int32_t* best_len, int32_t* best_row, int32_t* list_tok,
                        float* list_score, int32_t* tok_hist_row, int32_t* par_hist_row, int32_t* step_out, void* stream);
/* ---- the training step's row kernels alone (tests/test_hip_train_row_kernels.py).  Each entry vets on the host what the kernel would index
 * with, fills the launcher's arguments and calls it; all arrays on the device.
 * The loss head (rowops.hip ls_ce_kernel + ls_ce_reduce, mk_ls_ce): logits fp32 [rows][ld], gold int32 [rows] (a class, or -1 = not counted) ->
 * dlogits bf16 [rows][ld] (pad columns C .. ld and rows with gold -1: zero), row_loss fp32 [rows], row_correct int32 [rows], stats fp32 [3] =
 * {loss sum * inv_ntotal, number correct, n_total}.  inv_ntotal_ptr (optional, device): read instead of the by-value inv_ntotal, as a replayed
 * step graph does.  grad_w scales dlogits only.  Reads gold back first and refuses ld < C, rows < 1 and a gold value outside [-1, C). */
int masr_test_ls_ce(const float* logits, int64_t ld, const int32_t* gold, int rows, int C, float eps, float inv_ntotal, const float* inv_ntotal_ptr,
                    float grad_w, uint16_t* dlogits, float* row_loss, int32_t* row_correct, float* stats, void* stream);
/* embedding + positional encoding + positional dropout (rowops.hip embed_fwd_kernel): tok int32 [B][L], table fp32 [V][E], pe fp32 [>= L][E] ->
 * y32 / y16 [B][L][E] = (table[tok] + pe[l]) * keep-scale of element (b L + l) E + e at `site`; seed_ptr (optional, device) is read instead of
 * seed.  Refuses a token outside [0, V). */
int masr_test_embed_fwd(const int32_t* tok, const float* table, const float* pe, float* y32, uint16_t* y16, int B, int L, int E, int V, float drop_p,
                        uint32_t seed, uint32_t site, const uint32_t* seed_ptr, void* stream);
/* its backward (folds.h embed_bwd_body): dtable [V][E] (+)= the sum over the positions i that hold token v of dy [n][E] row i times the keep-scale
 * of element i E + col.  Takes the tokens tok int32 [n] and groups the positions by token on the host with the helper masr_run_batch uses.
 * Refuses a token outside [0, V) and E % 64 != 0; synchronises the stream. */
int masr_test_embed_bwd(const int32_t* tok, int n, const float* dy, float* dtable, int V, int E, int accumulate, float drop_p, uint32_t seed,
                        uint32_t site, const uint32_t* seed_ptr, void* stream);
/* y bf16 [n] = bf16(x [n] * keep-scale of element i at `site`) (rowops.hip cast_dropout_kernel: the encoder output gradient on its way to the VGG) */
int masr_test_cast_dropout(const float* x, uint16_t* y, int64_t n, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_ptr, void* stream);
/* vgg2enc's weight gradient from the engine's feature order back to the reference's (folds.h vgg2enc_unpermute_body):
 * dw [E][C][Dp] <- g [E][Dp][C] */
int masr_test_vgg2enc_grad_unpermute(const float* g, float* dw, int E, int C, int Dp, void* stream);
/* the arg-max of the full-sequence greedy decode (rowops.hip recog_argmax_kernel): out int32 [L][B], out[l][b] = first maximal index of logits fp32 [b L + l][:C]
 * (row stride ld; 0 when no value is above -inf) */
int masr_test_recog_argmax(const float* logits, int64_t ld, int32_t* out, int B, int L, int C, void* stream);
/* the operand-shadow pass of masr_refresh on ONE Linear weight: W fp32 [N][K] at P + src (P 16-byte aligned, src any dword offset >= 4 with at
 * least four floats of P behind the tensor -- in the flat parameter buffer the shadowed tensors are neither first nor last) -> k16 bf16 [N][K]
 * and its transpose t16 bf16 [K][ldt] (ldt >= N; the pads of a row stay untouched) */
int masr_test_linear_shadows(const float* P, int64_t src, int N, int K, int ldt, uint16_t* k16, uint16_t* t16, void* stream);
/* the first conv of the VGG front-end (CIN = 1, 64 output channels; mono_transformer_torch.py:49-50) as the engine launches it: x fp32 [B][H][W],
 * w fp32 [64][9], bias fp32 [64] -> out bf16 [B][H][W][64] = ReLU(conv + bias) (fp32 arithmetic on the exact-fp32 MFMA, rounded once) and, when
 * relu_bits is given, one 64-bit word per pixel whose bit c says whether channel c passed the ReLU (what the fused dgrad of the second conv reads) */
int masr_test_conv1_fwd(const float* x, const float* w, const float* bias, uint16_t* out, uint64_t* relu_bits, int B, int H, int W, void* stream);
int masr_test_conv3x3(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, uint16_t* out,
                      int B, int H, int W, int CIN, int COUT, void* stream);
/* dgrad/fused-pool flavours of the same kernel: mask (optional, same shape as out) zeroes outputs where mask <= 0;
   pool_out (optional, [B][H/2][W/2][COUT]) receives MaxPool2d(2,2) of the ReLU'd output */
int masr_test_conv3x3_ex(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, const uint16_t* mask, uint16_t* out,
                         uint16_t* pool_out, int B, int H, int W, int CIN, int COUT, void* stream);
/* 128-channel ReLU masks as sign bits (four dwords per pixel, dword q = the sign bytes of channel groups 8q.., 32+8q.., 64+8q.., 96+8q..):
   a forward launch with 128 output channels writes them for its output (out_sign_bits), a masked 128 <- 128 dgrad reads them
   (mask_bits, next to the bf16 mask it replaces on the streaming path) */
int masr_test_conv3x3_sign_bits(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, const uint16_t* mask, const uint32_t* mask_bits,
                                uint16_t* out, uint32_t* out_sign_bits, int B, int H, int W, int CIN, int COUT, void* stream);
/* the pooling forward conv as the engine launches it: pool_idx ([B][H/2][W/2][COUT] bytes) receives, per pooled element, the
   window position 0..3 (row-major) of its first maximum, or 4 where nothing passed the ReLU; drop_out != 0 allows the launch to
   leave `out` unwritten (the streaming kernels then never store the full-resolution map; the others still do). */
int masr_test_conv3x3_pool_idx(const uint16_t* in, const uint16_t* wk, const float* bias, uint16_t* out, uint16_t* pool_out,
                               uint8_t* pool_idx, int drop_out, int B, int H, int W, int CIN, int COUT, void* stream);
/* The two dgrad launches that sit behind a max-pool (reference: the autograd of nn.MaxPool2d + nn.ReLU in front of nn.Conv2d,
 * mono_transformer_torch.py:51-52,57-58).  Input either as the map dy [B][H][W][C] or -- dy == NULL -- as the pooled gradient dy_pooled
 * [B][H/2][W/2][C] + the codes of masr_test_conv3x3_pool_idx, expanded while the patches are staged (no map in memory): same bits.
 * masr_test_conv3x3_dgrad_pooled: 128 <- 128 channels through the ReLU mask given as sign words (masr_test_conv3x3_sign_bits).
 * masr_test_conv1_wgrad_fused: 64 <- 64 channels whose output is contracted with the network input x1 [B][H][W] inside the launch:
 * dw1 [64][9], db1 [64] = the weight / bias gradient of the FIRST conv; mask_bits = one 64-bit word of sign bits per pixel. */
int masr_test_conv3x3_dgrad_pooled(const uint16_t* dy, const uint16_t* dy_pooled, const uint8_t* pool_idx, const uint16_t* wk, const uint32_t* mask_bits,
                                   uint16_t* out, int B, int H, int W, void* stream);
int64_t masr_test_conv1_wgrad_fused_slab_floats(int B, int H, int W);
int masr_test_conv1_wgrad_fused(const uint16_t* dy, const uint16_t* dy_pooled, const uint8_t* pool_idx, const uint16_t* wk, const uint64_t* mask_bits,
                                const float* x1, float* slab, int64_t slab_floats, float* dw1, float* db1, int B, int H, int W, void* stream);
int masr_test_conv3x3_wgrad(const uint16_t* in, const uint16_t* dy, float* dw, float* slab, int64_t slab_floats,
                            int B, int H, int W, int CIN, int COUT, void* stream);
int64_t masr_test_conv3x3_wgrad_slab_floats(int B, int H, int W, int CIN, int COUT);
/* n > 0: every persistent conv grid of this process (the 3x3 forward / dgrad kernels, the two weight-gradient kernels, conv1 forward) is capped
 * at n workgroups, whatever the launch's `shared` hint says; 0 restores the normal rule (capped only beside other task slots).  Process-wide.
 * No result depends on it: it lets tiny shapes reach the capped paths (tests/test_hip_conv_grid_cap.py). */
void masr_test_set_conv_grid_cap(int n);
/* Linear weight gradients as a grouped launch (mk_gemm_wgrad_grouped: one grid of 256 x 256 tiles): dW[N][K] = dy[rows][N]^T x[rows][K], db[N] =
 * column sums of dy (or null); a second member with the same operands when dW2 is given.
 * _n: `members` members over the same operands (member i writes dW + i * member_stride); first_members > 0: the two-segment tile list of the
 * engine's merged launch -- members [0, first_members) reduce over `rows` rows and are dispatched first, the others over the first rows_rest. */
int masr_test_wgrad_grouped(const uint16_t* dy, int64_t lddy, const uint16_t* x, int64_t ldx, float* dW, float* db, float* dW2, float* db2,
                            int rows, int N, int K, void* stream);
/* the k-split GEMM + summing LayerNorm pair of the decoder (train.hip ffn_fwd / ffn_bwd / ln_bwd, engine_internal.h ln_fwd): forward when x == NULL, backward otherwise */
int masr_test_ksplit_ln(const uint16_t* A, const uint16_t* B, int rows, int E, int K, int split, const float* bias, const float* residual, float drop_p,
                        uint32_t seed, uint32_t site, float* part, const float* gamma, const float* beta, float* sum_out, float* y32, uint16_t* y16,
                        float* mean, float* rstd, const float* x, float* dx32, uint16_t* dx16, float* slab, void* stream);
int masr_test_wgrad_grouped_n(const uint16_t* dy, int64_t lddy, const uint16_t* x, int64_t ldx, float* dW, int64_t member_stride, int members,
                              int first_members, int rows, int rows_rest, int N, int K, void* stream);
/* the same with dy given as the pooled gradient [B][H/2][W/2][COUT] + the pool codes of masr_test_conv3x3_pool_idx (the weight-gradient kernel
 * expands the 2x2 max-pool + ReLU backward while staging; 64->64 and 128->128 channels); db may be null */
int masr_test_conv3x3_wgrad_pooled(const uint16_t* in, const uint16_t* dy_pooled, const uint8_t* pool_idx, float* dw, float* db, float* slab,
                                   int64_t slab_floats, int B, int H, int W, int CIN, int COUT, void* stream);
/* LayerNorm forward + backward of one [rows][E] fp32 matrix (nn.LayerNorm inside nn.Transformer*Layer, mono_transformer_torch.py:74-98):
 * y, y16 (bf16), mean / rstd per row; dx, dgamma, dbeta from dy.  slab: masr_test_layernorm_slab_floats(rows, E) floats of scratch. */
int64_t masr_test_layernorm_slab_floats(int rows, int E);
int masr_test_layernorm(const float* x, const float* gamma, const float* beta, const float* dy, float* y, uint16_t* y16, float* mean,
                        float* rstd, float* dx, uint16_t* dx16, float* dgamma, float* dbeta, float* slab, int rows, int E, float drop_p,
                        uint32_t seed, uint32_t site, void* stream);   /* dx16 = bf16(dx * keep-scale of element row * E + col at `site`) */
/* forward + backward of one attention with dropout on the probabilities (keep-scale of element ((b H + h) Tq + i) Tk + j at `site`,
 * masr_test_dropout_mask): the backward regenerates the masks of the forward from (seed, site, index) */
int masr_test_attention_dropout_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o, uint16_t* dq, uint16_t* dk,
                                    uint16_t* dv, float* lse, const int32_t* klens, int B, int H, int Tq, int Tk, int hd, int causal, float drop_p,
                                    uint32_t seed, uint32_t site, void* stream);
/* ... under a chunk mask (include/masr.h masr_chunk_policy; Tq == Tk, causal == 0): `chunk` / `left` by value, or the chunk read from device
 * memory where chunk_dev is non-null (then `chunk` is not read; a 0 there is full context).  -1 with a message, before any launch, for a chunk
 * together with causal, Tq != Tk, chunk < 0 or left < -1.  chunk = 0 with chunk_dev = null is masr_test_attention_dropout_bwd. */
int masr_test_attention_chunk(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o, uint16_t* dq, uint16_t* dk,
                              uint16_t* dv, float* lse, const int32_t* klens, int B, int H, int Tq, int Tk, int hd, int causal, float drop_p,
                              uint32_t seed, uint32_t site, int chunk, int left, const int32_t* chunk_dev, void* stream);
int masr_test_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o,
                        uint16_t* dq, uint16_t* dk, uint16_t* dv, float* lse, float* delta, const int32_t* klens,
                        int B, int H, int Tq, int Tk, int hd, int causal, void* stream);
/* The chunk step's self-attention against a K|V cache, alone (csrc/stream.hip attn_stream_kernel): q / knew / vnew / o bf16
 * [B][R][H * hd], the cache kc / vc bf16 [B][cap][H * hd] each.  Every query row attends the keys [lo, min(pos + R, klens[b])) (klens null:
 * pos + R): cache rows in front of pos, knew / vnew from pos on; the launch also copies knew / vnew into the cache rows [pos, pos + R).  A row
 * without a key gets o = 0.  -1 with a message, before any launch: R < 1, pos + R > cap, lo > pos, hd outside {16, 32, 64}. */
int masr_test_attention_stream(const uint16_t* q, const uint16_t* knew, const uint16_t* vnew, uint16_t* kc, uint16_t* vc, uint16_t* o,
                               const int32_t* klens, int B, int H, int hd, int R, int pos, int lo, int cap, void* stream);
/* The streamed greedy CTC decode, alone (csrc/stream.hip ctc_greedy_stream_kernel): logits fp32 [B][R][ld] = the frames pos .. pos + R, C valid
 * columns, blank 0; state int32 [2][B] (previous arg-max | len, all 0 at the start) is read and written; a frame < klens[b] (null: every frame)
 * whose arg-max (ties to the lower index) is neither blank nor the previous frame's appends to tokens / frames int32 [B][ld_out]. */
int masr_test_ctc_greedy_stream(const float* logits, int64_t ld, const int32_t* klens, int B, int R, int C, int pos, int32_t* state, int32_t* tokens,
                                int32_t* frames, int ld_out, void* stream);
/* where the last masr_recog_ctc_beam call with this B, T, K left the inputs of its masr_ctc_beam_search in the bound workspace: the CTC
 * head's fp32 logits (row of utterance b, frame t at logits + (b * (T / 4) + t) * ld, C = odim valid columns) and enc_lens int32 [B].
 * Valid until the next call that uses the workspace. */
int masr_test_ctc_beam_logits(masr_model* m, int B, int T, int K, float** logits, int64_t* ld, int32_t** enc_lens);
/* the same for the last masr_recog_ctc_align call with this B, T, maxL: the inputs of its masr_ctc_align */
int masr_test_ctc_align_logits(masr_model* m, int B, int T, int maxL, float** logits, int64_t* ld, int32_t** enc_lens);
/* include/masr.h's masr_ctc_align, with its arguments and refusals, whose sweep ends behind the score: no back-trace, and frames / start / end of a
 * feasible utterance are left as they were.  For tools/bench_ctc_align.py: the difference to the whole call is what the back-trace and the
 * start / end pass cost. */
int masr_test_ctc_align_no_trace(const float* logits, int64_t ld, const int32_t* enc_lens, const int32_t* targets, const int32_t* tgt_off,
                                 const int32_t* tgt_len, int B, int Tp, int C, int blank, int maxL, void* work, int64_t work_bytes, int32_t* frames,
                                 int32_t* start, int32_t* end, float* score, void* stream);
/* ---- attention rescoring (rescore.hip; tests/test_hip_rescore_kernels.py, tests/test_hip_rescore.py)
 * the score kernel alone (mk_rescore_score): logits fp32 [R*L][ld] (C <= ld valid columns), gold int32 [R*L] (-1 = no term; >= C is read as
 * no term) -> att fp32 [R] = the sum over l ascending of log_softmax(logits[r*L + l])[gold], -inf where a hypothesis has no term; row_lp fp32
 * [R*L] scratch (the terms) */
int masr_test_rescore_score(const float* logits, int64_t ld, const int32_t* gold, int R, int L, int C, float* row_lp, float* att, void* stream);
/* the select kernel alone (mk_rescore_select): the outputs of masr_rescore_nbest from lists, first-pass scores and attention scores att_in
 * [B][N]; 1 <= N <= 64, outputs apart from the inputs */
int masr_test_rescore_select(const int32_t* tokens_in, int64_t ld_tok, const int32_t* lens_in, const float* ctc_in, const float* att_in, int B, int N,
                             float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc, int32_t* order,
                             void* stream);
/* where the last masr_recog_rescore / masr_rescore_nbest call on m left what its score kernel read in the bound workspace: the decoder's
 * fp32 logits (row r * L + l at logits + (r * L + l) * ld, odim valid columns; r = b * N + first-pass rank) and gold int32 [R][L].  Valid until
 * the next call that uses the workspace; -1 before the first rescoring call and after masr_bind. */
int masr_test_rescore_logits(masr_model* m, float** logits, int64_t* ld, int32_t** gold, int* R, int* L);
/* ---- n-gram LM shallow fusion (lm.hip; tests/test_hip_lm_kernels.py)
 * the LM's score rule alone: ctx int32 [R][order - 1] (null at order 1), oldest first, -1 = nothing further left (a shorter context has its
 * -1 in front) -> out fp32 [R][C] = lm(c | ctx) for every class.  Reads ctx back first and refuses an id outside [-1, C) and a -1 behind an id;
 * all arrays on the device; synchronises the stream. */
int masr_test_lm_score(const masr_lm* lm, const int32_t* ctx, int R, float* out, void* stream);
/* the longest probe chain (slots examined) an insertion walked while the LM's tables were built; 1 = no n-gram ever met an occupied slot */
int masr_test_lm_max_probe(const masr_lm* lm);
/* ---- contextual phrase biasing (bias.hip; tests/test_hip_bias_kernels.py)
 * the automaton's step on `count` independent states (device int32 arrays): (nodes_out, n_out)[i] = step((nodes_in, n_in)[i], tokens[i]) by the
 * __device__ function the sweep calls; a node outside the trie gives (-1, -1), a token outside [0, C) has no child.  Waits for the stream. */
int masr_test_bias_step(const masr_bias* bias, const int32_t* nodes_in, const int32_t* n_in, const int32_t* tokens, int count, int32_t* nodes_out,
                        int32_t* n_out, void* stream);
/* the longest probe chain an insertion into the phrase table walked (slots examined) */
int masr_test_bias_max_probe(const masr_bias* bias);
/* the beam's row stage with the n-gram LM alone (beam.hip beam_rows_kernel, top-K) at step t >= 1 on R = B*K rows of caller-given fp32 logits [R][ld] (C = the LM's classes
 * <= ld): score fp32 [R] (-inf = dead row), minlen int32 [B], and the token / parent-row histories of the steps before, tok_hist / par_hist
 * int32 [t - 1][R] (null at t = 1; the kernel clamps what it reads).  Out: list_tok int32 / list_score fp32 [R][K].  The fused rows and the
 * step scalar are the entry's; no utterance is finished.  All arrays on the device; synchronises the stream. */
int masr_test_beam_lm_topk(const masr_lm* lm, float lm_w, int B, int K, int t, const int32_t* minlen, const float* logits, int64_t ld,
                           const float* score, const int32_t* tok_hist, const int32_t* par_hist, int32_t* list_tok, float* list_score, void* stream);

/* ---- the joint LM beam's step kernels alone (tests/test_hip_joint_lm_kernels.py).  All arrays on the device; each entry
 * synchronises the stream.
 * the fused pre-beam (the same kernel, pre-beam): masr_test_beam_lm_topk's inputs; P = floor(3K/2).  Out: pre_tok int32 / pre_lp / pre_lm
 * fp32 [R][P] -- the row's P best classes by g (blank never, eos from minlen on; -1 / -inf / 0 past the end), their attention log-probs and
 * fl(lm_w * lm(c | h)).  A dead row's entries are left as the caller gave them. */
int masr_test_joint_lm_prebeam(const masr_lm* lm, float lm_w, int B, int K, int t, const int32_t* minlen, const float* logits, int64_t ld,
                               const float* score, const int32_t* tok_hist, const int32_t* par_hist, int32_t* pre_tok, float* pre_lp, float* pre_lm,
                               void* stream);
/* the row stage with caller-given LM logit rows (the LSTM LM's place in masr_recog_beam_nlm and masr_recog_beam_ctc_nlm, DESIGN 5.10 / 5.11;
 * tests/test_hip_nlm_joint_kernels.py): lm_logits fp32 [R][ld_lm] over C classes (2 <= C <= ld_lm, ld), the rest as masr_test_beam_lm_topk; no
 * history is read.  lm(c) = the row's log-softmax.  pre_tok null: the top-K form, out list_tok int32 / list_score fp32 [R][K].  pre_tok given:
 * the pre-beam form, out pre_tok int32 / pre_lp / pre_lm fp32 [R][P] as masr_test_joint_lm_prebeam gives them, P = floor(3K/2). */
int masr_test_beam_nlm_rows(const float* lm_logits, int64_t ld_lm, float lm_w, int B, int K, int C, int t, const int32_t* minlen, const float* logits,
                            int64_t ld, const float* score, int32_t* list_tok, float* list_score, int32_t* pre_tok, float* pre_lp, float* pre_lm,
                            void* stream);
/* masr_test_ctc_prefix through beam_ctc_prefix_kernel<LM>: pre_lm fp32 [n] the candidates' weighted LM terms, len_bonus added to a token's score
 * (not to eos's); list_score = fl(fl(fl(fl(score + fl(att_w lp)) + fl(ctc_w fl(psi - psi_par))) + pre_lm) + b) */
int masr_test_ctc_prefix_lm(const float* lp, int C, int T, int last, const float* parent, float psi_par, float score, const int32_t* cand,
                            const float* att_lp, const float* pre_lm, int n, float att_w, float ctc_w, float len_bonus, int32_t* list_tok,
                            float* list_score, float* list_psi, int32_t* list_slot, float* out_state, void* stream);
/* one step t of the select with the N-best list (beam.hip beam_select_nbest_kernel) on caller-given sorted row lists list_tok / list_score /
 * list_psi / list_slot [B*K][P], P = floor(3K/2), eos = C - 1.  In / out: fin int32 [B], nb_score fp32 / nb_len / nb_row int32 [B][N] (the list
 * state), tok_hist_row / par_hist_row int32 [B*K] (row t - 1 of the histories, so untouched entries show).  Out: score / psi fp32 [B*K], src int32
 * [B*K], step_out int32 [2] (the step scalar and the ticket after the launch). */
int masr_test_beam_select_nbest(int B, int K, int N, int C, int t, const int32_t* maxlen, float len_bonus, const int32_t* list_tok,
                                const float* list_score, const float* list_psi, const int32_t* list_slot, float* score, float* psi, int32_t* src,
                                int32_t* fin, float* nb_score, int32_t* nb_len, int32_t* nb_row, int32_t* tok_hist_row, int32_t* par_hist_row,
                                int32_t* step_out, void* stream);

/* ---- the phrase-biased step kernels alone (tests/test_hip_bias_beam_kernels.py).  All arrays on the device; each entry synchronises
 * the stream.
 * the biased row stage (beam_rows_kernel<Lm, PRE, true>) at step t on masr_test_beam_lm_topk's inputs (lm may be NULL: f = lp; C = the list's
 * classes) plus maxlen int32 [B] and state_in int32 [R][2] = (node, credited tokens) of every row's PARENT row at step t - 1 (indexed by the parent
 * row as par_hist names it; null at t = 1; a node outside the trie is refused).  Out: state_out int32 [R][2], the state of every live row's
 * hypothesis (dead rows: zero).  pre_tok null: the top-K form, list_tok int32 / list_score fp32 [R][K].  pre_tok given: the pre-beam form, pre_tok
 * int32 / pre_lp / pre_lm / pre_b fp32 [R][P], P = floor(3K/2); lm_w and bias_w are then read from the device as the decode reads them. */
int masr_test_beam_bias_rows(const masr_lm* lm, const masr_bias* bias, float lm_w, float bias_w, int B, int K, int t, const int32_t* minlen,
                             const int32_t* maxlen, const float* logits, int64_t ld, const float* score, const int32_t* tok_hist, const int32_t* par_hist,
                             const int32_t* state_in, int32_t* state_out, int32_t* list_tok, float* list_score, int32_t* pre_tok, float* pre_lp,
                             float* pre_lm, float* pre_b, void* stream);
/* one step t of the attention beam's select with the stop bound of bias_w (beam_select_kernel<false, true>) on caller-given sorted row lists
 * list_tok / list_score [B*K][K]; sos 0, eos = C - 1; the other arguments as masr_test_beam_step's */
int masr_test_beam_select_bias(int B, int K, int C, int t, const int32_t* maxlen, float bias_w, const int32_t* list_tok, const float* list_score,
                               float* score, int32_t* fin, float* best_score, int32_t* best_len, int32_t* best_row, int32_t* tok_hist_row,
                               int32_t* par_hist_row, int32_t* step_out, void* stream);
/* masr_test_beam_select_nbest through beam_select_nbest_kernel<true>: the stop bound allows fl(max(len_bonus, 0) + bias_w) per further token */
int masr_test_beam_select_nbest_bias(int B, int K, int N, int C, int t, const int32_t* maxlen, float len_bonus, float bias_w, const int32_t* list_tok,
                                     const float* list_score, const float* list_psi, const int32_t* list_slot, float* score, float* psi, int32_t* src,
                                     int32_t* fin, float* nb_score, int32_t* nb_len, int32_t* nb_row, int32_t* tok_hist_row, int32_t* par_hist_row,
                                     int32_t* step_out, void* stream);

/* ---- the BLSTM path's LSTM kernels alone (lstm.hip, lstm_rec.hip; tests/test_hip_lstm_kernels.py).  Rows are batch-first (b * T + t), the gate
 * axis is unit-major (row / column u * 4 + g, g in torch's order i, f, g, o), index 0 / 1 = forward / reverse direction, KP = H rounded up to a
 * multiple of 32.  Each entry vets on the host what the kernel would index with, calls the launcher and synchronises the stream.
 * The weight shadows of one direction of one layer (mk_lstm_shadows): wih fp32 [4H][K], whh fp32 [4H][H], bih / bhh fp32 [4H] in torch's row order
 * g * H + u -> wih16 bf16 [4H][K] (unit-major rows; pc > 0: column d * pc + c holds torch's column c * pd + d, K == pc * pd), its transpose
 * wihT16 [K][4H], whh16 bf16 [4H][KP] (columns H .. KP zero), whhT16 bf16 [H][4H], bias fp32 [4H] = bih + bhh (unit-major). */
int masr_test_lstm_shadows(const float* wih, const float* whh, const float* bih, const float* bhh, int H, int K, int pc, int pd, uint16_t* wih16,
                           uint16_t* wihT16, uint16_t* whh16, uint16_t* whhT16, float* bias, void* stream);
/* a gradient back to torch's order (mk_lstm_unperm): src fp32 [4H][K] (unit-major rows, the shadow's column order) -> dst [4H][K] and, when given,
 * dst2 with the same values (the two biases, K = 1) */
int masr_test_lstm_unperm(const float* src, float* dst, float* dst2, int H, int K, int pc, int pd, void* stream);
/* the recurrence forward through time, both directions: lens int32 [B], gx0 / gx1 fp32 [B*T][4H] (input contribution + biases), whh16_0 / whh16_1
 * bf16 [4H][KP] -> y16 bf16 [B*T][2H] (forward | reverse halves; zero at t >= len), act0 / act1 fp32 [B*T][4H] and c0 / c1 fp32 [B*T][H] (rows t >= len
 * are not written).  resident == 0: one launch per timestep (mk_lstm_fwd_steps); resident == 1: one launch (mk_lstm_fwd_rec) with exchange words and an
 * error word of the entry's own -- a non-zero error word after the launch returns < 0 ("timed out").  The ping-pong and running-state buffers are the
 * entry's.  Refuses lens outside [1, T] and, with resident == 1, shapes for which the resident recurrence is not built (B > 32, KP > 384, 4H % 32). */
int masr_test_lstm_fwd(int resident, int B, int T, int H, const int32_t* lens, const float* gx0, const float* gx1, const uint16_t* whh16_0,
                       const uint16_t* whh16_1, uint16_t* y16, float* act0, float* act1, float* c0, float* c1, void* stream);
/* the recurrence backward through time: dy fp32 [B*T][2H], the forward's act / c, whhT16_0 / whhT16_1 bf16 [H][4H] -> dz16_0 / dz16_1 bf16 [B*T][4H]
 * (zero at t >= len).  mk_lstm_bwd_steps / mk_lstm_bwd_rec; the refusals of masr_test_lstm_fwd, and 4H % 32 != 0 in both forms. */
int masr_test_lstm_bwd(int resident, int B, int T, int H, const int32_t* lens, const float* dy, const float* act0, const float* act1, const float* c0,
                       const float* c1, const uint16_t* whhT16_0, const uint16_t* whhT16_1, uint16_t* dz16_0, uint16_t* dz16_1, void* stream);
/* h_{t-1} as the forward pass saw it (mk_lstm_hprev): y16 bf16 [B*T][2H] -> hp0 [B*T][KP] = y16[b][t-1][0:H], hp1 = y16[b][t+1][H:2H], zero at the
 * sequence ends and in columns H .. KP */
int masr_test_lstm_hprev(const uint16_t* y16, uint16_t* hp0, uint16_t* hp1, int B, int T, int H, int KP, void* stream);
/* x fp32 [rows][C] -> y bf16 [rows][Cp], columns C .. Cp zero (mk_cast_rows_pad) */
int masr_test_cast_rows_pad(const float* x, uint16_t* y, int64_t rows, int C, int Cp, void* stream);
/* dy == NULL: y32 [n] = tanh(x [n]), out16 = bf16(y32) (mk_tanh_fwd); else out16 [n] = bf16(dy (1 - x^2)) with x = the forward's y32 (mk_tanh_bwd) */
int masr_test_tanh(const float* x, const float* dy, float* y32, uint16_t* out16, int64_t n, void* stream);
/* rows (b, t >= lens[b]) of x32 fp32 / x16 bf16 [B*T][C] (either may be null) -> 0 (mk_mask_rows) */
int masr_test_mask_rows(float* x32, uint16_t* x16, const int32_t* lens, int B, int T, int C, void* stream);
/* time sub-sampling.  dys == NULL: ys bf16 [B][Tout][C] = y bf16 [B][Tin][C] rows t' * sub (mk_subsample_rows, C % 8 == 0); else its backward
 * dy fp32 [B][Tin][C] = dys fp32 [B][Tout][C] at t % sub == 0, zero elsewhere (mk_subsample_rows_bwd, C % 4 == 0).  Tout == ceil(Tin / sub). */
int masr_test_subsample_rows(const uint16_t* y, uint16_t* ys, const float* dys, float* dy, int B, int Tin, int Tout, int sub, int C, void* stream);
/* one step of the LSTM LM's layer stack alone (nlm.hip: the L nlm_lstm_step launches and the output projection of masr_recog_beam_nlm's step) as
 * step t >= 1 on R rows, K rows per utterance (R % K == 0).  t == 1: every row feeds the LM's start token from the zero state, tok / par are not
 * read.  t > 1: row r feeds tok[r] (an id outside [0, C) reads as 0) and continues the state of row par[r] (null: r itself; outside the rows
 * of r's utterance: r).  hstate bf16 / cstate fp32 [2][L][R][Hp], Hp = H padded to 32: the caller's previous states at parity (t - 1) & 1 are
 * read, the new ones are written at parity t & 1.  score fp32 [R] (null: every row live): a row with -inf writes nothing.  logits fp32
 * [R][ld], ld >= C: the LM logits of the live rows; logp (null: skipped) fp32 [R][ld]: their log_softmax as the beam composes it,
 * (y - mx) - log_s.  Synchronises the stream. */
int masr_test_nlm_step(const masr_nlm* nlm, int R, int K, int t, const int32_t* tok, const int32_t* par, const float* score, uint16_t* hstate,
                       float* cstate, float* logits, int64_t ld, float* logp, void* stream);
/* the same step in its carry form (nlm.h mk_nlm_step_carry: the LM advance of masr_ctc_beam_search_nlm, DESIGN 5.12;
 * tests/test_hip_ctc_nlm_beam_kernel.py).  tok / par int32 [R]: tok[r] in [1, C - 2] is row r's token, anything else marks a stay; par[r] its
 * parent row (outside the rows of r's utterance: r).  live int32 [2][R / K]: row r of utterance u is live when r - u * K < live[t & 1][u].  A token
 * row equals masr_test_nlm_step's, bit for bit, and its log_softmax goes to logp[t & 1][r]; a stay row gets its parent's (h, c) of every layer
 * and its parent's logp row of parity (t - 1) & 1; a dead row is left as the caller gave it.  logp fp32 [2][R][ld].  t == 1: every live row
 * feeds the start token from the zero state.  Synchronises the stream. */
int masr_test_nlm_step_carry(const masr_nlm* nlm, int R, int K, int t, const int32_t* tok, const int32_t* par, const int32_t* live, uint16_t* hstate,
                             float* cstate, float* logits, int64_t ld, float* logp, void* stream);

/* ---- the flat optimiser passes and the operand-shadow kernels alone (optim.hip; tests/test_hip_optim_kernels.py, tests/test_hip_shadow_kernels.py).
 * All arrays on the device unless said otherwise; each entry vets on the host what the kernel would index with, calls the launcher and
 * synchronises the stream.
 * the gradient norm (sumsq_kernel + sumsq_final, mk_sumsq) with a slab of the entry's own: out_norm[0] = sqrt(sum x[0 .. n)^2), accumulated in
 * fp64.  Refuses n < 1 and an x that is not 16-byte aligned (the kernel reads float4 at every multiple of four floats). */
int masr_test_sumsq(const float* x, int64_t n, float* out_norm, void* stream);
/* clip + SGD (clip_sgd_kernel, mk_clip_sgd) on a caller-given device norm fp32 [1] (null: the unclipped step).  step_flags: bit 0 = the
 * optimiser's first step (no buffer read), bit 1 = its last (no buffer written).  mom may be null only when momentum == 0 or both bits are set. */
int masr_test_clip_sgd(float* p, const float* g, float* mom, int64_t n, const float* norm, float max_norm, float lr, float momentum, int nesterov,
                       int step_flags, void* stream);
/* acc += coef g / g *= coef with coef from the device norm (clip_axpy_kernel / clip_scale_kernel); nan_zero: a NaN norm leaves acc alone /
 * zeroes g instead of spreading NaNs */
int masr_test_clip_axpy(float* acc, const float* g, int64_t n, const float* norm, float max_norm, int nan_zero, void* stream);
int masr_test_clip_scale(float* g, int64_t n, const float* norm, float max_norm, int nan_zero, void* stream);
/* the Adam step the device skips under a NaN norm (adam_guarded_kernel, mk_adam_guarded): scalars A = (lr_a, t_a) when the launch before
 * was applied, B = (lr_b, t_b) when it was skipped, as flags[slot ^ 1] says; flags int32 [2] on the device, slot 0 or 1; t_a, t_b >= 1 */
int masr_test_adam_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr_a, int t_a, float lr_b, int t_b, float b1, float b2,
                           float eps, float weight_decay, int decoupled, const float* norm, int32_t* flags, int slot, void* stream);
/* ONE launch of the shadow refresh (all_shadows_kernel, mk_all_shadows) over a caller-given job list, built as masr_bind builds its own
 * (tile_start from the jobs' workgroup counts, in list order).  desc: HOST array of n_jobs rows {src, type, N, K, ldt, a0, a1} (type: 0 Linear
 * [N][K] -> k16 [N][K], t16 [K][ldt]; 1 conv [CO = N][CI = K][3][3] -> wk, wd; 2 vgg2enc [E = N][C = a0][Dp = a1] -> wk [E][Dp C], its
 * transpose [Dp C][E]; 3 copy of N floats); outs: HOST array of 2 n_jobs device pointers (job i: outs[2 i], outs[2 i + 1]; the second of a
 * copy is not used).  P 16-byte aligned; a Linear job reads up to three floats in front of its rows and behind them.  Refuses n_jobs
 * outside [1, 56], a type outside 0..3, a negative src, a Linear job with src < 4 or ldt < N, non-positive sizes, and a null output where
 * the job's type writes one. */
int masr_test_shadow_jobs(const float* P, int n_jobs, const int64_t* desc, void* const* outs, void* stream);
/* the BLSTM engine's shadow passes: y bf16 [C][ldy] = x fp32 [R][C] transposed (ldy >= R; pads untouched); y bf16 [n] = x fp32 [n];
 * w fp32 [CO][CI][3][3] -> wk bf16 [CO][tap CI + ci] and (wd may be null) wd bf16 [CI][(8 - tap) CO + co] */
int masr_test_transpose_cast_bf16(const float* x, uint16_t* y, int R, int C, int64_t ldy, void* stream);
int masr_test_cast_bf16(const float* x, uint16_t* y, int64_t n, void* stream);
int masr_test_conv_weight_shadows(const float* w, uint16_t* wk, uint16_t* wd, int CO, int CI, void* stream);

/* ---- the CTC loss kernels alone (ctc.hip: ctc_lse_kernel, ctc_sweep_kernel, ctc_grad_kernel, ctc_mean_kernel, ctc_mix_kernel;
 * tests/test_hip_ctc_loss_kernels.py against tests/ctc_loss_ref.py).  All arrays on the device.
 * include/masr.h's CTC loss entry with its arguments, refusals and status word (masr_ctc_status on the same work buffer), and the launcher's
 * batch_first flag exposed: set, logits and grad are [B][T][C] (what the BLSTM engine passes), else [T][B][C].  Does not synchronise. */
int masr_test_ctc_loss_layout(const float* logits, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int T,
                              int B, int C, int blank, float* nll, float* loss, float* grad, float* work, int maxS, void* stream, int batch_first);
/* the transformer's joint form (mk_ctc_loss_joint as train.hip ctc_forward calls it): logits fp32 [B][T][ld] with C <= ld valid columns, blank 0;
 * nll fp32 [B]; stats[0] (the decoder's CE on entry) becomes (1 - w) stats[0] + w mean_b(nll_b / max(tgt_len_b, 1)); grad16 bf16 [B][T][ld] =
 * w * d CTC / d logits with the pad columns C .. ld zero on every row, or null: forward only.  work: as many floats as masr_ctc_work_floats gives for T, B, maxS.
 * This path has no device-side status word, so the entry reads in_len, tgt_len, tgt_off and the targets back and refuses, before any launch:
 * in_len outside [0, T], a negative tgt_len or tgt_off, 2 tgt_len + 1 > maxS, a target id outside [1, C); and with the launcher: maxS > 2048,
 * C > 4096, ld < C, ld % 8 != 0 with a gradient.  Synchronises the stream. */
int masr_test_ctc_loss_joint(const float* logits, int64_t ld, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len,
                             const int32_t* tgt_len, int T, int B, int C, float* nll, uint16_t* grad16, float w, float* stats, float* work, int maxS,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
