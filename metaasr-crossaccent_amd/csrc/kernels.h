// Internal launch API of the libmasr kernels (C++ side; the public C ABI is include/masr.h).
// Every launcher is stream-ordered, allocates nothing, never synchronises (graph-capturable).
#pragma once
#include "common.h"

// ---------------------------------------------------------------- GEMM (gemm.hip)
struct GemmArgs {
    // C[m][n] = epi( alpha * sum_k A(m,k) B(n,k) )
    const bf16* A; long lda;      // reduction_major=0: A[m*lda + k]   =1: A[k*lda + m]
    const bf16* B; long ldb;      // reduction_major=0: B[n*ldb + k]   =1: B[k*ldb + n]
    int M, N, K;
    int reduction_major;          // 1 = both operands have the reduction index as the slow index (wgrad)
    float alpha;
    const float* bias;            // [N] or null
    const float* pe; int pe_period;   // add pe[(m % pe_period)*N + n]
    int relu;
    const bf16* mask; long ldmask; float mask_scale;   // v = mask>0 ? v*mask_scale : 0
    float drop_p; uint32_t seed, site;                 // dropout on element index m*N+n
    const uint32_t* seed_ptr;                          // non-null: the seed is read from device memory (graph-replayed steps)
    const float* residual; long ldres;                 // + residual[m*ldres + n]
    float* colsum;                // reduction-major only: colsum[m] = sum_k A(m,k) (fused bias gradient) or null
    int split_k;                  // reduction-major only: >1 splits the reduction over gridDim.z workgroups; split 0 writes
    long split_delta, split_stride;   // C32/colsum, split z>0 writes the same addresses + split_delta + (z-1)*split_stride (mk_split_reduce combines)
    int accumulate;               // C32 += v
    int xcd_order;                // set by mk_gemm: XCD-contiguous tile order
    int lean;                     // the GPU is shared with other task streams (masr_set_concurrency > 1): forms with the smaller LDS footprint
    float* C32; long ldc;         // fp32 output or null
    bf16* C16; long ldc16;        // bf16 output or null
    // segmented fp32 output rows (grouped weight gradients: one GEMM whose M axis spans several Linear layers that sit at a
    // constant distance from each other in the flat gradient buffer): row m lives at C32 + (m / cseg_rows) * cseg_stride +
    // (m % cseg_rows) * ldc, colsum[m] at colsum + (m / cseg_rows) * cseg_stride + m % cseg_rows.  cseg_rows = 0: plain rows;
    // otherwise a multiple of the 128-row tile.
    int cseg_rows; long cseg_stride;
};
int mk_gemm(const GemmArgs& g, hipStream_t s);
// Linear weight gradients as one grouped launch: dW[N][K] = dy[rows][N]^T x[rows][K], db[N] = column sums of dy (or null)
struct WgradDesc { const bf16* dy; const bf16* x; float* dW; float* db; int lddy, ldx, rows, N, K, tile_start; };
constexpr int WGRAD_GROUP_MAX = 40;
struct WgradGroup { int n; WgradDesc p[WGRAD_GROUP_MAX]; };
// ONE grid of 256 x 256 tiles on eight waves (LDS-DMA ring) over all members; fills tile_start.  first_members > 0: members [0, first_members)
// are dispatched first (the engine's merged launch: long encoder-row reductions, then the short decoder-row ones)
int mk_gemm_wgrad_grouped(WgradGroup& grp, hipStream_t s, int first_members = 0);
inline GemmArgs gemm_args() { GemmArgs g{}; g.alpha = 1.f; g.mask_scale = 1.f; return g; }

// ---------------------------------------------------------------- conv front-end (conv.hip)
// activations NHWC bf16: [B][H][W][C]; x input fp32 [B][H][W] (C=1)
// relu_bits (optional): [B][H][W] 64-bit words, bit c = (out[..][c] > 0) -- ConvArgs::mask_bits of the next conv's fused dgrad
int mk_conv1_fwd(const float* x, const float* w /*[64][9]*/, const float* bias, bf16* out, int B, int H, int W, hipStream_t s, unsigned long long* relu_bits = nullptr);
long mk_conv1_wgrad_slab_floats(int B, int H, int W);
// implicit-GEMM 3x3 pad 1: out[p][co] = epi( sum_{tap,ci} in[p+off(tap)][ci] * wk[co][tap*CIN+ci] )
struct ConvArgs {
    const bf16* in; const bf16* wk; const float* bias; int relu;
    // the input map given as a 2x2 max-pool (+ ReLU) backward that is never materialised: in_pooled [B][H/2][W/2][CIN] (the pooled gradient)
    // under the codes in_idx (ConvArgs::pool_idx of the forward launch that pooled).  `in` is then null.  Honoured by the two dgrad launches
    // that sit behind a pool: 64 <- 64 with the fused conv1 weight gradient (x1) and 128 <- 128 with mask_bits; their patch producers expand
    // the 2 x 2 windows while staging (a quarter of the gradient bytes + one code byte per pooled element instead of the map)
    const bf16* in_pooled; const uint8_t* in_idx;
    const bf16* mask;             // optional ReLU mask source (same shape as out): out = mask>0 ? v : 0
    // the same mask as one 64-bit word per pixel [B][H][W] (bit c = mask[..][c] > 0, written by mk_conv1_fwd): what the
    // fused-conv1-wgrad dgrad reads instead of the map (16 x 16 tiles)
    const unsigned long long* mask_bits;
    // the 128-channel layout of the same idea: FOUR dwords per pixel [B][H][W][4], dword q = the sign bytes of channel groups
    // 8q.., 32+8q.., 64+8q.., 96+8q.. (a lane of the streaming kernels masks exactly those).  out_sign_bits: a 128-output-channel
    // forward launch writes them for its ReLU'd output; a masked 128 <- 128 dgrad given them as mask_bits runs on 32-row tiles
    unsigned long long* out_sign_bits;
    bf16* out; int B, H, W, CIN, COUT;
    // 64->64 dgrad of the second conv only: fuse the weight gradient of conv1 (x1 = fp32 network input [B][H][W]) into the
    // epilogue; `out` is then never written, w1_slab receives 640 partial sums per virtual workgroup (mk_conv1_wgrad_fused_reduce)
    const float* x1; float* w1_slab;
    unsigned* sched;              // streaming kernel: 2 zero-initialised counters owned by the calling stream (null: a process-wide pair)
    bf16* pool_out;               // optional: MaxPool2d(2,2) (floor) of the ReLU'd output, [B][H/2][W/2][COUT], written by the same launch
    // optional, with pool_out: one byte per pooled element = window position (0..3, row-major scan) of its FIRST maximum, 4 where
    // that maximum is <= 0 (nothing passes the ReLU): all the pool + ReLU backward needs of the full-resolution map
    uint8_t* pool_idx;
    int out_optional;             // the caller does not need `out`: a launch that pools in its epilogue may skip storing it
    // streaming kernels only: `out` (and `mask`, same shape) has out_cstride channels per pixel and this launch computes channels
    // out_coff .. out_coff + COUT of it (wk / bias already offset by the caller); 0 = a plain [..][COUT] map.  How mk_conv3x3 runs the
    // 256-channel convs of the BLSTM front-end: two passes of 128 output channels over the same patches.
    int out_cstride, out_coff;
    // the task slots that share the GPU (masr_set_concurrency; the training step sets it, as GemmArgs::lean): from three on the persistent
    // grid is capped below one workgroup per CU (conv_grid_limit in conv.hip states the rule), so that workgroups of the
    // other streams find CUs whose LDS no conv workgroup holds for the whole launch.  Never part of the result's bits: the kernels that take
    // tiles from the atomic counter do not care who computes a tile, and the two whose partition into partial sums IS part of the bits (the
    // weight gradient, the fused conv1 weight gradient) keep that partition as VIRTUAL workgroups -- a launched workgroup runs the ids r,
    // r + grid, ... one after the other, each with its own tile walk, slab row and zeroed accumulators.  0 = the grid of a launch that has
    // the GPU to itself.  Which family a launcher belongs to is said in two places of conv.hip that go together: the static walks size
    // their grid through conv_static_grid (which asks conv_grid_limit with counter_fed = false and spreads the ids evenly), every other
    // launcher asks conv_grid_limit with counter_fed = true.
    int shared;
};
int mk_conv3x3(const ConvArgs& a, hipStream_t s);
long mk_conv1_wgrad_fused_slab_floats(int B, int H, int W);
int mk_conv1_wgrad_fused_reduce(float* slab, int B, int H, int W, float* dw, float* db, hipStream_t s);
// wgrad: dw[co][ci][3][3] (+ db[co]) from in (NHWC, CIN) and dy (NHWC, COUT)
struct ConvWgradArgs {
    const bf16* in; const bf16* dy; float* dw; float* db; float* slab; int B, H, W, CIN, COUT;
    // optional: dy = the 2x2 max-pool (+ ReLU) backward of dy_pooled [B][H/2][W/2][COUT] under the codes of ConvArgs::pool_idx -- the kernel
    // expands it while staging (a quarter of the gradient bytes + one code byte per pooled element instead of the full-resolution map)
    const bf16* dy_pooled; const uint8_t* pool_idx;
    int shared;                   // as ConvArgs::shared
};
// test hook (masr_test_set_conv_grid_cap): n > 0 caps every persistent conv grid at n workgroups whatever `shared` says; 0 = the normal rule
void mk_conv_force_grid_cap(int n);
int mk_conv3x3_wgrad(const ConvWgradArgs& a, hipStream_t s, int phase = 0);     // phase 1 / 2: the partial-slab kernel / the slab reduce alone
long mk_conv3x3_wgrad_slab_floats(int B, int H, int W, int CIN, int COUT);
int mk_maxpool_fwd(const bf16* in, bf16* out, int B, int H, int W, int C, hipStream_t s, int ceil_mode = 0);
// din = (in is the first max of its window && in > 0) ? dout : 0   (ReLU backward fused)
int mk_maxpool_relu_bwd(const bf16* in, const bf16* dout, bf16* din, int B, int H, int W, int C, hipStream_t s, int ceil_mode = 0);
// ConvArgs::pool_idx computed from a stored map (for the conv kernels that cannot emit the codes in their epilogue)
int mk_maxpool_idx(const bf16* in, uint8_t* idx, int B, int H, int W, int C, hipStream_t s);
// CIN = 1 convs with COUT = 64 n channels
int mk_conv1_fwd_n(const float* x, const float* w, const float* bias, bf16* out, int B, int H, int W, int COUT, hipStream_t s);
int mk_conv1_wgrad_n(const float* x, const bf16* dy, float* dw, float* db, float* slab, int B, int H, int W, int COUT, hipStream_t s);

// ---------------------------------------------------------------- attention (attention.hip)
struct AttnArgs {
    const bf16 *q, *k, *v; long ldq, ldk, ldv;   // row (b*T + t), head h at column h*hd
    bf16* o; long ldo; float* lse;               // lse [B][H][Tq]
    const bf16 *dout; long lddo;                 // backward
    bf16 *dq, *dk, *dv; long lddq, lddk, lddv;
    float* delta;                                // [B][H][Tq] scratch: rowsum(dO*O)
    const int* klens;                            // [B] valid keys per batch or null (all Tk)
    int B, H, Tq, Tk, hd, causal;
    float drop_p; uint32_t seed, site;
    const uint32_t* seed_ptr;                    // non-null: the seed is read from device memory (graph-replayed steps)
    // chunk mask (include/masr.h masr_chunk_policy; needs Tq == Tk and causal == 0): query i sees key j iff j < (i / c + 1) c and
    // (left < 0 or j >= (i / c - left) c).  chunk = 0 and chunk_ptr = null: no mask, the kernels without it.  A chunk read as 0 from
    // chunk_ptr is full context inside the masked kernels (a dynamic policy's step that drew none).
    int chunk, left;
    const int* chunk_ptr;                        // non-null: the chunk is read from device memory (graph-replayed steps)
};
int mk_attn_fwd(const AttnArgs& a, hipStream_t s);
int mk_attn_bwd(const AttnArgs& a, hipStream_t s);

// ---------------------------------------------------------------- streaming first pass (stream.hip)
// One chunk step of an encoder layer's self-attention: R new rows per utterance (row b*R + i of q / knew / vnew / o, head h at column h*hd)
// against the layer's cache.  Every row attends the keys [lo, min(pos + R, klens[b])): cache rows in front of pos, the step's own rows from
// pos on (read from knew / vnew).  The same launch appends the new rows to the cache at [pos, pos + R).  A row without a key: o = 0.
struct AttnStreamArgs {
    const bf16* q; long ldq;
    const bf16 *knew, *vnew; long ldnew;
    bf16 *kc, *vc; long ldc, batch_stride;     // cache row j of utterance b: kc + b*batch_stride + j*ldc + h*hd
    const int* klens;                          // [B] valid keys per utterance (device) or null (pos + R)
    bf16* o; long ldo;
    int B, H, hd, R, pos, lo, cap;             // cap: rows of the cache per utterance
};
int mk_attn_stream(const AttnStreamArgs& a, hipStream_t s);
// Greedy (best-path) CTC over the step's R logit rows of every utterance (row (b, i) at logits + b*batch_stride + i*ld, absolute frame pos + i):
// arg-max over the C valid columns, ties to the lower index; a frame < klens[b] whose arg-max is neither blank (0) nor the previous frame's
// appends (token, frame) at tokens / frames [b][len].  state [2][B] = previous arg-max | len, carried across steps (start: all 0)
struct CtcGreedyStreamArgs {
    const float* logits; long ld, batch_stride;
    const int* klens;                          // [B] or null (every frame of the step counts)
    int B, R, C, pos;
    int* state; int *tokens, *frames; int ld_out;
};
int mk_ctc_greedy_stream(const CtcGreedyStreamArgs& a, hipStream_t s);
// win [B][W][D] = rows w0 .. w0 + W of xbuf [B][cap_frames][D], zero at and behind lens[b]
int mk_stream_window(const float* xbuf, const int* lens, float* win, int B, int W, int D, int w0, long cap_frames, hipStream_t s);
// x32 / x16 [B*R][E] = rows off .. off + R of each utterance of v [B*Wp][E] + pe[s0 + i] (fp32 add, then the bf16 rounding)
int mk_stream_centre_pe(const float* v, const float* pe, float* x32, bf16* x16, int B, int R, int E, int Wp, int off, int s0, hipStream_t s);

// ---------------------------------------------------------------- incremental greedy decode (decode.hip)
// C[m][n] = epi(sum_k A[m][k] W[n][k]) for a handful of rows (one per utterance): bias, ReLU, fp32 residual
struct SkinnyArgs {
    const bf16* A; long lda; const bf16* W; long ldw; int M, N, K;
    const float* bias; int relu; const float* residual; long ldres;
    float* C32; long ldc; bf16* C16; long ldc16;
};
int mk_skinny_gemm(const SkinnyArgs& g, hipStream_t s);
// one query row per (utterance, head) against cached keys/values; see decode.hip
struct AttnDecodeArgs {
    const bf16* q; long ldq;                   // [B][ldq], head h at column h*hd
    const bf16 *k, *v; long ldk, kv_batch_stride;   // cache rows: k + b*kv_batch_stride + j*ldk + h*hd
    const bf16 *knew, *vnew; long ldnew;       // self-attention: newest row (appended to the cache at slot *step-1) or null
    const int* step;                           // device scalar: number of valid keys (self-attention) or null
    const int* klens;                          // [B] valid keys (cross-attention) when step == null
    bf16* o; long ldo;
    int B, H, hd, Tk_cap;                      // Tk_cap bounds the key count (sizes the LDS score row)
    // beam search (beam.hip).  rows_per_utt > 1: query row b reads the cross-attention cache / klens of utterance b / rows_per_utt.
    // src != null (self-attention): cached key/value j of row b lives in cache row src[(klen & 1) * src_flip + b * ld_src + j]
    // (the slot table of the step, double-buffered by step parity); the newest row is still appended to b's own cache row.
    // Greedy passes 0 / null: same loads, same arithmetic.
    int rows_per_utt;
    const int* src; long ld_src, src_flip;
};
int mk_attn_decode(const AttnDecodeArgs& a, hipStream_t s);
int mk_recog_embed_step(const int* step, const int* out, const float* table, const float* pe, float* y32, bf16* y16, int B, int E, int sos,
                        hipStream_t s);
// also advances step[0] once all B rows are done (ticket counter in step[1])
int mk_recog_argmax_step(int* step, const float* logits, long ld, int* out, int B, int C, hipStream_t s);
int mk_recog_step_set(int* step, int value, int inc, hipStream_t s);     // inc ? *step += 1 : *step = value
// logits[r][c] = bias[c] + <y32[r], W32[c]> in fp32 on the master weights (the decode's last projection: an arg-max follows)
int mk_logits_f32(const float* y32, const float* W32, const float* bias, float* logits, long ld, int rows, int C, int E, hipStream_t s);

// ---------------------------------------------------------------- beam search (beam.hip)
// device state of one beam decode: R = B*K hypothesis rows (row r = rank r % K of utterance r / K), Lmax steps at most
struct BeamArgs {
    int* step;                                 // [2]: current step t (1-based), ticket counter
    int B, K, R, Lmax, C, sos, eos;
    const int *maxlen, *minlen;                // [B] per utterance
    int* tab;                                  // [2][R][Lmax] self-attention slot tables (step parity)
    int *tok_hist, *par_hist;                  // [Lmax][R]: token / parent row of the running hypothesis in row r after step t
    float* score;                              // [R] running scores (-inf = dead row)
    int* list_tok; float* list_score;          // [R][K] each row's K best extensions of the step
    int* fin;                                  // [B] utterance finished
    float* best_score; int *best_len, *best_row;   // [B] best ended hypothesis: score, token count, row at step best_len
    // joint CTC/attention decode (masr_recog_beam_ctc; P = 0 and null otherwise).  list_tok / list_score are then [R][P] and hold each
    // row's candidates sorted by joint score
    int P, Tp;                                 // pre-beam width floor(3K/2), frame stride of the CTC arrays
    float att_w, ctc_w;
    const int* enc_lens;                       // [B] CTC frames T_b
    const float* ctc_lp;                       // [B][C][Tp] fp32 log_softmax of the CTC head (frame-contiguous per class)
    float2* ctc_state;                         // [2][R][Tp][P] (r^n, r^b) of row r's candidate i at frame t, step parity
    float* psi;                                // [R] CTC prefix score of the row's hypothesis
    int* src;                                  // [R] its CTC state: parent row * P + candidate slot of the previous step
    int* pre_tok; float* pre_lp;               // [R][P] pre-beam: the P best tokens by logit, their attention log-probs
    int* list_slot; float* list_psi;           // [R][P] beside list_tok / list_score: the candidate's chain slot and prefix score
    // joint decode with an n-gram LM, a length bonus and an N-best list (masr_recog_beam_ctc_lm; N = 0 and null otherwise).  The
    // four weights live on the device, so that a cached step graph never holds a value of theirs
    const float* wts;                          // [4] att_w, ctc_w, lm_w, len_bonus (att_w / ctc_w above are not read); the biased beam: [5], bias_w last
    float* pre_lm;                             // [R][P] beside pre_tok / pre_lp: the weighted LM term fl(lm_w * lm(c | h))
    int N;                                     // entries of the N-best list, 1 <= N <= K
    float* nb_score; int *nb_len, *nb_row;     // [B][N] ended hypotheses, best first (best_* are not used): score, token count, row at step nb_len;
                                               // an empty slot holds -inf / -1 / the utterance's first row, and the empty slots are the last
};
// The LM of the row stage, if any (one at most): backoff n-gram tables (lm.h) or a row of LM logits per hypothesis row
// (the LSTM LM, nlm.h).  Either one needs the fp32 workspace `fused`, where a row's fused increments stand while it is ranked
struct LmDev;
struct BeamRowLm {
    const LmDev* ngram;                        // null: no n-gram LM
    const float* lm_logits; long ld_lm;        // [R][ld_lm], null: no LM logits; lm(c) = their log-softmax
    float* fused; long ldf;                    // [R][ldf]
    float lm_w;                                // the LM weight of the top-K; the pre-beam reads a.wts[2]
};
// One step: mk_beam_embed_step, the decoder layers (engine), mk_beam_rows, in the joint beams mk_beam_ctc_prefix, and mk_beam_select.  Each
// launcher picks its kernel by a.P (> 0: joint CTC/attention) and a.N (> 0: the joint LM beam with its N-best list):
//   mk_beam_rows        logits [R][ld] -> P == 0: list_tok / list_score [R][K], the row's K best classes by the increment f(c); P > 0:
//                       the pre-beam pre_tok / pre_lp (/ pre_lm) [R][P], the P best by f.  f(c) = lp(c), or with an LM
//                       fl(lp(c) + fl(lm_w * lm(c | h))).  LM logits with P > 0 are refused: no decode runs that
//   mk_beam_ctc_prefix  the prefix scores and the row sort of the pre-beam; N > 0: with the LM term and the length bonus, weights from a.wts
//   mk_beam_select      the K-way merge; P > 0: the joint bookkeeping; N > 0: the N-best list and its stop rule.  Also advances step[0] once
//                       all B utterances are done
//   mk_beam_backtrace   once after the last step: tokens [B][Lmax], lens / scores [B]; N > 0: tokens [B][N][Lmax], lens / scores [B][N]
int mk_beam_init(const BeamArgs& a, hipStream_t s);
int mk_beam_embed_step(const BeamArgs& a, const float* table, const float* pe, float* y32, bf16* y16, int E, hipStream_t s);
// Contextual phrase biasing of the step beams (bias null / pre_b null: the unbiased kernels, as they were).  With it
//   mk_beam_rows        advances each live row's automaton state and ranks by g(c) = fl(f(c) + fl(bias_w * dn(h, c))), f = lp without an LM;
//                       the pre-beam also writes pre_b, and pre_lm = +0 without an LM.  LM logits with a list are refused
//   mk_beam_ctc_prefix  adds pre_b as the sixth term of the score (the N-best beam only)
//   mk_beam_select      stops on the bound that allows bias_w more per further token: the attention beam's from bias->bias_w, the N-best
//                       beam's from a.wts[4] (mk_beam_set_bias_weight)
//   mk_beam_backtrace   also writes nbias = n_final of every returned hypothesis ([B], or [B][N] with -1 in an empty slot)
struct BiasDev;
struct BeamBias {
    const BiasDev* dev;
    int2* state;                               // [2][R] (node, credited tokens), step parity
    float* pre_b;                              // [R][P] beside pre_lm (joint beam)
    float bias_w;                              // the attention beam's weight; the joint beam reads a.wts[4]
};
int mk_beam_rows(const BeamArgs& a, const BeamRowLm& lm, const float* logits, long ld, hipStream_t s, const BeamBias* bias = nullptr);
int mk_beam_ctc_prefix(const BeamArgs& a, hipStream_t s, const float* pre_b = nullptr);
int mk_beam_select(const BeamArgs& a, hipStream_t s, const BeamBias* bias = nullptr);
int mk_beam_backtrace(const BeamArgs& a, int* tokens, int* lens, float* scores, hipStream_t s, const BiasDev* bias = nullptr, int* nbias = nullptr);
int mk_beam_set_bias_weight(const BeamArgs& a, float bias_w, hipStream_t s);      // a.wts[4] (five floats then), behind mk_beam_set_weights
// once per joint decode: logits [B*Tp][ld] of the CTC head -> a.ctc_lp; the empty hypothesis's CTC state (after mk_beam_init); the joint LM
// beam's four weights into a.wts (a plain launch in front of the step replays)
int mk_beam_ctc_logsoftmax(const BeamArgs& a, const float* logits, long ld, hipStream_t s);
int mk_beam_ctc_init(const BeamArgs& a, hipStream_t s);
int mk_beam_set_weights(const BeamArgs& a, float att_w, float ctc_w, float lm_w, float len_bonus, hipStream_t s);
// out [R][C] = lm(c | ctx row) for every class; ctx int32 [R][order - 1], oldest first, -1 in front of a shorter context
int mk_lm_score(const LmDev& lm, const int* ctx, int R, float* out, hipStream_t s);

// ---------------------------------------------------------------- CTC prefix beam search (ctc_beam.hip)
// logits: row of utterance b, frame t at logits + (b*Tp + t)*ld.  P = min(K, emittable classes).  The arrays below are carved from the work buffer.
struct CtcBeamArgs {
    const float* logits; long ld;
    const int* enc_lens;                       // [B] valid frames (clamped to [0, Tp] by the kernels)
    int B, Tp, C, K, P, blank, eos;            // eos -1 = none
    float *lse, *xb;                           // [B*Tp] log-sum-exp of the row, x_t(blank)
    int* s_cls; float* s_lp;                   // [B*Tp][P] the frame's token set S_t and its log-probs
    int* rec;                                  // [B*Tp][K] back-pointers: parent slot | (emitted class + 1) << 8, 0 in the high part = stay
};
int64_t mk_ctc_beam_work_bytes(int B, int Tp, int C, int K);
// tokens int32 [B][nbest][Tp] (-1 behind each list), lens int32 [B][nbest] (-1 = no entry), scores fp32 [B][nbest] (-inf = no entry)
int mk_ctc_beam_search(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos, void* work,
                       int64_t work_bytes, int* tokens, int* lens, float* scores, hipStream_t s);
// the same search with an n-gram LM and a per-token bonus in the ranking: scores = the fused finals, am [B][nbest] = the acoustic
// totals; blank 0 and eos C - 1 only
struct masr_lm;
int64_t mk_ctc_beam_lm_work_bytes(int B, int Tp, int C, int K);
int mk_ctc_beam_search_lm(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const masr_lm* lm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int* tokens, int* lens, float* scores,
                          float* am, hipStream_t s);
// the same search (lm null: the plain one) with contextual phrase biasing (bias.h): scores = fl(final + fl(bias_w * n_final)),
// nbias int32 [B][nbest] = n_final (-1 = no entry), am written with or without an LM; blank 0 and eos C - 1 only
struct masr_bias;
struct BiasDev;
int64_t mk_ctc_beam_bias_work_bytes(int B, int Tp, int C, int K);
int mk_ctc_beam_search_bias(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                            const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work, int64_t work_bytes,
                            int* tokens, int* lens, float* scores, float* am, int* nbias, hipStream_t s);
// the resumable form of the three searches above (include/masr.h masr_ctc_beam_run_* has the contract): a host-only run object
// over the caller's work buffer of mk_ctc_beam_run_work_bytes = mk_ctc_beam_work_bytes + the state block.  open checks, launches the initial
// state and returns null on a refusal; advance runs the frames [done, t_end) (two launches, none with nothing to do); result runs the tail on
// the beam as it stands and stores nothing into the state.  fn: the entry point named in a refusal
struct masr_ctc_beam_run;
int64_t mk_ctc_beam_run_work_bytes(int B, int Tp, int C, int K);
masr_ctc_beam_run* mk_ctc_beam_run_open(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int blank, int eos,
                                        const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work,
                                        int64_t work_bytes, hipStream_t s);
int mk_ctc_beam_run_advance(const char* fn, masr_ctc_beam_run* r, int t_end, hipStream_t s);
int mk_ctc_beam_run_result(const char* fn, const masr_ctc_beam_run* r, int nbest, int* tokens, int* lens, float* scores, float* am, int* nbias,
                           hipStream_t s);
void mk_ctc_beam_run_close(masr_ctc_beam_run* r);
// (nodes_out, n_out)[i] = bias_step((nodes_in, n_in)[i], tokens[i]) for count independent states (device arrays)
int mk_bias_step(const BiasDev& d, const int* nodes_in, const int* n_in, const int* tokens, int count, int* nodes_out, int* n_out, hipStream_t s);

// ---------------------------------------------------------------- CTC forced alignment (ctc_align.hip)
// the best alignment of each utterance's transcript (targets[tgt_off[b] .. + tgt_len[b]), device arrays as mk_ctc_loss takes them) to its
// frames: frames int32 [B][Tp] (token index, -1 = blank, -2 past enc_len), start / end int32 [B][maxL] (-1 behind tgt_len), score fp32 [B].
// trace false (the benchmark, through masr_test_ctc_align_no_trace): only score is written, for feasible utterances the rest is left as it was
int64_t mk_ctc_align_work_bytes(int B, int Tp, int maxL);
int mk_ctc_align(const float* logits, long ld, const int* enc_lens, const int* targets, const int* tgt_off, const int* tgt_len, int B, int Tp, int C,
                 int blank, int maxL, void* work, int64_t work_bytes, int* frames, int* start, int* end, float* score, hipStream_t s, bool trace = true);

// ---------------------------------------------------------------- attention rescoring of an N-best list (rescore.hip)
// tok [R][ld_tok], lens [R] (-1 = no entry; a live one is <= L - 1) -> the decoder's tok_in [R][L] = [sos, h.., eos ..] and gold [R][L] =
// [h.., eos, -1 ..]; an entry without a list: all eos / all -1
int mk_rescore_prepare(const int* tok, long ld_tok, const int* lens, int R, int L, int sos, int eos, int* tok_in, int* gold, hipStream_t s);
// att[r] = sum over l (ascending) of log_softmax(logits[r*L + l][0 .. C))[gold[r*L + l]] over the rows with gold >= 0, -inf where there is none;
// row_lp [R*L]: the terms (scratch, 0 where gold < 0)
int mk_rescore_score(const float* logits, long ld, const int* gold, int R, int L, int C, float* row_lp, float* att, hipStream_t s);
// per utterance: score = att_w att + ctc_w ctc (the ctc term is left out when ctc_w == 0), entries reordered by (filled first, score descending,
// input rank ascending): order[b][j] = input rank of output entry j; tokens rows, lens and ctc are copies, scores / att -inf and lens -1
// where lens_in < 0.  N <= 64; the outputs may not alias the inputs
int mk_rescore_select(const int* tok_in, long ld_tok, const int* lens_in, const float* ctc_in, const float* att_in, int B, int N, float att_w,
                      float ctc_w, int* tokens, int* lens, float* scores, float* att, float* ctc, int* order, hipStream_t s);

// ---------------------------------------------------------------- row ops (rowops.hip)
int mk_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y32, bf16* y16,
                       float* mean, float* rstd, int rows, int E, hipStream_t s);
// dx32 = LN backward; dx16 = bf16 copy (optionally dropout-masked with (seed,site) for the branch GEMMs)
int mk_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                       float* dx32, bf16* dx16, float drop_p, uint32_t seed, uint32_t site,
                       float* dgamma, float* dbeta, float* slab, int rows, int E, hipStream_t s, const uint32_t* seed_ptr = nullptr);
// LayerNorm whose input row (forward) / incoming gradient (backward) is NOT in memory: it is what the epilogue of a k-split GEMM would have
// written -- the sum of n fp32 partial products part[z][row][E] (z-th at part + z * stride) (+ bias) (x dropout at element index row * E + column,
// the GEMM's) + residual.  Forward: the sum is stored to sum_out (the backward pass normalises it again).  Few rows only (< 2048).
struct LnSumArgs { const float* part; long stride; int n; const float* bias; const float* residual; float drop_p; uint32_t seed, site; const uint32_t* seed_ptr; float* sum_out; };
int mk_layernorm_fwd_sum(const LnSumArgs& sm, const float* gamma, const float* beta, float* y32, bf16* y16, float* mean, float* rstd, int rows, int E,
                         hipStream_t s);
int mk_layernorm_bwd_sum(const LnSumArgs& sm, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx32, bf16* dx16,
                         float drop_p, uint32_t seed, uint32_t site, float* slab, int rows, int E, hipStream_t s, const uint32_t* seed_ptr = nullptr);
long mk_layernorm_bwd_slab_floats(int rows, int E);     // capacity for any row count <= rows
int mk_layernorm_bwd_blocks(int rows);                    // partial-sum blocks a launch over `rows` rows writes
// dgamma == null: only the per-block partials are written to `slab` (each LayerNorm its own region) and
// mk_layernorm_bwd_reduce_grouped folds all of them in one launch at the end of the backward pass
struct LnReduceDesc { const float* slab; float* dgamma; float* dbeta; int nblocks; };
constexpr int LN_GROUP_MAX = 64;
struct LnReduceGroup { int n; LnReduceDesc p[LN_GROUP_MAX]; };
int mk_layernorm_bwd_reduce_grouped(const LnReduceGroup& grp, int E, hipStream_t s);
// every fold pass that closes a transformer step's backward as ONE launch (fold.hip): conv[k] = slab reduce of a 3x3-conv weight gradient
// (mk_conv3x3_wgrad phase 2; nsplit = the partial slabs its phase 1 wrote), conv1 = the 640-sum rows of the fused conv1 weight gradient
// (nblocks rows: one per VIRTUAL workgroup of that launch -- a function of the shape, not of the launched grid), ln = mk_layernorm_bwd_reduce_grouped's list, unperm = mk_vgg2enc_grad_unpermute,
// embed = mk_embed_bwd.  A null output pointer (dw / dtable) leaves the job out.
struct FoldJobs {
    int nconv, E;
    struct { const float* slab; int nsplit; float* dw; float* db; int CIN, COUT; } conv[3];
    struct { const float* slab; int nblocks; float* dw; float* db; } conv1;
    struct { const float* g; float* dw; int E, C, Dp; } unperm;
    struct { const int* order; const int* start; const float* dy; float* dtable; int V, E, accumulate; float drop_p; uint32_t seed, site; const uint32_t* seed_ptr; } embed;
    LnReduceGroup ln;
};
int mk_backward_folds(const FoldJobs& j, hipStream_t s);
int mk_conv3x3_wgrad_nsplit(const ConvWgradArgs& a);                     // the partial slabs mk_conv3x3_wgrad's phase 1 writes for this launch (virtual workgroups: whatever grid runs them)
int mk_conv1_wgrad_fused_rows(int B, int H, int W);                      // the 640-sum rows the fused conv1 weight gradient writes
int mk_embed_fwd(const int* tok, const float* table, const float* pe, float* y32, bf16* y16,
                   int B, int L, int E, float drop_p, uint32_t seed, uint32_t site, hipStream_t s, const uint32_t* seed_ptr = nullptr);
// dtable[v] (+)= sum over rows with tok==v of dy[row]  (deterministic: one block per vocab row)
// order / start: the token positions sorted by token id (ascending position inside a token) and the V + 1 segment starts, from the host
int mk_embed_bwd(const int* order, const int* start, const float* dy, float* dtable, int V, int E, int accumulate,
                 float drop_p, uint32_t seed, uint32_t site, hipStream_t s, const uint32_t* seed_ptr = nullptr);
// greedy decode: build the next decoder input from the previous step's tokens; arg-max of every logits row
int mk_recog_build_tok(int* tok, const int* out, int B, int L, int sos, hipStream_t s);
int mk_recog_argmax(const float* logits, long ld, int* out, int B, int L, int C, hipStream_t s);
// out[i] = the keep-scale (0 or 1/(1-p)) every dropout site applies to element i of its tensor (parity tests)
int mk_dropout_mask(float* out, long n, float p, uint32_t seed, uint32_t site, hipStream_t s);
// y16 = bf16(x32 * dropout_mask)
int mk_cast_dropout(const float* x, bf16* y, long n, float drop_p, uint32_t seed, uint32_t site, hipStream_t s, const uint32_t* seed_ptr = nullptr);
// column sums of x[rows][cols] (cols % 8 == 0, ld >= cols); only the first out_cols are written
int mk_colsum(const bf16* x, long ld, float* out, float* slab, int rows, int cols, int out_cols, hipStream_t s);
long mk_colsum_slab_floats(int rows, int cols);
// label-smoothed CE: logits fp32 [rows][ld]; gold int [rows] (-1 ignored); writes dlogits bf16 [rows][ld]
// stats[0] = loss (already / n_total), stats[1] = n_correct, stats[2] = n_total
// grad_w: factor of the gradient alone (the joint CTC/attention objective's 1 - w; 1 = the plain CE, the same bits)
int mk_ls_ce(const float* logits, long ld, const int* gold, int rows, int C, float eps, float inv_ntotal,
               bf16* dlogits, float* row_loss, int* row_correct, float* stats, hipStream_t s, const float* inv_ntotal_ptr = nullptr,
               float grad_w = 1.f);

// ---------------------------------------------------------------- flat optimiser ops (optim.hip)
// PRECONDITION: x is 16-byte aligned -- the kernel reads float4 at every multiple of four floats, whatever the pointer.  Every caller passes
// an engine's flat gradient buffer, which masr_bind / masr_blstm_bind refuse unless it is 16-byte aligned.
int mk_sumsq(const float* x, long n, float* slab, float* out_norm, hipStream_t s);       // out_norm[0] = sqrt(sum x^2)
long mk_sumsq_slab_floats(long n);
// coef = clip(max_norm / (norm+1e-6), <=1) (NaN propagates like torch.clamp)
// norm == nullptr: plain SGD step without clipping
int mk_clip_sgd(float* p, const float* g, float* mom, long n, const float* norm, float max_norm, float lr,
                  float momentum, int nesterov, int first_step, hipStream_t s);     // NaN norm -> step skipped
// (nan_zero: a NaN norm zeroes g / leaves acc alone instead of spreading NaNs -- masr_set_drop_nan_grads)
int mk_clip_scale(float* g, long n, const float* norm, float max_norm, hipStream_t s, int nan_zero = 0);    // g *= coef
int mk_clip_axpy(float* acc, const float* g, long n, const float* norm, float max_norm, hipStream_t s, int nan_zero = 0); // acc += coef*g
int mk_scale(float* x, long n, float a, hipStream_t s);
// weight_decay: decoupled != 0 -> AdamW (p *= 1 - lr*wd first), else torch.optim.Adam's L2 term (g += wd*p); 0 = plain Adam
int mk_adam_guarded(float* p, const float* g, float* m, float* v, long n, float lr_a, int t_a, float lr_b, int t_b, float b1, float b2, float eps,
                    float weight_decay, int decoupled, const float* norm, int* flags, int slot, hipStream_t s);
int mk_adam_sum(float* p, const float* const* grads, int n_grads, float gscale, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                int t, hipStream_t s);
int mk_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int t, float weight_decay,
            int decoupled, hipStream_t s);
int mk_sum_n(float* out, const float* const* grads, int n_grads, float scale, long n, hipStream_t s);     // out = (g0 + g1 + ...) * scale, n_grads <= 8
int mk_radam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int t, float weight_decay, int variant, hipStream_t s);
int mk_axpy(float* y, const float* x, long n, float a, hipStream_t s);
int mk_cast_bf16(const float* x, bf16* y, long n, hipStream_t s);
int mk_transpose_cast_bf16(const float* x /*[R][C]*/, bf16* y /*[C][ldy]*/, int R, int C, long ldy, hipStream_t s);
// conv weight shadows: w [CO][CI][3][3] fp32 -> wk [CO][tap*CI+ci] (fwd) and wd [CI][tap'*CO+co] = w[co][ci][8-tap'] (dgrad)
int mk_conv_weight_shadows(const float* w, bf16* wk, bf16* wd, int CO, int CI, hipStream_t s);       // (BLSTM engine; the transformer uses mk_all_shadows)
// EVERY bf16 operand shadow of the model in ONE launch (masr_refresh after each parameter update), descriptor driven:
//   SH_LINEAR   weight [N][K] at P+src -> k16 [N][K] and its transpose t16 [K][ldt] (64x64 tiles); ptrs[2i] = k16, ptrs[2i+1] = t16
//   SH_CONV     w [CO=N][CI=K][3][3] -> wk [CO][tap*CI+ci] (forward) and wd [CI][tap'*CO+co] = w[co][ci][8-tap'] (dgrad)
//   SH_VGG2ENC  w [E=N][a0*a1] with reference feature index c*Dp+d (a0 = C, a1 = Dp) -> wk [E][d*C+c] (NHWC order) and wt = wk^T
//   SH_COPY32   N floats at P+src -> (float*)ptrs[2i]   (the cross-attention K/V biases gathered into one vector)
enum { SH_LINEAR = 0, SH_CONV = 1, SH_VGG2ENC = 2, SH_COPY32 = 3 };
struct ShadowDesc { long src; int type, N, K, ldt, tile_start, a0, a1; };
// the whole job list travels in the kernel-argument segment (uniform scalar loads; a descriptor table in global memory cost
// every workgroup a chain of dependent loads to find its job)
constexpr int SHADOW_JOBS_MAX = 56;
struct ShadowJobs { int n, blocks; ShadowDesc d[SHADOW_JOBS_MAX]; bf16* p[2 * SHADOW_JOBS_MAX]; };
int mk_shadow_blocks(const ShadowDesc& d);                          // workgroups this job needs (tile_start bookkeeping on the host)
int mk_all_shadows(const float* P, const ShadowJobs& jobs, hipStream_t s);
// inverse map for the weight gradient: g_nhwc [E][d*C+c] fp32 -> dw [E][c*Dp+d]
int mk_vgg2enc_grad_unpermute(const float* g_nhwc, float* dw, int E, int C, int Dp, hipStream_t s);

// ---------------------------------------------------------------- data (data.hip)
// ragged gather + zero pad: rows of feat [sum T_i][D] -> xs [B][Tmax][D]
int mk_gather_pad(const float* feat, const long* row_start, const int* lens, float* xs, int B, int Tmax, int D, hipStream_t s);
// SpecAugment of xs [B][T][D] into out (another buffer) with the raw frame lengths lens [B] (device); rows >= lens[b] of out are zero.
// p: include/masr.h masr_specaug_policy, vetted by the caller; seed / seed_ptr: the step's seed, as every dropout kernel takes it
struct masr_specaug_policy;
int mk_specaug(const float* xs, const int* lens, float* out, int B, int T, int D, const masr_specaug_policy& p, uint32_t seed,
               const uint32_t* seed_ptr, hipStream_t s);

// ---------------------------------------------------------------- bidirectional LSTM (lstm.hip) -- BLSTM-P encoder of the CTC config
// rows are batch-first (b*T + t); the gate axis is unit-major (u*4 + g, g in torch order i,f,g,o); index [2] = direction
struct LstmStepArgs {
    int B, T, H, KP;                  // KP = H rounded up to a multiple of 32 (zero-padded bf16 recurrent operands)
    const int* lens;                  // [B] valid frames per sequence (device)
    bf16* h16[2][2];                  // [B][KP] hidden state ping-pong
    const bf16* whh16[2];             // [4H][KP]  W_hh, rows unit-major
    const bf16* whhT16[2];            // [H][4H]   W_hh^T (columns unit-major)
    const float* gx[2];               // [B*T][4H] input contribution + biases
    float* act[2];                    // [B*T][4H] gate activations (saved for backward)
    float* c[2];                      // [B*T][H]  cell states
    float* cstate[2];                 // [B][H]    running cell state (forward) / dL/dc carry (backward)
    bf16* y16;                        // [B*T][2H] layer output (fwd | bwd halves), 0 at padded frames
    const float* dy;                  // [B*T][2H] gradient wrt y (backward)
    bf16* dz16[2];                    // [B*T][4H] gradient wrt the gate pre-activations (backward output)
};
int mk_lstm_fwd_steps(const LstmStepArgs& a, hipStream_t s);
int mk_lstm_bwd_steps(const LstmStepArgs& a, hipStream_t s);
// The same recurrences as ONE launch per layer and pass: workgroups that stay for the whole sequence, W_hh slices in registers, h_t / dz_t
// exchanged between them as self-flagging 8-byte granules (lstm_rec.hip).  `words`: mk_lstm_rec_words() 64-bit words of scratch (start of an
// allocation-aligned block); *err is set to 1 when a workgroup gave up waiting for its peers (never cleared by the kernels).
bool mk_lstm_rec_ok(int B, int H, int KP);
int64_t mk_lstm_rec_words(int B, int H);
int mk_lstm_fwd_rec(const LstmStepArgs& a, unsigned long long* words, int* err, hipStream_t s, int test_stall = 0);   // test_stall: fault injection of the time-out test -- workgroup 0 leaves without publishing
int mk_lstm_bwd_rec(const LstmStepArgs& a, unsigned long long* words, int* err, hipStream_t s);
// W_ih [4H][K], W_hh [4H][H], biases in torch order -> unit-major bf16 shadows (+ transposes for the dgrad GEMMs)
int mk_lstm_shadows(const float* wih, const float* whh, const float* bih, const float* bhh, int H, int K, int KP_in, int KP_h,
                    bf16* wih16, bf16* wihT16, bf16* whh16, bf16* whhT16, float* bias, int pc, int pd, hipStream_t s);
// (pc, pd) != 0: the input features are an NHWC conv map [pd][pc]; torch's weight columns are c*pd + d
int mk_lstm_unperm(const float* src, float* dst, float* dst2, int H, int K, int pc, int pd, hipStream_t s);   // unit-major rows -> torch rows
int mk_lstm_hprev(const bf16* y16, bf16* hp0, bf16* hp1, int B, int T, int H, int KP, hipStream_t s);
int mk_cast_rows_pad(const float* x, bf16* y, long rows, int C, int Cp, hipStream_t s);
int mk_tanh_fwd(const float* x, float* y32, bf16* y16, long n, hipStream_t s);
int mk_tanh_bwd(const float* dy, const float* y, bf16* dx16, long n, hipStream_t s);
int mk_mask_rows(float* x32, bf16* x16, const int* lens, int B, int T, int C, hipStream_t s);
// time sub-sampling between BLSTM-P layers (ys_pad[:, ::sub], src/modules/encoder.py:118-121): ys[b][t'] = y[b][t' * sub], C % 8 == 0;
// backward: dy[b][t] = t % sub == 0 ? dys[b][t / sub] : 0 (fp32, C % 4 == 0)
int mk_subsample_rows(const bf16* y, bf16* ys, int B, int Tin, int Tout, int sub, int C, hipStream_t s);
int mk_subsample_rows_bwd(const float* dys, float* dy, int B, int Tin, int Tout, int sub, int C, hipStream_t s);

// ---------------------------------------------------------------- features (fbank.hip)
// Kaldi-style log-mel filterbank: wav fp32 (PCM scale, utterances concatenated), wav_off [B+1], row_off [B] (first output
// row of each utterance), feat [sum T_b][n_mel]; T_b = 1 + (n_b - 400) / 160; grid covers max_frames frames per utterance
// with_pitch: rows have n_mel + 3 columns (the pitch dims are mk_pitch's) and an utterance has min(fbank, pitch) frames
int mk_fbank(const float* wav, const long* wav_off, const long* row_off, int B, int max_frames, int n_mel, float* feat, hipStream_t s, int with_pitch = 0);
// Kaldi pitch features (pitch.hip): columns n_mel .. n_mel+2 of the same rows
long mk_pitch_work_bytes(long total_samples, int B, int max_frames);
int mk_pitch(const float* wav, const long* wav_off, const long* row_off, long total_samples, long max_samples, int B, int max_frames, int n_mel, float* feat,
             void* work, long work_bytes, hipStream_t s);

// ---------------------------------------------------------------- CTC (ctc.hip)
// logits fp32 [T][B][C] (pre-softmax); targets concatenated int [sum tl]; per-sample offsets tgt_off [B]
// loss_out[0] = mean_b( nll_b / max(tl_b,1) ), zero_infinity; grad wrt logits [T][B][C]
int mk_ctc_loss(const float* logits, const int* targets, const int* tgt_off, const int* in_len, const int* tgt_len,
                  int T, int B, int C, int blank, float* nll /*[B]*/, float* loss_out, float* grad, float* work,
                  int maxS, hipStream_t s, int batch_first = 0);      // batch_first: logits / grad are [B][T][C]
int mk_ctc_status(const float* work, int T, int B, int maxS, hipStream_t s);     // > 0: (index + 1) of an utterance the CTC launch on `work` refused (bad lengths)
long mk_ctc_work_floats(int T, int B, int maxS);
// the transformer's joint CTC/attention objective (train.hip ctc_forward): logits fp32 [B][T][ld] of the CTC head over the encoder memory, blank 0.
// stats[0] (the decoder's CE, mk_ls_ce) becomes (1 - w) CE + w CTC; grad16 (null: forward only) = w * d CTC / d logits as bf16 [B][T][ld],
// pad columns C .. ld zero.  Lengths are vetted on the host by the caller (no mk_ctc_status on this path).
int mk_ctc_loss_joint(const float* logits, long ld, const int* targets, const int* tgt_off, const int* in_len, const int* tgt_len, int T, int B,
                      int C, float* nll /*[B]*/, bf16* grad16, float w, float* stats, float* work, int maxS, hipStream_t s);
