// Internal to the transformer engine (not installed): what engine.hip (model, parameters, arena plans, setters, stats), train.hip (the
// training step) and recog.hip (the decoders) share -- the model behind the opaque handle of include/masr.h, the activation plan of
// one batch, and the few helpers every launch sequence goes through.
#pragma once
#include <utility>
#include <vector>

#include "../../include/masr.h"
#include "kernels.h"
#include "host_util.h"

struct Lin { int64_t w, b; int N, K; bf16 *k16, *t16; };          // weight [N][K]; k16 = bf16 copy, t16 = bf16 [K][Npad]
struct Norm { int64_t w, b; };
struct Attn { Lin in, out; bf16 *q_k16, *q_t16; };             // q_*: cross-attention only -- the query third of in_proj on its own
struct EncL { Attn sa; Lin l1, l2; Norm n1, n2; };
struct DecL { Attn sa, ca; Lin l1, l2; Norm n1, n2, n3; };
struct Conv { int64_t w, b; int CO, CI; bf16 *k16, *d16; };
struct EncAct { float *s1, *x1_32, *s2, *m1, *r1, *m2, *r2, *lse; bf16 *qkv, *ao, *x1_16, *f; uint32_t site[4]; };
struct DecAct {
    float *s1, *y1_32, *s2, *y2_32, *s3, *m1, *r1, *m2, *r2, *m3, *r3, *lse_s, *lse_c;
    bf16 *qkv, *ao, *y1_16, *q, *kv, *co, *y2_16, *f; uint32_t site[6];      // kv: this layer's 2E columns of Acts::kv_all (row stride NK)
};
// per-decoder-layer bf16 gradient operands of the deferred (grouped) weight-gradient launch
struct DecGrad { bf16 *g3, *g2, *g1, *gf, *gq, *gqkv; };
struct EncGrad { bf16 *g2, *g1, *gf, *gqkv; };          // per-layer gradient operands of the encoder-row weight gradients (kept for the grouped launch)
struct Acts {
    int B, T, D, H2, W2, Tp, Dp, L, rows_e, rows_d;
    int *tok_in, *gold, *enc_lens, *step_dev;
    int *tok_order, *tok_start;             // decoder-input token positions sorted by token id + the C + 1 segment starts (embedding backward)
    uint32_t* meta;                                        // [8] behind enc_lens, same upload: [0] dropout seed of the step, [1] 1/n_total (float bits), [2] the step's chunk (masr_set_chunk; 0 = none)
    bf16* step_qkv;                                        // incremental decode: the newest position's q|k|v [B][3E]
    bf16 *a1, *p1, *a3, *p2;
    unsigned long long *a1_bits, *a3_bits;                           // ReLU mask of a1, one word per pixel (written by conv1's forward, read by conv2's fused dgrad)
    uint8_t *i1, *i2;                                  // ConvArgs::pool_idx of the two pools (a2 / a4 are only written by conv kernels that cannot emit them)
    std::vector<float*> x32; std::vector<bf16*> x16;        // encoder layer inputs/outputs [NE+1]
    std::vector<EncAct> enc;
    float *mf, *rf; bf16* mem16; bf16* kv_all;             // kv_all [rows_e][ND*2E]: K|V of every decoder layer's cross-attention
    std::vector<float*> y32; std::vector<bf16*> y16;        // decoder layer inputs/outputs [ND+1]
    std::vector<DecAct> dec;
    float *mdf, *rdf; bf16* yf16;
    float* logits; bf16* dlogits; float* row_loss; int* row_correct;
    uint32_t site_v2e, site_emb;
    // backward scratch
    float *ge_a, *ge_b, *gd_a, *gd_b, *dmem32, *v2e_g32;
    bf16 *ge16, *gao_e, *gao_d, *gkv_all, *dp2, *da3, *dp1;      // (d(a4), d(a2) exist only as pooled gradient + codes; d(a1) never)
    float *delta_e, *delta_d;
    std::vector<DecGrad> dgr;
    std::vector<EncGrad> egr;
    float* part;                                           // fp32 partial products of a k-split few-row GEMM, summed by the LayerNorm that follows ([<= 8][rows_d][E])
    float* slab; int64_t slab_floats;
    float *cw_slab[3], *c1_slab;                           // partial slabs of the conv weight gradients: each its own, all folded by ONE launch at the end of the pass
    float* ln_slab; int64_t ln_slab_floats;                // one region per LayerNorm backward (grouped reduce)
    // joint CTC/attention objective (masr_create_ctc; null otherwise): the head's fp32 logits [rows_e][Cp] over the encoder memory, w * their
    // CTC gradient as the bf16 operand of the head's backward [rows_e][Cp] (training only), per-utterance nll [B], the lattice's work buffer,
    // and the targets' offsets | lengths into `gold` [2][B] (behind tok_start, in the same upload)
    float *ctc_logits = nullptr, *ctc_nll = nullptr, *ctc_work = nullptr; bf16* ctc_d16 = nullptr; int* ctc_tgt = nullptr; int ctc_maxS = 0;
    // SpecAugment (masr_set_specaug; null otherwise): the raw frame lengths [B] at the end of the tok_in upload (enc_lens is ilens / 4), and the
    // augmented batch [B][T][D] that conv1's forward and conv1's weight gradient read instead of xs (training plans only)
    int* raw_lens = nullptr; float* xa = nullptr;
};

// The captured launch sequence of ONE decode step, replayed once per step (recog.hip run_steps).  key / key_ptr: what it was captured
// for (unused slots zero); done: recorded behind the last replay -- nothing of a graph may be in flight when it is destroyed.
struct DecodeGraph {
    hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; hipEvent_t done = nullptr;
    int key[6] = {0, 0, 0, 0, 0, 0}; const void* key_ptr[3] = {nullptr, nullptr, nullptr};
    void destroy() {
        if (done) { hipEventSynchronize(done); hipEventDestroy(done); }
        if (exec) hipGraphExecDestroy(exec);
        if (graph) hipGraphDestroy(graph);
    }
};
// the slots of masr_model::decode_graphs (the table there says which decoder takes which)
enum GraphSlot { G_GREEDY, G_BEAM, G_JOINT, G_LM, G_NLM, G_JOINT_LM, G_JOINT_NLM, G_BIAS, G_JOINT_BIAS, G_CTC_NLM, G_COUNT };

constexpr int KSPLIT_MAX = 8;                              // partial products of a k-split GEMM (Acts::part)
constexpr int MASR_PE_ROWS = 3000;                         // rows of the positional-encoding table (masr_bind)

struct masr_model {
    masr_config cfg;
    int E, H, hd, Fi, NE, ND, C, Cp, D, Dp, F;
    std::vector<PInfo> params; int64_t nparams = 0;
    Conv conv[4]; Lin v2e, ct; int64_t embed_w;
    std::vector<EncL> enc; Norm enc_norm; std::vector<DecL> dec; Norm dec_norm;
    float ctc_w = 0.f; Lin ctc{};                          // joint CTC/attention objective (masr_create_ctc): weight, head ctc.ctc_lo [odim][E] (0: no head)
    float *P = nullptr, *G = nullptr; const float* pe = nullptr;
    char* ws = nullptr; int64_t ws_bytes = 0, persist_bytes = 0;
    bf16 *v2e_k = nullptr;                    // permuted vgg2enc weight (NHWC feature order)
    // cross-attention K/V projections of ALL decoder layers as one operand: the encoder memory is projected once by one GEMM
    // with N = ND*2E (forward), its gradient comes back through one GEMM with K = ND*2E and the ND weight gradients are one
    // reduction-major GEMM with M = ND*2E (segmented output rows).  kv_k16 [ND*2E][E], kvT [E][ND*2E], kv_bias [ND*2E].
    bf16 *kv_k16 = nullptr, *kvT = nullptr; float* kv_bias = nullptr; int NK = 0;
    std::vector<ShadowJobs> shadows;                       // job list(s) of the operand-shadow refresh: one launch per <= SHADOW_JOBS_MAX jobs (hkust: one)
    float* stats = nullptr;                   // device [8]: loss, n_correct, n_total, grad_norm
    unsigned* conv_sched = nullptr;           // tile counters of the streaming conv kernel (this model's stream only)
    float* h_stats = nullptr;                 // pinned
    // ring of page-locked stats blocks owned by the handle, one event each (masr_stats_post / masr_stats_wait): a block is only
    // handed out again after its previous copy's event has completed, whatever became of the ticket
    static constexpr int RING = 64;
    float* h_ring = nullptr; hipEvent_t ring_ev[RING]; bool ring_used[RING]; int64_t ring_next = 0;
    int* h_stage = nullptr; int64_t stage_ints = 0; int stage_slot = 0; hipEvent_t stage_ev[4];
    uint64_t seed = 0x1234; uint64_t step = 0;
    masr_specaug_policy aug{}; bool aug_on = false;        // masr_set_specaug
    bool aug_ran = false;                                  // the last masr_run_batch left its augmented batch in acts.xa (masr_specaug_last)
    masr_chunk_policy chunk{0, -1, 0}; bool chunk_on = false;   // masr_set_chunk: the chunk mask of the encoder's self-attention
    int chunk_last = -1;                                   // the chunk the last encoder forward ran with (masr_chunk_last; 0 = full context, -1 = none yet)
    Acts acts; bool have_acts = false;
    LnReduceGroup lng; int64_t ln_slab_used = 0;           // LayerNorm dgamma/dbeta partials, folded by one grouped launch
    bool split_wgrad = false;                              // masr_set_split_wgrad_launches
    int slots = 1;                                         // masr_set_concurrency: task slots sharing the GPU
    int drop_nan_grads = 0;                                // masr_set_drop_nan_grads: masr_clip_grads / masr_clip_accumulate turn a NaN-norm gradient into zeros (opt-out of quirk Q5)
    bool ksplit = false;                                   // masr_set_ksplit: few-row long-reduction GEMMs k-split, partials summed by the LayerNorm behind them
    int64_t n_ksplit = 0;                                  // k-split GEMM launches of the last masr_run_batch (masr_step_counters out[3])
    WgradGroup wg, wge;                                    // decoder-row / encoder-row weight gradients collected for the grouped launch (lin_wgrad)
    // captured training / evaluation steps (masr_run_batch, opt-in): a batch shape that repeats is replayed as ONE graph launch
    // instead of ~150 kernel launches.  Measured: host enqueue 0.61 -> 0.11 ms per step, step time unchanged (the GPU, not the
    // launch path, bounds both the single-task and the 4-task mode: tools/host_launch_cost.py) -- hence off by default
    struct StepGraph { int B, T, L, train; const void *ws, *P, *xs; hipGraph_t g; hipGraphExec_t e; uint64_t used; };
    std::vector<StepGraph> step_graphs; int last_key[4] = {0, 0, 0, -1}; const void* last_xs = nullptr; uint64_t graph_clock = 0;
    int64_t n_direct = 0, n_captured = 0, n_replayed = 0;  // masr_step_counters
    bool step_graphs_on = false;                           // masr_set_step_graphs
    // cached step graphs of the decoders, one slot per decoder variant (recog.hip run_steps): alternating decoders do not evict one
    // another.  A call whose key equals the slot's replays its graph, any other captures anew.  A weight that is in no key is a device value
    // written in front of the replays.  The step beams' keys are written by recog.hip beam_graph_key alone; words 0-3 are B, T, K, Lmax and
    // pointers 0-1 are ws, P:
    //   slot           decoder                      word 4                          word 5             pointer 2
    //   G_BEAM         attention beam               0                               0                  null
    //   G_JOINT        joint                        bits of att_w                   bits of ctc_w      null
    //   G_LM           n-gram LM                    bits of lm_w                    LM serial          null
    //   G_NLM          LSTM LM                      bits of lm_w                    NLM serial         null
    //   G_JOINT_LM     joint + n-gram LM (N-best)   N                               LM serial          null
    //   G_JOINT_NLM    joint + LSTM LM (N-best)     N                               NLM serial         null
    //   G_BIAS         biased attention beam        bits of lm_w with an LM, else 0 LM serial, else 0  bias serial << 32 | bits of bias_w
    //   G_JOINT_BIAS   biased joint (N-best)        N                               LM serial, else 0  bias serial << 32
    // and the two that are no step beam's, keyed where they run:
    //   G_GREEDY       masr_recog                   words {B, T, Ldec, 0, 0, 0}, pointers {ws, P, out}
    //   G_CTC_NLM      CTC beam + LSTM LM, a frame  words {B, T/4, K, NLM serial, the offsets of enc_lens and of the head's logits in ws, in
    //                  (ctc_first_pass)             4-byte units}, pointers {ws, P, the search's work buffer}
    DecodeGraph decode_graphs[G_COUNT];
    // the streaming first pass (stream_engine.hip): the open stream's geometry and host bookkeeping; its buffers are the plan of
    // (B, max_frames, c) behind the persistent region.  Every other call that plans the workspace closes it (stream_close)
    struct Stream {
        bool open = false, last = false;
        int B = 0, max_frames = 0, c = 0, left = -1;
        int recv = 0, emitted = 0;                         // input frames buffered, encoder frames emitted
        std::vector<int> len; std::vector<char> ended;     // per utterance: valid frames received, ended
        masr_ctc_beam_run* beam = nullptr;                 // the resumable prefix beam that follows the chunks, if one is open
    } stream;
    struct { float* logits; int* gold; int R, L; } last_rescore{};   // where the last rescoring call's decoder pass left its logits / gold (masr_test_rescore_logits)
    // profiling
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[MASR_PROF_N]; int prof_used[MASR_PROF_N] = {0};
};

// ------------------------------------------------------------------ profiling scope
struct Prof {
    masr_model* m; int cat; hipStream_t s; bool on;
    Prof(masr_model* m_, int cat_, hipStream_t s_) : m(m_), cat(cat_), s(s_), on(m_->prof) {
        if (!on) return;
        auto& v = m->prof_ev[cat];
        if (m->prof_used[cat] == (int)v.size()) {
            hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b); v.push_back({a, b});
        }
        hipEventRecord(v[m->prof_used[cat]].first, s);
    }
    ~Prof() {
        if (!on) return;
        hipEventRecord(m->prof_ev[cat][m->prof_used[cat]].second, s);
        m->prof_used[cat]++;
    }
};

// Y = X W^T (+bias ...) with the bf16 shadow of W
inline GemmArgs lin_fwd_args(const bf16* x, long ldx, const bf16* wk, int M, int N, int K, const float* bias) {
    GemmArgs g = gemm_args();
    g.A = x; g.lda = ldx; g.B = wk; g.ldb = K; g.M = M; g.N = N; g.K = K; g.bias = bias;
    return g;
}

// the 32-bit seed of one step: what every dropout mask and SpecAugment draw of the step is hashed from (masr_run_batch, masr_specaug)
inline uint32_t step_seed_of(uint64_t seed, uint64_t step) { return (uint32_t)(seed * 0x9E3779B97F4A7C15ull >> 32) + (uint32_t)step * 7919u; }
// host check of a policy against the batch geometry it will run on; null, or what is wrong (engine.hip)
const char* specaug_policy_error(const masr_specaug_policy& p, int D);
// the chunk a dynamic policy's training step runs with, from the step's 32-bit seed (include/masr.h masr_chunk_policy; 0 = full context).
// The hash of common.h (mix32, dropout_key, dropout_word) on the host: one word per step
inline uint32_t host_mix32(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
inline int chunk_draw_of(uint32_t step_seed, int Tp) {
    if (Tp < 2) return 0;
    const uint32_t key = host_mix32(step_seed * 0x9E3779B1u + 0x43484E4Bu * 0x85EBCA77u + 0x632BE5ABu), w = host_mix32(0u ^ key);
    const int r = 1 + (int)(((uint64_t)w * (uint64_t)(Tp - 1)) >> 32);
    return r > Tp / 2 ? 0 : r % 25 + 1;
}

// seed_ptr / inv_ptr: non-null while a step is being captured into a graph -- the dropout seed and 1/n_total of the step
// then live in device memory (Acts::meta, uploaded with the tokens), so one captured launch sequence serves every step
// chunk / left / chunk_ptr: the chunk mask of the encoder's self-attention in this pass (masr_set_chunk; 0: none).  Training passes get it from
// masr_run_batch -- chunk_ptr (Acts::meta + 2) under capture of a dynamic policy's step --, every other pass from forward_encoder itself.
struct Ctx {
    masr_model* m; hipStream_t s; uint32_t seed; bool train; float p_drop, p_pos; const uint32_t* seed_ptr = nullptr; const float* inv_ptr = nullptr;
    int chunk = 0, left = -1; const int* chunk_ptr = nullptr;
};

inline int gemm(Ctx& c, const GemmArgs& g) {
    const int re = c.m->acts.rows_e;
    const int cat = g.reduction_major ? (g.K == re ? MASR_PROF_WGRAD_ENC : MASR_PROF_WGRAD_DEC) : (g.M == re ? MASR_PROF_GEMM_ENC : MASR_PROF_GEMM_DEC);
    masr_model* m = c.m;
    Prof p(c.m, cat, c.s);
    GemmArgs h = g; h.seed_ptr = c.seed_ptr; h.lean = m->slots > 1;
    return mk_gemm(h, c.s);
}

inline int ln_fwd(Ctx& c, const Norm& n, const float* x, float* y32, bf16* y16, float* mean, float* rstd, int rows, const LnSumArgs* sum = nullptr) {
    masr_model* m = c.m;
    Prof p(m, MASR_PROF_LAYERNORM, c.s);
    // sum: x = the partial products of a k-split GEMM (train.hip gemm_or_ksplit), summed on the way in
    if (sum && sum->n > 0) return mk_layernorm_fwd_sum(*sum, m->P + n.w, m->P + n.b, y32, y16, mean, rstd, rows, m->E, c.s);
    return mk_layernorm_fwd(x, m->P + n.w, m->P + n.b, y32, y16, mean, rstd, rows, m->E, c.s);
}

// what every call that plans the workspace does to an open stream: its buffers are about to be overwritten
inline void stream_close(masr_model* m) {
    m->stream.open = false;
    mk_ctc_beam_run_close(m->stream.beam);                  // (host memory only; null is allowed)
    m->stream.beam = nullptr;
}

// engine.hip.  ctc: the branches of masr_run_batch alone, which the decoders do not plan -- the joint objective's (hybrid models) and
// SpecAugment's batch
void plan_acts(const masr_model* m, Arena& ar, Acts& a, int B, int T, int L, bool train, bool ctc = false);
// train.hip: the forward pass over m->acts (the decoders run the encoder, the K|V projection and, masr_recog_full, the decoder too)
int forward_encoder(Ctx& c, const float* xs);
int project_memory_kv(Ctx& c);
struct DecoderGeom { int seqs, L; };                       // forward_decoder on other than the plan's a.B x a.L rows (the rescoring pass)
int forward_decoder(Ctx& c, bool project_kv = true, bool logits_f32 = false, const DecoderGeom* gm = nullptr);
