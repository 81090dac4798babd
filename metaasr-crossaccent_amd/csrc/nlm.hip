// Shallow fusion of an LSTM language model into the attention beam (masr_recog_beam_nlm): the host builder of the device
// weights (masr_nlm_create), the per-step kernels, and the teacher-forced score operator (masr_nlm_score).
//
// The LM is Embedding -> L LSTM layers -> Linear.  Unlike the n-gram tables of lm.hip it has state: every hypothesis row carries (h, c) per
// layer, and a row of step st continues the state of its PARENT row of step st - 1.  The states are double-buffered by step parity (the
// slot-table idea of beam_embed_step): row r reads its parent's state at parity (st - 1) & 1 and writes its own at st & 1, so no copy pass
// follows the beam's re-parenting and nothing that is still being read gets overwritten.
//
// Per step (st read from the device scalar, so the launches are parameter-identical for every step and replay as one hipGraph):
//   nlm_lstm_step   one launch per layer: gates = [x | h_par] [W_ih | W_hh]^T + b on MFMA, the cell in the epilogue
//   skinny_gemm     the output projection of the top layer's new h -> fp32 LM logits [R][ld]   (decode.hip, no new kernel)
//   beam_rows       the beams' row stage (beam.hip) with the LM term = log_softmax of that row
#include <cmath>
#include <cstring>
#include <atomic>
#include <string>
#include <vector>

#include "kernels.h"
#include "search.h"
#include "host_util.h"
#include "nlm.h"
#include "../../include/masr.h"

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// token and parent row of row r at step st (search.h hist_entry: clamped); an id outside the LM's classes reads as 0
__device__ __forceinline__ HistEntry nlm_row_source(const NlmStepArgs& a, const NlmDev& lm, int r, int st) {
    if (st <= 1) return {lm.start_id, r};
    return hist_entry(a.tok_hist, a.par_hist, a.hist_stride, st - 1, r, lm.C, a.K, 0);
}

// the carry form's row (nlm.h mk_nlm_step_carry): token (-1: a stay), parent row, live.  Vetted: a token outside [1, C - 2] is a stay, a parent
// outside the K rows of the row's utterance is the row
struct CarrySrc { int tok, par; bool live; };
__device__ __forceinline__ CarrySrc nlm_carry_source(const NlmStepArgs& a, const NlmDev& lm, int r, int st) {
    const int u = r / a.K, u0 = u * a.K;
    const bool live = r - u0 < a.live[(st & 1) * (a.R / a.K) + u];
    if (st <= 1) return {lm.start_id, r, live};
    int tok = a.tok_hist[r], par = a.par_hist[r];
    if (tok < 1 || tok > lm.C - 2) tok = -1;
    if (par < u0 || par >= u0 + a.K) par = r;
    return {tok, par, live};
}

// Layer l of one step.  grid (Hp / 16, ceil(R / 16)), 256 threads: a workgroup owns 16 rows x 16 hidden units x the four gates, its four
// waves split the reduction over INp + Hp (k = wave * 32 + 128 i) as skinny_gemm_kernel does and combine through LDS.  Operands go global
// -> MFMA fragments directly (one 16-byte load per lane, operand and chunk): with <= 16 rows per tile there is no reuse to stage.  The A
// row is embed[tok] (layer 0: the gather is the row index) or layer l - 1's new h of the row for the first INp columns, and layer l's h of
// the PARENT row for the last Hp; a 32-wide chunk never straddles the two (INp % 32 == 0).  At st = 1 the state is zero: the recurrent half
// is skipped (it would add exact zeros) and c_par = 0.
// CARRY (mk_nlm_step_carry): a stay row copies its parent's (h, c), a dead row writes nothing, and a tile without a token row skips the
// reduction -- the same 16 rows stand in every wave, so the vote is uniform over the workgroup.  A token row's arithmetic is the other form's.
template <bool CARRY>
__global__ __launch_bounds__(256) void nlm_lstm_step_kernel(NlmDev lm, NlmStepArgs a, int l) {
    __shared__ float red[4][4][16][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
    const int st = *a.step, cur = st & 1, prv = cur ^ 1;
    const int Hp = lm.Hp, INp = l ? Hp : lm.Ep, KT = INp + Hp;
    const long LS = (long)a.R * Hp;                              // one layer's states
    int row = r0 + (lane & 15); if (row > a.R - 1) row = a.R - 1;
    int tok, par;
    bool work = true;
    if constexpr (CARRY) {
        const CarrySrc src = nlm_carry_source(a, lm, row, st);
        work = __ballot(src.live && src.tok >= 0) != 0;
        tok = src.tok < 0 ? 0 : src.tok; par = src.par;
    } else {
        const HistEntry src = nlm_row_source(a, lm, row, st);
        tok = src.tok; par = src.par;
    }
    const int ko = 8 * (lane >> 4);
    const bf16* __restrict__ x = (l ? a.hstate + ((long)cur * lm.L + (l - 1)) * LS + (long)row * Hp : lm.embed + (long)tok * lm.Ep) + ko;
    const bf16* __restrict__ hp = a.hstate + ((long)prv * lm.L + l) * LS + (long)par * Hp + ko;
    const bf16* __restrict__ wp = lm.w[l] + (long)(u0 + (lane & 15)) * KT + ko;
    const long GS = (long)Hp * KT;                               // one gate's rows
    const int kend = st == 1 ? INp : KT;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    int k = work ? wave * 32 : kend;
    for (; k + 128 < kend; k += 256) {                           // two chunks = ten independent loads in flight
        const bf16x8 a0 = ld8(k < INp ? x + k : hp + (k - INp)), a1 = ld8(k + 128 < INp ? x + k + 128 : hp + (k + 128 - INp));
        bf16x8 w0[4], w1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) { w0[g] = ld8(wp + g * GS + k); w1[g] = ld8(wp + g * GS + k + 128); }
#pragma unroll
        for (int g = 0; g < 4; ++g) { acc[g] = mma16(a0, w0[g], acc[g]); acc[g] = mma16(a1, w1[g], acc[g]); }
    }
    for (; k < kend; k += 128) {
        const bf16x8 a0 = ld8(k < INp ? x + k : hp + (k - INp));
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = mma16(a0, ld8(wp + g * GS + k), acc[g]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][g][4 * (lane >> 4) + r][lane & 15] = acc[g][r];
    __syncthreads();
    const int tm = threadIdx.x >> 4, tn = threadIdx.x & 15, m = r0 + tm, u = u0 + tn;
    if (m >= a.R) return;
    const long LO = ((long)cur * lm.L + l) * LS + (long)m * Hp + u;
    if constexpr (CARRY) {
        const CarrySrc sm = nlm_carry_source(a, lm, m, st);
        if (!sm.live) return;
        if (sm.tok < 0) {
            const long po = ((long)prv * lm.L + l) * LS + (long)sm.par * Hp + u;
            const bf16 h = a.hstate[po];
            a.cstate[LO] = a.cstate[po];
            a.hstate[LO] = h;
            if (l == lm.L - 1) a.htop[(long)m * Hp + u] = h;
            return;
        }
    }
    if (a.fin && a.fin[m / a.K]) return;
    if (a.score && a.score[m] == NEG_INF) return;               // dead row: its stale state is never a live row's parent
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) z[g] = ((red[0][g][tm][tn] + red[1][g][tm][tn]) + (red[2][g][tm][tn] + red[3][g][tm][tn])) + lm.b[l][g * Hp + u];
    const int mpar = CARRY ? nlm_carry_source(a, lm, m, st).par : nlm_row_source(a, lm, m, st).par;
    const float cp = st == 1 ? 0.f : a.cstate[((long)prv * lm.L + l) * LS + (long)mpar * Hp + u];
    const float ig = sigm(z[0]), fg = sigm(z[1]), gg = tanhf(z[2]), og = sigm(z[3]);      // torch gate order i, f, g, o
    const float cn = fg * cp + ig * gg;
    const bf16 h = (bf16)(og * tanhf(cn));
    a.cstate[LO] = cn;
    a.hstate[LO] = h;
    if (l == lm.L - 1) a.htop[(long)m * Hp + u] = h;
}

// grid ceil(R / 4), 256 threads: one wave per row
__global__ __launch_bounds__(256) void nlm_logp_kernel(const float* __restrict__ logits, long ld, int R, int C, float* __restrict__ out, long ldo) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* y = logits + (long)r * ld;
    const RowLse l = row_lse(y, C, lane);
    for (int c = lane; c < C; c += 64) out[(long)r * ldo + c] = (y[c] - l.mx) - l.log_s;
}

// the carry form's last launch, grid ceil(R / 4), 256 threads: one wave per row.  A token row's log-softmax goes to logp[st & 1][r], a stay
// row's is copied from its parent's row of the other parity, a dead row writes nothing; then the step advances
__global__ __launch_bounds__(256) void nlm_logp_carry_kernel(NlmDev lm, NlmStepArgs a, const float* __restrict__ logits, long ld, float* __restrict__ logp,
                                                            long ldp, int* step) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int st = *step;
    if (r < a.R) {
        const CarrySrc src = nlm_carry_source(a, lm, r, st);
        if (src.live) {
            float* out = logp + ((long)(st & 1) * a.R + r) * ldp;
            if (src.tok < 0) {
                const float* in = logp + ((long)((st & 1) ^ 1) * a.R + src.par) * ldp;
                for (int c = lane; c < lm.C; c += 64) out[c] = in[c];
            } else {
                const float* y = logits + (long)r * ld;
                const RowLse z = row_lse(y, lm.C, lane);
                for (int c = lane; c < lm.C; c += 64) out[c] = (y[c] - z.mx) - z.log_s;
            }
        }
    }
    __syncthreads();                                             // every wave of the block has read the step
    if (threadIdx.x == 0) step_ticket(step, st, gridDim.x);
}

// masr_nlm_score.  prepare, grid ceil(max(R * ld, R) / 256): hist[p][r] = tokens[r][p] (0 behind the row's length), out[r] = 0, step = 1
__global__ void nlm_score_prepare_kernel(const int* __restrict__ tokens, const int* __restrict__ lens, int R, int ld, int* __restrict__ hist,
                                         float* __restrict__ out, int* step) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { step[0] = 1; step[1] = 0; }
    if (i < R) out[i] = 0.f;
    if (i < (long)R * ld) {
        const int r = (int)(i % R), p = (int)(i / R);
        hist[i] = p < lens[r] ? tokens[(long)r * ld + p] : 0;
    }
}
// accumulate, grid ceil(R / 4), 256 threads: one wave per row.  Position i = st - 1 of row r has the target tokens[r][i] (i < len) or eos
// (i == len); out[r] = fl(out[r] + lm(target)), positions ascending
__global__ __launch_bounds__(256) void nlm_score_accum_kernel(const int* __restrict__ step, const float* __restrict__ logits, long ld,
                                                             const int* __restrict__ tokens, const int* __restrict__ lens, int R, int ldt, int C,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int i = *step - 1, len = lens[r];
    if (i > len) return;
    int t = i < len ? tokens[(long)r * ldt + i] : C - 1;
    if (t < 0 || t >= C) t = 0;
    const float* y = logits + (long)r * ld;
    const RowLse l = row_lse(y, C, lane);
    if (lane == 0) out[r] = out[r] + ((y[t] - l.mx) - l.log_s);
}

std::atomic<uint32_t> g_nlm_serial{1};

int pad32(int n) { return (n + 31) / 32 * 32; }
int64_t pad256(int64_t b) { return (b + 255) & ~(int64_t)255; }
uint16_t bf16_bits(float v) {                                    // round to nearest even (finite inputs)
    uint32_t u; memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
bool all_finite(const float* p, int64_t n) {
    for (int64_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
    return true;
}

}  // namespace

int mk_nlm_step(const NlmDev& lm, const NlmStepArgs& a, float* logits, long ld, hipStream_t s) {
    if (a.R < 1 || a.K < 1 || lm.L < 1 || lm.L > NLM_MAX_LAYERS || lm.Hp % 32 || lm.Ep % 32 || ld < lm.C || !a.hstate || !a.cstate || !a.htop || !a.step) {
        mk_set_error("mk_nlm_step", "need R, K >= 1, an LM of 1 .. 4 layers, ld >= C and the state buffers"); return -1;
    }
    for (int l = 0; l < lm.L; ++l) {
        hipLaunchKernelGGL(nlm_lstm_step_kernel<false>, dim3(lm.Hp / 16, (a.R + 15) / 16), dim3(256), 0, s, lm, a, l);
        if (LAUNCH_OK()) return -1;
    }
    SkinnyArgs g{};
    g.A = a.htop; g.lda = lm.Hp; g.W = lm.lo; g.ldw = lm.Hp; g.M = a.R; g.N = lm.C; g.K = lm.Hp; g.bias = lm.lo_b; g.C32 = logits; g.ldc = ld;
    return mk_skinny_gemm(g, s);
}
int mk_nlm_step_carry(const NlmDev& lm, const NlmStepArgs& a, float* logits, long ld, float* logp, long ldp, int* step, hipStream_t s) {
    if (a.R < 1 || a.K < 1 || a.R % a.K || lm.L < 1 || lm.L > NLM_MAX_LAYERS || lm.Hp % 32 || lm.Ep % 32 || ld < lm.C || ldp < lm.C || !a.hstate ||
        !a.cstate || !a.htop || !a.step || !a.live || !a.tok_hist || !a.par_hist || !logp || step != a.step) {
        mk_set_error("mk_nlm_step_carry", "need R a multiple of K >= 1, an LM of 1 .. 4 layers, ld, ldp >= C, the state buffers and the row records"); return -1;
    }
    for (int l = 0; l < lm.L; ++l) {
        hipLaunchKernelGGL(nlm_lstm_step_kernel<true>, dim3(lm.Hp / 16, (a.R + 15) / 16), dim3(256), 0, s, lm, a, l);
        if (LAUNCH_OK()) return -1;
    }
    SkinnyArgs g{};
    g.A = a.htop; g.lda = lm.Hp; g.W = lm.lo; g.ldw = lm.Hp; g.M = a.R; g.N = lm.C; g.K = lm.Hp; g.bias = lm.lo_b; g.C32 = logits; g.ldc = ld;
    CK(mk_skinny_gemm(g, s));
    hipLaunchKernelGGL(nlm_logp_carry_kernel, dim3((a.R + 3) / 4), dim3(256), 0, s, lm, a, logits, ld, logp, ldp, step);
    return LAUNCH_OK();
}
int mk_nlm_logp(const float* logits, long ld, int R, int C, float* out, long ldo, hipStream_t s) {
    hipLaunchKernelGGL(nlm_logp_kernel, dim3((R + 3) / 4), dim3(256), 0, s, logits, ld, R, C, out, ldo);
    return LAUNCH_OK();
}
extern "C" {

masr_nlm* masr_nlm_create(int C, int E, int H, int L, int start_id, const float* embed, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, const float* lo_w, const float* lo_b) {
    const char* fn = "masr_nlm_create";
    auto refuse = [&](const char* why) -> masr_nlm* { mk_set_error(fn, why); return nullptr; };
    if (C < 2 || C > 65535) return refuse("the number of classes must be in [2, 65535]");
    if (E < 1 || E > NLM_MAX_DIM || H < 1 || H > NLM_MAX_DIM) return refuse("E and H must be in [1, 2048]");
    if (L < 1 || L > NLM_MAX_LAYERS) return refuse("the number of layers must be in [1, 4]");
    if (start_id < 0 || start_id >= C) return refuse("start_id must be in [0, C - 1]");
    if (!embed || !w_ih || !w_hh || !b_ih || !b_hh || !lo_w || !lo_b) return refuse("null pointer");
    for (int l = 0; l < L; ++l) if (!w_ih[l] || !w_hh[l] || !b_ih[l] || !b_hh[l]) return refuse("null pointer");
    // every check runs on the host before anything is allocated on the device
    bool fin = all_finite(embed, (int64_t)C * E) && all_finite(lo_w, (int64_t)C * H) && all_finite(lo_b, C);
    for (int l = 0; l < L && fin; ++l)
        fin = all_finite(w_ih[l], (int64_t)4 * H * (l ? H : E)) && all_finite(w_hh[l], (int64_t)4 * H * H) && all_finite(b_ih[l], 4 * H) &&
              all_finite(b_hh[l], 4 * H);
    if (!fin) return refuse("a weight is not finite");

    const int Ep = pad32(E), Hp = pad32(H);
    // the device image: embed | per layer (w, b) | lo | lo_b, each rounded up to 256 bytes
    int64_t bytes = pad256((int64_t)C * Ep * 2);
    for (int l = 0; l < L; ++l) bytes += pad256((int64_t)4 * Hp * ((l ? Hp : Ep) + Hp) * 2) + pad256((int64_t)4 * Hp * 4);
    bytes += pad256((int64_t)C * Hp * 2) + pad256((int64_t)C * 4);
    std::vector<char> img((size_t)bytes, 0);                     // (zero: every pad)
    masr_nlm* lm = new masr_nlm();
    memset(&lm->dev, 0, sizeof lm->dev);
    lm->mem = nullptr; lm->bytes = bytes; lm->serial = g_nlm_serial.fetch_add(1);
    NlmDev& d = lm->dev;
    d.C = C; d.E = E; d.H = H; d.L = L; d.Ep = Ep; d.Hp = Hp; d.start_id = start_id;
    int64_t off = 0, off_embed, off_w[NLM_MAX_LAYERS], off_b[NLM_MAX_LAYERS], off_lo, off_lob;
    {
        off_embed = off;
        uint16_t* p = (uint16_t*)(img.data() + off);
        for (int c = 0; c < C; ++c) for (int e = 0; e < E; ++e) p[(int64_t)c * Ep + e] = bf16_bits(embed[(int64_t)c * E + e]);
        off += pad256((int64_t)C * Ep * 2);
    }
    for (int l = 0; l < L; ++l) {
        const int in = l ? H : E, INp = l ? Hp : Ep, KT = INp + Hp;
        off_w[l] = off;
        uint16_t* p = (uint16_t*)(img.data() + off);
        for (int g = 0; g < 4; ++g)
            for (int u = 0; u < H; ++u) {
                uint16_t* row = p + ((int64_t)g * Hp + u) * KT;
                const float* wi = w_ih[l] + ((int64_t)g * H + u) * in;
                const float* wh = w_hh[l] + ((int64_t)g * H + u) * H;
                for (int k = 0; k < in; ++k) row[k] = bf16_bits(wi[k]);
                for (int k = 0; k < H; ++k) row[INp + k] = bf16_bits(wh[k]);
            }
        off += pad256((int64_t)4 * Hp * KT * 2);
        off_b[l] = off;
        float* b = (float*)(img.data() + off);
        for (int g = 0; g < 4; ++g) for (int u = 0; u < H; ++u) b[g * Hp + u] = b_ih[l][g * H + u] + b_hh[l][g * H + u];
        off += pad256((int64_t)4 * Hp * 4);
    }
    {
        off_lo = off;
        uint16_t* p = (uint16_t*)(img.data() + off);
        for (int c = 0; c < C; ++c) for (int k = 0; k < H; ++k) p[(int64_t)c * Hp + k] = bf16_bits(lo_w[(int64_t)c * H + k]);
        off += pad256((int64_t)C * Hp * 2);
        off_lob = off;
        memcpy(img.data() + off, lo_b, sizeof(float) * (size_t)C);
    }
    hipError_t e = hipMalloc(&lm->mem, (size_t)bytes);
    if (e == hipSuccess) e = hipMemcpy(lm->mem, img.data(), (size_t)bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        mk_set_error(fn, hipGetErrorString(e));
        if (lm->mem) hipFree(lm->mem);
        delete lm;
        return nullptr;
    }
    const char* base = (const char*)lm->mem;
    d.embed = (const bf16*)(base + off_embed); d.lo = (const bf16*)(base + off_lo); d.lo_b = (const float*)(base + off_lob);
    for (int l = 0; l < L; ++l) { d.w[l] = (const bf16*)(base + off_w[l]); d.b[l] = (const float*)(base + off_b[l]); }
    return lm;
}

void masr_nlm_destroy(masr_nlm* lm) {
    if (!lm) return;
    hipDeviceSynchronize();                                       // no decode that reads the weights is still in flight
    if (lm->mem) hipFree(lm->mem);
    delete lm;
}

int64_t masr_nlm_bytes(const masr_nlm* lm) {
    if (!lm) { mk_set_error("masr_nlm_bytes", "null model"); return -1; }
    return lm->bytes;
}

// the work buffer of masr_nlm_score: step [2] | tokens by position [ld][R] | hstate | cstate | htop | logits [R][C padded to 128]
struct NlmScorePlan { int64_t step, hist, h, c, htop, logits, total; long ldl; };
static NlmScorePlan nlm_score_plan(const NlmDev& d, int R, int ld) {
    NlmScorePlan p{};
    p.ldl = (d.C + 127) / 128 * 128;
    int64_t off = 0;
    p.step = off; off += 256;
    p.hist = off; off += pad256((int64_t)std::max(ld, 1) * R * 4);
    p.h = off; off += pad256(nlm_state_elems(d, R) * 2);
    p.c = off; off += pad256(nlm_state_elems(d, R) * 4);
    p.htop = off; off += pad256((int64_t)R * d.Hp * 2);
    p.logits = off; off += pad256((int64_t)R * p.ldl * 4);
    p.total = off;
    return p;
}
static bool nlm_score_shape_ok(const masr_nlm* lm, int R, int ld) { return lm && R >= 1 && R <= (1 << 20) && ld >= 0 && ld <= 4096; }

int64_t masr_nlm_score_work_bytes(const masr_nlm* lm, int R, int ld) {
    if (!nlm_score_shape_ok(lm, R, ld)) { mk_set_error("masr_nlm_score_work_bytes", "need an LM, 1 <= R <= 2^20, 0 <= ld <= 4096"); return -1; }
    return nlm_score_plan(lm->dev, R, ld).total;
}

int masr_nlm_score(const masr_nlm* lm, const int32_t* tokens, const int32_t* lens, int R, int ld, float* logp_out, void* work, int64_t work_bytes,
                   void* stream) {
    const char* fn = "masr_nlm_score";
    auto fail = [&](const char* why) { mk_set_error(fn, why); return -1; };
    if (!lm) return fail("null language model");
    if (!nlm_score_shape_ok(lm, R, ld)) return fail("need 1 <= R <= 2^20, 0 <= ld <= 4096");
    if (!lens || !logp_out || !work || (ld > 0 && !tokens)) return fail("null pointer");
    if ((uintptr_t)work & 255) return fail("the work buffer must be 256-byte aligned");
    const NlmDev& d = lm->dev;
    const NlmScorePlan p = nlm_score_plan(d, R, ld);
    if (work_bytes < p.total) return fail("work buffer too small (masr_nlm_score_work_bytes(nlm, R, ld))");
    hipStream_t s = (hipStream_t)stream;
    // the one host synchronisation of the call: lengths and tokens come to the host and are vetted (a token indexes the embedding table)
    std::vector<int> h_lens((size_t)R), h_tok((size_t)R * ld);
    HIP_CHECK_RET(hipMemcpyAsync(h_lens.data(), lens, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
    if (ld) HIP_CHECK_RET(hipMemcpyAsync(h_tok.data(), tokens, sizeof(int) * h_tok.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    int mx = 0;
    for (int r = 0; r < R; ++r) {
        const int n = h_lens[r];
        if (n < 0 || n > ld) return fail("lens must lie in [0, ld]");
        for (int i = 0; i < n; ++i) if (h_tok[(size_t)r * ld + i] < 0 || h_tok[(size_t)r * ld + i] >= d.C) return fail("tokens must lie in [0, C - 1]");
        mx = std::max(mx, n);
    }
    char* w = (char*)work;
    int* step = (int*)(w + p.step); int* hist = (int*)(w + p.hist); float* logits = (float*)(w + p.logits);
    NlmStepArgs a{};
    a.step = step; a.R = R; a.K = 1; a.tok_hist = hist; a.par_hist = nullptr; a.hist_stride = R;
    a.hstate = (bf16*)(w + p.h); a.cstate = (float*)(w + p.c); a.htop = (bf16*)(w + p.htop);
    const long n = std::max((long)R * ld, (long)R);
    hipLaunchKernelGGL(nlm_score_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tokens, lens, R, ld, hist, logp_out, step);
    CK(LAUNCH_OK());
    for (int i = 0; i <= mx; ++i) {                              // position i: feed [start] + tokens[.. i), score the target at i
        CK(mk_nlm_step(d, a, logits, p.ldl, s));
        hipLaunchKernelGGL(nlm_score_accum_kernel, dim3((R + 3) / 4), dim3(256), 0, s, step, logits, p.ldl, tokens, lens, R, ld, d.C, logp_out);
        CK(LAUNCH_OK());
        CK(mk_recog_step_set(step, 0, 1, s));
    }
    return 0;
}

}  // extern "C"
