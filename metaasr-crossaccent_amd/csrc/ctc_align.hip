// CTC forced alignment: the single best alignment of a known transcript to the frames of a CTC output layer (masr_ctc_align, DESIGN 5.9;
// the Viterbi recursion over the S = 2L + 1 lattice of ctc.hip, with a max where that one has a log-add).
//
//   ctc_align_frames   one wave per valid frame row (b, t < enc_len): the row's maximum and log-sum (row_lse), and the compact emission row
//                      em[b][t][0 .. L] = u_t(blank), u_t(y_0), .. with u_t(c) = z_t(c) - max_t, so that the serial sweep reads L + 1
//                      contiguous floats per frame instead of gathering from a C-wide row
//   ctc_align_sweep    one workgroup per utterance, serial over its frames: vets the targets, runs the recursion with the v row
//                      double-buffered in LDS (one barrier per frame, states strided over the threads, the next frames' emissions
//                      requested ahead), parks one back-pointer byte per (t, s) -- in LDS where the lattice fits, else in the work buffer --,
//                      walks them back with one lane and writes frames / start / end with all threads
//
// The path is decided on u, not on log_softmax: the frame's normaliser is the same for every state, so it cannot move an arg-max, and
// without it v is built from fp32 additions and comparisons alone.  The normalisers enter the score only, summed in frame order.
#include <cmath>

#include "kernels.h"
#include "search.h"

namespace {

constexpr int AL_THREADS = 256, AL_MAXS = 2048, AL_PF = 4;
constexpr int AL_BP_LDS = 32768;                   // back-pointer bytes kept on chip: enc_len * S up to this

struct CtcAlignArgs {
    const float* logits; long ld;
    const int *enc_lens, *targets, *tgt_off, *tgt_len;
    int B, Tp, C, blank, maxL;
    float *em, *lsum;                              // [B*Tp][maxL + 1] emissions, [B*Tp] log sum exp(u_t)
    unsigned char* bp;                             // [B*Tp][2 maxL + 1] back-pointers of the lattices too large for LDS
};

__device__ __forceinline__ int clamp_len(int n, int Tp) { return n < 0 ? 0 : (n > Tp ? Tp : n); }
__device__ __forceinline__ bool token_ok(int tok, int C, int blank) { return tok >= 0 && tok < C && tok != blank; }

// grid ceil(B*Tp / 4), 256 threads: one wave per frame row b*Tp + t.  A target the sweep will refuse is not gathered (its slot gets 0).
__global__ __launch_bounds__(256) void ctc_align_frames_kernel(CtcAlignArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)a.B * a.Tp) return;
    const int b = (int)(row / a.Tp), t = (int)(row % a.Tp);
    const int L = a.tgt_len[b];
    if (t >= clamp_len(a.enc_lens[b], a.Tp) || L < 0 || L > a.maxL) return;
    const float* z = a.logits + row * a.ld;
    const RowLse l = row_lse(z, a.C, lane);
    float* em = a.em + row * (a.maxL + 1);
    const int* tg = a.targets + a.tgt_off[b];
    if (lane == 0) { a.lsum[row] = l.log_s; em[0] = z[a.blank] - l.mx; }
    for (int i = lane; i < L; i += 64) {
        const int tok = tg[i];
        em[1 + i] = token_ok(tok, a.C, a.blank) ? z[tok] - l.mx : 0.f;
    }
}

// The recursion over frames 0 .. n - 1 for the states s = tid + 256 k, k < NS, of this thread.  Frame f's emissions and normaliser ride in
// ring slot f % AL_PF, requested AL_PF - 1 frames before their use (they do not depend on the recursion).  Returns the frame-order sum of
// the normalisers; the last row is left in v[(n - 1) & 1].  lds_bp: the back-pointers go to bp_lds [t][S], else to bp_glb [t][Sp].
template <int NS>
__device__ __forceinline__ float align_sweep(const float* __restrict__ em, int E, const float* __restrict__ lsum, const int* __restrict__ tg, int n, int S,
                                             float (*v)[AL_MAXS], bool lds_bp, unsigned char* bp_lds, unsigned char* __restrict__ bp_glb, int Sp, int tid) {
    int idx[NS];                                   // emission slot of the state: 0 = blank, 1 + i = token i
    bool live[NS], skip[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid + AL_THREADS * k;
        live[k] = s < S;
        idx[k] = live[k] && (s & 1) ? (s >> 1) + 1 : 0;
        skip[k] = live[k] && (s & 1) && s >= 3 && tg[s >> 1] != tg[(s >> 1) - 1];
    }
    float ring[AL_PF][NS], ringl[AL_PF];
#pragma unroll
    for (int f = 0; f < AL_PF; ++f) {
        ringl[f] = f < n ? lsum[f] : 0.f;
#pragma unroll
        for (int k = 0; k < NS; ++k) ring[f][k] = f < n && live[k] ? em[(long)f * E + idx[k]] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid + AL_THREADS * k;
        if (live[k]) v[0][s] = s < 2 ? ring[0][k] : NEG_INF;
    }
    float acc = add_rn(0.f, ringl[0]);
    __syncthreads();
    for (int i = 1; i < n; i += AL_PF) {
#pragma unroll
        for (int j = 0; j < AL_PF; ++j) {
            const int t = i + j;
            if (t >= n) break;                                              // (uniform)
            const int tn = t + AL_PF - 1;                                   // slot j held frame t - 1: free now
            float e[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) e[k] = ring[(j + 1) % AL_PF][k];
            const float ls = ringl[(j + 1) % AL_PF];
            ringl[j] = tn < n ? lsum[tn] : 0.f;
#pragma unroll
            for (int k = 0; k < NS; ++k) ring[j][k] = tn < n && live[k] ? em[(long)tn * E + idx[k]] : 0.f;
            const float* prev = v[(t - 1) & 1];
            float* cur = v[t & 1];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int s = tid + AL_THREADS * k;
                if (!live[k]) continue;
                float m = prev[s];
                int d = 0;
                if (s >= 1) { const float c1 = prev[s - 1]; if (c1 > m) { m = c1; d = 1; } }
                if (skip[k]) { const float c2 = prev[s - 2]; if (c2 > m) { m = c2; d = 2; } }
                if (m == NEG_INF) d = 0;
                cur[s] = m == NEG_INF ? NEG_INF : add_rn(m, e[k]);
                if (lds_bp) bp_lds[t * S + s] = (unsigned char)d;
                else bp_glb[(long)t * Sp + s] = (unsigned char)d;
            }
            acc = add_rn(acc, ls);
            __syncthreads();
        }
    }
    return acc;
}

// grid B, 256 threads.  TRACE false (masr_test_ctc_align_no_trace, the benchmark's leg): the kernel ends behind the score, so the difference to
// the whole is what the back-trace and the start / end pass cost
template <bool TRACE>
__global__ __launch_bounds__(AL_THREADS) void ctc_align_sweep_kernel(CtcAlignArgs a, int* __restrict__ frames, int* __restrict__ start,
                                                                     int* __restrict__ end, float* __restrict__ score) {
    __shared__ float s_v[2][AL_MAXS];
    __shared__ unsigned char s_bp[AL_BP_LDS];
    const int tid = threadIdx.x, b = blockIdx.x, Tp = a.Tp, maxL = a.maxL;
    const int n = clamp_len(a.enc_lens[b], Tp), L = a.tgt_len[b];
    int* fr = frames + (long)b * Tp;
    int* st = start + (long)b * maxL;
    int* en = end + (long)b * maxL;
    // the targets are vetted here, on the device: a refused utterance reads no emission and no back-pointer
    int bad = L < 0 || L > maxL;
    const int* tg = a.targets + (bad ? 0 : a.tgt_off[b]);
    if (!bad) for (int i = tid; i < L; i += AL_THREADS) bad |= !token_ok(tg[i], a.C, a.blank);
    bad = __syncthreads_or(bad);
    const int S = bad ? 1 : 2 * L + 1, Sp = 2 * maxL + 1;
    float acc = 0.f, vfin = NEG_INF;
    int fin = 0;
    const bool lds_bp = (long)n * S <= AL_BP_LDS;
    unsigned char* bp_glb = a.bp + (long)b * Tp * Sp;
    if (!bad && n > 0) {
        const float* em = a.em + (long)b * Tp * (maxL + 1);
        const float* lsum = a.lsum + (long)b * Tp;
        if (S <= AL_THREADS) acc = align_sweep<1>(em, maxL + 1, lsum, tg, n, S, s_v, lds_bp, s_bp, bp_glb, Sp, tid);
        else acc = align_sweep<AL_MAXS / AL_THREADS>(em, maxL + 1, lsum, tg, n, S, s_v, lds_bp, s_bp, bp_glb, Sp, tid);
        const float* last = s_v[(n - 1) & 1];
        fin = S - 1; vfin = last[S - 1];
        if (L > 0 && last[S - 2] > vfin) { fin = S - 2; vfin = last[S - 2]; }
    } else if (!bad && L == 0) {
        vfin = 0.f;                                                         // no frames, no tokens: the empty path
    }
    if (bad || vfin == NEG_INF) {                                           // refused or infeasible (uniform)
        for (int t = tid; t < Tp; t += AL_THREADS) fr[t] = -2;
        for (int i = tid; i < maxL; i += AL_THREADS) { st[i] = -1; en[i] = -1; }
        if (tid == 0) score[b] = bad ? __int_as_float(0x7fc00000) : NEG_INF;
        return;
    }
    // the back-trace: a chain of n dependent reads, one lane.  Non-finite logits may have left any byte behind: the step is masked to
    // {0, 1, 2} and the state clamped, so every index stays inside the lattice
    if (tid == 0) score[b] = add_rn(vfin, -acc);
    if constexpr (!TRACE) return;
    if (tid == 0) {
        int s = fin;
        for (int t = n - 1; t >= 0; --t) {
            fr[t] = (s & 1) ? s >> 1 : -1;
            if (t > 0) {
                const int d = (lds_bp ? s_bp[t * S + s] : bp_glb[(long)t * Sp + s]) & 3;
                s = max(s - min(d, 2), 0);
            }
        }
    }
    __syncthreads();                                                        // (every thread has read its last row: s_v is free)
    int* s_st = reinterpret_cast<int*>(s_v[0]);
    int* s_en = reinterpret_cast<int*>(s_v[1]);
    for (int i = tid; i < L; i += AL_THREADS) { s_st[i] = -1; s_en[i] = -1; }
    __syncthreads();
    for (int t = tid; t < Tp; t += AL_THREADS) {
        if (t >= n) { fr[t] = -2; continue; }
        const int i = fr[t];
        if (i < 0 || i >= L) continue;
        if (t == 0 || fr[t - 1] != i) s_st[i] = t;
        if (t == n - 1 || fr[t + 1] != i) s_en[i] = t + 1;
    }
    __syncthreads();
    for (int i = tid; i < maxL; i += AL_THREADS) { st[i] = i < L ? s_st[i] : -1; en[i] = i < L ? s_en[i] : -1; }
}

long align256(long v) { return (v + 255) & ~255l; }

}  // namespace

int64_t mk_ctc_align_work_bytes(int B, int Tp, int maxL) {
    if (B < 1 || Tp < 1 || maxL < 0 || 2 * (long)maxL + 1 > AL_MAXS) {
        mk_set_error("mk_ctc_align_work_bytes", "need B >= 1, Tp >= 1, maxL >= 0 and 2 * maxL + 1 <= 2048");
        return -1;
    }
    const long rows = (long)B * Tp;
    return align256(4 * rows * (maxL + 1)) + align256(4 * rows) + align256(rows * (2 * maxL + 1));
}

int mk_ctc_align(const float* logits, long ld, const int* enc_lens, const int* targets, const int* tgt_off, const int* tgt_len, int B, int Tp, int C,
                 int blank, int maxL, void* work, int64_t work_bytes, int* frames, int* start, int* end, float* score, hipStream_t s, bool trace) {
    const char* fn = "mk_ctc_align";
    if (!logits || !enc_lens || !targets || !tgt_off || !tgt_len || !work || !frames || !start || !end || !score) { mk_set_error(fn, "null pointer"); return -1; }
    if (B < 1 || Tp < 1) { mk_set_error(fn, "need B >= 1 and Tp >= 1"); return -1; }
    if (C < 2 || C > 4096 || ld < C) { mk_set_error(fn, "need 2 <= C <= 4096 and ld >= C"); return -1; }
    if (blank < 0 || blank >= C) { mk_set_error(fn, "blank must be in [0, C)"); return -1; }
    if (maxL < 0 || 2 * (long)maxL + 1 > AL_MAXS) { mk_set_error(fn, "need maxL >= 0 and 2 * maxL + 1 <= 2048 (the lattice width)"); return -1; }
    if (work_bytes < mk_ctc_align_work_bytes(B, Tp, maxL) || ((uintptr_t)work & 3)) {
        mk_set_error(fn, "work buffer too small (masr_ctc_align_work_bytes(B, Tp, maxL)) or misaligned");
        return -1;
    }
    CtcAlignArgs a{};
    a.logits = logits; a.ld = ld; a.enc_lens = enc_lens; a.targets = targets; a.tgt_off = tgt_off; a.tgt_len = tgt_len;
    a.B = B; a.Tp = Tp; a.C = C; a.blank = blank; a.maxL = maxL;
    const long rows = (long)B * Tp;
    char* w = (char*)work;
    a.em = (float*)w; w += align256(4 * rows * (maxL + 1));
    a.lsum = (float*)w; w += align256(4 * rows);
    a.bp = (unsigned char*)w;
    hipLaunchKernelGGL(ctc_align_frames_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    if (trace) hipLaunchKernelGGL(ctc_align_sweep_kernel<true>, dim3(B), dim3(AL_THREADS), 0, s, a, frames, start, end, score);
    else hipLaunchKernelGGL(ctc_align_sweep_kernel<false>, dim3(B), dim3(AL_THREADS), 0, s, a, frames, start, end, score);
    return LAUNCH_OK();
}
