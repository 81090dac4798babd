// Row-search primitives of the decoders: beam.hip, ctc_beam.hip, decode.hip and the arg-max kernels of rowops.hip.  Device helpers only;
// a wave is one row unless a helper says otherwise.  What differs between the call sites is an argument here, never a second copy.
#pragma once
#include "common.h"

constexpr float NEG_INF = -__builtin_inff();

__device__ __forceinline__ uint32_t ord_f32(float v) {             // monotone float -> uint32 (larger float, larger key)
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = ((unsigned long long)(uint32_t)__shfl_xor((int)(v >> 32), o, 64) << 32) |
                                     (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ float log_add(float a, float b) {      // log(e^a + e^b); -inf + -inf = -inf, never NaN
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(1.f + __expf(fminf(a, b) - m));
}

// fl(a * b) and fl(a + b) that no later pass fuses into a multiply-add: under the default -ffp-contract the plain operators (and __fmul_rn /
// __fadd_rn, which are the plain operators) were contracted in ctc_beam_sweep<true>, fma(lm_w, lm, len_bonus).  The LM-fused searches
// (ctc_beam.hip, the row stage and the joint LM beam of beam.hip) compose their scores from these two
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// Wave arg-max, ties to the lowest index (torch's first maximal index): every lane brings the (mx, am) of its own scan and leaves
// with the wave's.  The lanes' initial am is the caller's business: it is what a row with nothing above -inf returns.
__device__ __forceinline__ void wave_argmax_first(float& mx, int& am) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(mx, o, 64); const int oa = __shfl_xor(am, o, 64);
        if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
    }
}

// Log-sum-exp of the row z[0 .. C) in two parts, lse = mx + log_s: strided max, wave_max, strided sum of __expf(z - mx), wave_sum,
// __logf -- fp32 in that order.  The caller composes its log-prob, and the two compositions in use round differently:
//   (z - mx) - log_s    beam_rows, beam_ctc_logsoftmax (beam.hip)
//   z - (mx + log_s)    ctc_beam_frames, and ctc_beam_sweep through the stored lse (ctc_beam.hip)
// They may not be merged: the decoders' scores are pinned bit for bit to the written order, and the two kernels of ctc_beam.hip must
// agree with each other (a class scores the same whether it is read from the frame's token set or gathered as a prefix's last token).
struct RowLse { float mx, log_s; };
__device__ __forceinline__ RowLse row_lse(const float* z, int C, int lane) {
    float mx = NEG_INF;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += __expf(z[c] - mx);
    s = wave_sum(s);
    return {mx, __logf(s)};
}

// The N best classes of the row z[0 .. C), logit descending, class ascending: N rounds of "largest key below the previous one",
// key = (ordered logit, inverted class), unique per class.  skip(c): the class never enters.  Lane 0 runs emit(i, c) for position i; when
// the row runs out it gets c = -1, and the lanes share emit(k, -1) for the positions k behind it.
// CANON_ZERO orders -0 as +0 (ties between them go to the lower class); without it -0 sorts below +0.  Today ctc_beam_frames alone
// canonicalises, the kernels of beam.hip do not: changing either changes the tie order of the lists.
template <bool CANON_ZERO, class Skip, class Emit>
__device__ __forceinline__ void row_top_n(const float* z, int C, int N, int lane, Skip skip, Emit emit) {
    unsigned long long prev = ~0ull;
    for (int i = 0; i < N; ++i) {
        unsigned long long best = 0;
        for (int c = lane; c < C; c += 64) {
            if (skip(c)) continue;
            const unsigned long long key = ((unsigned long long)ord_f32(CANON_ZERO ? z[c] + 0.f : z[c]) << 32) | (uint32_t)(0x7fffffff - c);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        if (lane == 0) emit(i, best ? 0x7fffffff - (int)(uint32_t)best : -1);
        prev = best;
        if (best == 0) {
            for (int k = i + 1 + lane; k < N; k += 64) emit(k, -1);
            break;
        }
    }
}

// The step beams' histories, [step][stride]: token s >= 1 of the hypothesis that stands in row `row` after step s, and the row it stood in
// after step s - 1 (par_hist null: the row itself).  Rows of a finished utterance are not written any more, so an entry may be stale: the
// read is clamped -- a token outside [0, C) reads as `fallback`, a parent outside the K rows of the row's utterance as the row.  Every
// kernel that walks the histories reads them through this (beam_embed_step and the n-gram context of beam.hip, nlm_lstm_step of nlm.hip)
struct HistEntry { int tok, par; };
__device__ __forceinline__ HistEntry hist_entry(const int* tok_hist, const int* par_hist, long stride, int s, int row, int C, int K, int fallback) {
    const long o = (long)(s - 1) * stride + row;
    const int u0 = (row / K) * K;
    int tok = tok_hist[o], par = par_hist ? par_hist[o] : row;
    if (tok < 0 || tok >= C) tok = fallback;
    if (par < u0 || par >= u0 + K) par = row;
    return {tok, par};
}

// Step ticket of a per-step kernel whose n blocks each end their part of step st: the last one to arrive resets the ticket and advances
// the step (every block has read step[0] before taking its ticket).  One thread per block calls it.
__device__ __forceinline__ void step_ticket(int* step, int st, int n) {
    __threadfence();
    if (atomicAdd(step + 1, 1) == n - 1) { step[1] = 0; step[0] = st + 1; }
}
