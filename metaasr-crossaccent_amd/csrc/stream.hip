// Kernels of the streaming first pass: the chunk step's self-attention against a per-layer K|V cache, the greedy CTC decode
// that carries its state across chunks, and the two copies around the windowed front-end.
//
// attn_stream_kernel.  A chunk step has R <= c query rows per (utterance, head), typically 16, and every row of the step attends the same key
// range [lo, min(pos + R, klen_b)): the keys in front of pos are cache rows, the keys [pos, pos + R) the step's own.  One workgroup = one
// (b, h, 16-row query tile) on four waves; the key range is cut into 64-key blocks from lo on, wave w takes the blocks w, w + 4, .. and
// keeps its own running (m, l, o); the four are merged once through LDS at the end (the flash-decoding shape: at 16 query rows the
// parallelism that is left lies along the keys).  The products are the transposed ones of attention.hip: S^T = K Q^T with the K rows read
// straight from global memory as the A operand (a key block is read by one wave, once: LDS would add a round trip and share nothing), so lane
// (i, g) holds keys 4g .. 4g + 3 of query i in each 16-key tile -- the B operand layout of O^T = V^T P^T, contraction over the keys in the
// order the transposing reads of the wave's V tile deliver.  P goes from one MFMA to the next through registers.
//   New keys are read from knew / vnew, never from the cache: the workgroup of query tile 0 copies its head's columns of the R new rows into
// the cache rows [pos, pos + R), which no workgroup of this launch reads.  Key rows outside [lo, kend) are never loaded (the row index is
// clamped into the range, the element masked), so nothing that was not written by a step reaches the arithmetic.
#include "common.h"
#include "kernels.h"
#include "search.h"

namespace {

constexpr int SBLK = 64;            // keys per block
constexpr int SNW = 4;              // waves per workgroup
constexpr float SNEG = -1e30f;
constexpr float SLOG2E = 1.44269504088896341f;

template <int HD> struct SCfg {
    static constexpr int HDP = HD < 32 ? 32 : HD;   // contraction length of q.k (zero padded)
    static constexpr int KS = HDP / 32;
    static constexpr int DT = HD / 16;
    static constexpr int LD = HDP + 16;             // row stride of the V tile (attention.hip's)
    static constexpr int CPR = HD / 8;              // 16-byte chunks per row
};

typedef __attribute__((address_space(3))) bf16x4 lds_b4;

// attention.hip's frag_tr: contraction over the tile's row index, rows krow0 .. krow0 + 31, columns c0 .. c0 + 15; element e of lane group g
// is row 4g + e (e < 4) | 16 + 4g + (e - 4).  EXEC must be all ones
template <int LD>
__device__ __forceinline__ bf16x8 sfrag_tr(const bf16* tile, int krow0, int c0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const bf16* a0 = tile + (krow0 + 4 * g + q) * LD + c0 + 4 * p;
    const bf16* a1 = a0 + 16 * LD;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)a0);
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)a1);
    bf16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
}
__device__ __forceinline__ bf16x8 sfrag_acc(const f32x4& t0, const f32x4& t1) {
    bf16x8 f;
    f[0] = (bf16)t0[0]; f[1] = (bf16)t0[1]; f[2] = (bf16)t0[2]; f[3] = (bf16)t0[3];
    f[4] = (bf16)t1[0]; f[5] = (bf16)t1[1]; f[6] = (bf16)t1[2]; f[7] = (bf16)t1[3];
    return f;
}
__device__ __forceinline__ float sfold_max(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float sfold_sum(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }

template <int HD>
__global__ __launch_bounds__(64 * SNW) void attn_stream_kernel(AttnStreamArgs a) {
    using C = SCfg<HD>;
    constexpr int LD = C::LD, KS = C::KS, DT = C::DT, CPR = C::CPR;
    __shared__ __attribute__((aligned(16))) bf16 sV[SNW][SBLK * LD];      // each wave's own V tile: no workgroup barrier inside the key loop
    __shared__ float sO[SNW][16][HD];
    __shared__ float sM[SNW][16], sL[SNW][16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 16;
    const int R = a.R, pos = a.pos, lo = a.lo;
    const int klen = a.klens ? a.klens[b] : pos + R;
    const int kend = min(pos + R, klen);                                  // the step's key range [lo, kend), the same for every row
    const float scale = rsqrtf((float)HD), sc2 = scale * SLOG2E;

    const bf16* qb = a.q + (long)b * R * a.ldq + h * HD;
    const bf16* knb = a.knew + (long)b * R * a.ldnew + h * HD;
    const bf16* vnb = a.vnew + (long)b * R * a.ldnew + h * HD;
    bf16* kcb = a.kc + (long)b * a.batch_stride + h * HD;
    bf16* vcb = a.vc + (long)b * a.batch_stride + h * HD;

    // the cache append: this head's columns of the R new rows (query tile 0 alone; rows no workgroup of this launch reads)
    if (blockIdx.x == 0) {
        for (int c = tid; c < R * CPR; c += 64 * SNW) {
            const int r = c / CPR, dc = (c % CPR) * 8;
            st8(kcb + (long)(pos + r) * a.ldc + dc, ld8(knb + (long)r * a.ldnew + dc));
            st8(vcb + (long)(pos + r) * a.ldc + dc, ld8(vnb + (long)r * a.ldnew + dc));
        }
    }

    const int gi = lane & 15, g = lane >> 4, g4 = g * 4;
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int r = q0 + gi, dcol = ks * 32 + g * 8;
        const bf16x8 v = ld8(qb + (long)(r < R ? r : R - 1) * a.ldq + (dcol < HD ? dcol : 0));
        qf[ks] = (r < R && dcol < HD) ? v : zero8();
    }
    float m = SNEG, l = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // a key row: the cache in front of pos, the step's own rows from pos on; j is inside [lo, kend)
    auto krow = [&](int j) -> const bf16* { return j >= pos ? knb + (long)(j - pos) * a.ldnew : kcb + (long)j * a.ldc; };
    auto vrow = [&](int j) -> const bf16* { return j >= pos ? vnb + (long)(j - pos) * a.ldnew : vcb + (long)j * a.ldc; };

    const int nkb = kend > lo ? (kend - lo + SBLK - 1) / SBLK : 0;
    bf16* myV = sV[wave];
    for (int kb = wave; kb < nkb; kb += SNW) {                            // (wave-uniform trip count: EXEC stays full for the transposing reads)
        const int k0 = lo + kb * SBLK;
        // V tile of the block: 64 rows x HD through registers into the wave's LDS image; rows at or behind kend are clamped (their p is 0)
        bf16x8 vr[CPR];
#pragma unroll
        for (int i = 0; i < CPR; ++i) {
            const int c = lane + i * 64, r = c / CPR, dc = (c % CPR) * 8;
            const int j = min(k0 + r, kend - 1);
            vr[i] = ld8(vrow(j) + dc);
        }
        f32x4 s[4];                                                       // S^T: keys jt*16 + 4g + r of query gi
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int j = min(k0 + jt * 16 + gi, kend - 1);
            const bf16* kr = krow(j);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int dcol = ks * 32 + g * 8;
                const bf16x8 kf = ld8(kr + (dcol < HD ? dcol : 0));
                s[jt] = mma16(dcol < HD ? kf : zero8(), qf[ks], s[jt]);
            }
        }
#pragma unroll
        for (int i = 0; i < CPR; ++i) {
            const int c = lane + i * 64, r = c / CPR, dc = (c % CPR) * 8;
            st8(myV + r * LD + dc, vr[i]);
        }
        const bool full = k0 + SBLK <= kend;
        float mx = SNEG;
        if (!full) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + jt * 16 + g4 + r >= kend) s[jt][r] = SNEG;
        }
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[jt][r]);
        const float mn = fmaxf(m, sfold_max(mx));
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sc2);
        m = mn;
        float rs = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f((s[jt][r] - m) * sc2);
                if (!full && s[jt][r] <= SNEG) p = 0.f;
                rs += p;
                s[jt][r] = p;
            }
        l = l * alpha + sfold_sum(rs);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        // the wave's LDS writes above are read by other lanes of the same wave: order them (LDS operations of one wave complete in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int m2 = 0; m2 < 2; ++m2) {
            const bf16x8 pf = sfrag_acc(s[2 * m2], s[2 * m2 + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mma16(sfrag_tr<LD>(myV, m2 * 32, dt * 16, lane), pf, o[dt]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // (the next block's tile writes stay behind these reads)
        __builtin_amdgcn_wave_barrier();
    }
    // merge: every wave leaves its (m, l, o^T); a wave without a block leaves (NEG, 0, 0), whose weight below is 0 beside a real maximum
    if (g == 0) { sM[wave][gi] = m; sL[wave][gi] = l; }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) sO[wave][gi][dt * 16 + g4 + r] = o[dt][r];
    __syncthreads();
    // 16 rows x HD / 4 column quads over the 256 threads; a row without a visible key (l == 0 exactly): o = 0, the empty-row rule
    for (int e = tid; e < 16 * (HD / 4); e += 64 * SNW) {
        const int row = e / (HD / 4), c4 = (e % (HD / 4)) * 4;
        if (q0 + row >= R) continue;
        float M = SNEG;
#pragma unroll
        for (int w = 0; w < SNW; ++w) M = fmaxf(M, sM[w][row]);
        float L = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < SNW; ++w) {
            const float f = __builtin_amdgcn_exp2f((sM[w][row] - M) * sc2);
            L += sL[w][row] * f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += sO[w][row][c4 + r] * f;
        }
        const float inv = L > 0.f ? 1.f / L : 0.f;
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (bf16)(acc[r] * inv);
        *reinterpret_cast<bf16x4*>(a.o + ((long)b * R + q0 + row) * a.ldo + h * HD + c4) = ov;
    }
}

// ---------------------------------------------------------------------------- greedy CTC with carry
// One workgroup per utterance over the step's R logit rows: the waves take the rows' arg-max (the valid columns, ties to the lower index --
// search.h), 64 rows at a time, then one thread walks them in order with the carried {previous arg-max, len}.
__global__ __launch_bounds__(256) void ctc_greedy_stream_kernel(CtcGreedyStreamArgs a) {
    __shared__ int s_am[64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int klen = a.klens ? a.klens[b] : a.pos + a.R;
    int prev = 0, len = 0;
    if (tid == 0) { prev = a.state[b]; len = a.state[a.B + b]; }
    for (int r0 = 0; r0 < a.R; r0 += 64) {
        const int n = min(64, a.R - r0);
        for (int r = wave; r < n; r += 4) {
            const float* z = a.logits + (long)b * a.batch_stride + (long)(r0 + r) * a.ld;
            float mx = NEG_INF; int am = 0;
            for (int c = lane; c < a.C; c += 64) { const float v = z[c]; if (v > mx) { mx = v; am = c; } }
            wave_argmax_first(mx, am);
            if (lane == 0) s_am[r] = am;
        }
        __syncthreads();
        if (tid == 0) {
            for (int r = 0; r < n; ++r) {
                const int t = a.pos + r0 + r;
                if (t >= klen) break;
                const int am = s_am[r];
                if (am != 0 && am != prev && len < a.ld_out) {
                    a.tokens[(long)b * a.ld_out + len] = am;
                    a.frames[(long)b * a.ld_out + len] = t;
                    ++len;
                }
                prev = am;
            }
        }
        __syncthreads();
    }
    if (tid == 0) { a.state[b] = prev; a.state[a.B + b] = len; }
}

// ---------------------------------------------------------------------------- the copies around the windowed front-end
// win [B][W][D] = rows w0 .. w0 + W of the buffered input xbuf [B][cap_frames][D]; rows at or behind lens[b] (the frames of b received, final
// once b has ended) are zero: the engine's own zero fill behind an utterance's end
__global__ void stream_window_kernel(const float* __restrict__ xbuf, const int* __restrict__ lens, float* __restrict__ win, int B, int W, int D,
                                     int w0, long cap_frames) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, n = (long)B * W * D;
    if (i >= n) return;
    const int b = (int)(i / ((long)W * D)); const long rem = i % ((long)W * D); const int r = (int)(rem / D);
    win[i] = w0 + r < lens[b] ? xbuf[((long)b * cap_frames + w0 + r) * D + rem % D] : 0.f;
}
// x32 / x16 [B*R][E] = the window's centre rows v [B*Wp][E] (rows off .. off + R of each utterance) + pe[s + i], added in fp32 in front of the
// bf16 rounding
__global__ void stream_centre_pe_kernel(const float* __restrict__ v, const float* __restrict__ pe, float* __restrict__ x32, bf16* __restrict__ x16,
                                        int B, int R, int E, int Wp, int off, int s) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4, n = (long)B * R * E;
    if (i >= n) return;
    const long row = i / E; const int col = (int)(i % E), b = (int)(row / R), r = (int)(row % R);
    const float4 x = *reinterpret_cast<const float4*>(v + ((long)b * Wp + off + r) * E + col);
    const float4 p = *reinterpret_cast<const float4*>(pe + (long)(s + r) * E + col);
    const float4 y = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
    *reinterpret_cast<float4*>(x32 + i) = y;
    bf16x4 h; h[0] = (bf16)y.x; h[1] = (bf16)y.y; h[2] = (bf16)y.z; h[3] = (bf16)y.w;
    *reinterpret_cast<bf16x4*>(x16 + i) = h;
}

int stream_fail(const char* fn, const char* msg) { mk_set_error(fn, msg); return -1; }

}  // namespace

int mk_attn_stream(const AttnStreamArgs& a, hipStream_t s) {
    const char* fn = "mk_attn_stream";
    if (!a.q || !a.knew || !a.vnew || !a.kc || !a.vc || !a.o) return stream_fail(fn, "null pointer");
    if (a.B < 1 || a.B > 65535 || a.H < 1 || a.H > 65535) return stream_fail(fn, "need 1 <= B, H <= 65535");
    if (a.R < 1) return stream_fail(fn, "need R >= 1");
    if (a.hd != 16 && a.hd != 32 && a.hd != 64) return stream_fail(fn, "head dim must be 16/32/64");
    if (a.pos < 0 || a.cap < 1 || (long)a.pos + a.R > a.cap) return stream_fail(fn, "need 0 <= pos and pos + R <= cap");
    if (a.lo < 0 || a.lo > a.pos) return stream_fail(fn, "need 0 <= lo <= pos");
    if ((a.ldq | a.ldnew | a.ldc | a.batch_stride) & 7 || (a.ldo & 3)) return stream_fail(fn, "row strides must be multiples of 8 (o: 4) elements");
    const dim3 grid((a.R + 15) / 16, a.H, a.B), block(64 * SNW);
    if (a.hd == 64) hipLaunchKernelGGL(attn_stream_kernel<64>, grid, block, 0, s, a);
    else if (a.hd == 32) hipLaunchKernelGGL(attn_stream_kernel<32>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(attn_stream_kernel<16>, grid, block, 0, s, a);
    return LAUNCH_OK();
}

int mk_ctc_greedy_stream(const CtcGreedyStreamArgs& a, hipStream_t s) {
    const char* fn = "mk_ctc_greedy_stream";
    if (!a.logits || !a.state || !a.tokens || !a.frames) return stream_fail(fn, "null pointer");
    if (a.B < 1 || a.R < 1 || a.C < 1 || a.pos < 0 || a.ld_out < 0) return stream_fail(fn, "need B, R, C >= 1, pos >= 0, ld_out >= 0");
    hipLaunchKernelGGL(ctc_greedy_stream_kernel, dim3(a.B), dim3(256), 0, s, a);
    return LAUNCH_OK();
}

int mk_stream_window(const float* xbuf, const int* lens, float* win, int B, int W, int D, int w0, long cap_frames, hipStream_t s) {
    const long n = (long)B * W * D;
    hipLaunchKernelGGL(stream_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, xbuf, lens, win, B, W, D, w0, cap_frames);
    return LAUNCH_OK();
}

int mk_stream_centre_pe(const float* v, const float* pe, float* x32, bf16* x16, int B, int R, int E, int Wp, int off, int s0, hipStream_t s) {
    const long n = (long)B * R * E / 4;                                   // (E % 8 == 0: masr_create)
    hipLaunchKernelGGL(stream_centre_pe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, pe, x32, x16, B, R, E, Wp, off, s0);
    return LAUNCH_OK();
}
