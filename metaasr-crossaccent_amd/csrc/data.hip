// Ragged gather + zero pad of the numpy-memmap fbank shard rows (reference: CommonVoiceDataset.__getitem__
// and collate_fn, src/io/dataset.py:21-33,147-153) as one coalesced HBM pass: the shard [sum T_i][D] is
// resident in HBM, each utterance is rows [row_start, row_start+len).
#include "../../include/masr.h"
#include "common.h"
#include "kernels.h"

namespace {
__global__ void gather_pad_kernel(const float* __restrict__ feat, const long* __restrict__ row_start,
                                  const int* __restrict__ lens, float* __restrict__ xs, int B, int Tmax, int D) {
    const long n = (long)B * Tmax * D;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int d = (int)(i % D);
        const int t = (int)((i / D) % Tmax);
        const int b = (int)(i / ((long)D * Tmax));
        xs[i] = t < lens[b] ? feat[(row_start[b] + t) * D + d] : 0.f;
    }
}

// SpecAugment (Park et al. 2019) on the padded batch, out of place (the warp reads neighbouring rows): a linear time warp around one
// centre, frequency masks and time masks, all drawn per utterance from the step's dropout seed (include/masr.h masr_specaug has the
// definition).  grid (x, B): the utterance is workgroup-uniform, its <= 34 hash words and the draws made of them are formed once per
// workgroup in LDS; the lanes then walk the flat [T * D] range of the utterance (D = 83: rows are not 16-byte aligned, so the accesses
// are scalar, consecutive lanes on consecutive floats).  One read of x -- a second, adjacent row where the warp interpolates, an L2 hit --
// and one write; masked and padding cells are not read at all, and no row >= n of the input ever is.
constexpr uint32_t SPECAUG_SITE = 0x53504147u;
struct SpecAugDraws { int n, warp, c, cw, f0[8], f1[8], t0[8], t1[8]; };
__device__ __forceinline__ int uni(uint32_t w, int r) { return (int)(((uint64_t)w * (uint32_t)r) >> 32); }     // [0, r)

__global__ void __launch_bounds__(256) specaug_kernel(const float* __restrict__ xs, const int* __restrict__ lens, float* __restrict__ out, int T, int D,
                                                       masr_specaug_policy p, uint32_t seed, const uint32_t* __restrict__ seed_ptr) {
    __shared__ uint32_t word[34];
    __shared__ SpecAugDraws dr;
    const int b = blockIdx.y;
    if (threadIdx.x < 34) word[threadIdx.x] = dropout_word(dropout_key(seed_ptr ? *seed_ptr : seed, SPECAUG_SITE), (uint32_t)b * 64u + threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = lens[b];
        n = n < 0 ? 0 : n > T ? T : n;
        dr.n = n; dr.warp = 0; dr.c = dr.cw = 0;
        const int W = p.time_warp;
        if (W > 0 && W <= (n - 1) / 2) {                                     // n > 2W, without forming 2W for an absurd W
            dr.c = W + uni(word[0], n - 2 * W);
            dr.cw = dr.c + uni(word[1], 2 * W - 1) - (W - 1);                  // 1 <= c' <= n - 2
            dr.warp = dr.cw != dr.c;
        }
        const int Fm = p.freq_width < p.freq_bins ? p.freq_width : p.freq_bins;
        for (int i = 0; i < p.freq_masks; ++i) {
            const int f = uni(word[2 + 2 * i], Fm + 1);
            dr.f0[i] = uni(word[3 + 2 * i], p.freq_bins - f + 1); dr.f1[i] = dr.f0[i] + f;
        }
        const int byratio = (int)floorf(__fmul_rn(p.time_ratio, (float)n));
        const int cap = p.time_width < byratio ? p.time_width : byratio;
        for (int i = 0; i < p.time_masks; ++i) {
            const int tau = uni(word[18 + 2 * i], cap + 1);
            dr.t0[i] = uni(word[19 + 2 * i], n - tau + 1); dr.t1[i] = dr.t0[i] + tau;
        }
    }
    __syncthreads();
    const int n = dr.n, c = dr.c, cw = dr.cw;
    const bool warp = dr.warp != 0;
    const float* __restrict__ x = xs + (long)b * T * D;
    float* __restrict__ y = out + (long)b * T * D;
    const int total = T * D;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int t = e / D, d = e - t * D;
        bool live = t < n;
        for (int i = 0; i < p.freq_masks; ++i) live = live && !(d >= dr.f0[i] && d < dr.f1[i]);
        for (int i = 0; i < p.time_masks; ++i) live = live && !(t >= dr.t0[i] && t < dr.t1[i]);
        float v = 0.f;
        if (live) {
            int i = t, r = 0, den = 1;
            if (warp) {
                // piecewise-linear map of the output rows onto the source: [0, c') -> [0, c), [c', n - 1] -> [c, n - 1]; exact integer floor
                int num, base;
                if (t < cw) { num = t * c; den = cw; base = 0; } else { num = (t - cw) * (n - 1 - c); den = n - 1 - cw; base = c; }
                const int q = num / den;
                i = base + q; r = num - q * den;
            }
            v = x[(long)i * D + d];                                            // r == 0: a bit-exact copy
            if (r != 0) {
                const int i1 = i + 1 < n ? i + 1 : n - 1;                      // (i + 1 <= n - 1 whenever r != 0; the clamp keeps a bad length inside)
                v = fmaf((float)r / (float)den, x[(long)i1 * D + d] - v, v);
            }
        }
        y[e] = v;
    }
}
}  // namespace

int mk_specaug(const float* xs, const int* lens, float* out, int B, int T, int D, const masr_specaug_policy& p, uint32_t seed,
               const uint32_t* seed_ptr, hipStream_t s) {
    if (B <= 0 || T <= 0 || D <= 0) return 0;
    // (the caller has vetted the policy and that T * T and T * D fit an int: masr_specaug_check)
    int nx = (T * D + 1023) / 1024;                                            // ~4 elements per lane: the per-workgroup draws stay a small share
    if (nx > 128) nx = 128;
    hipLaunchKernelGGL(specaug_kernel, dim3((unsigned)nx, (unsigned)B), dim3(256), 0, s, xs, lens, out, T, D, p, seed, seed_ptr);
    return LAUNCH_OK();
}

int mk_gather_pad(const float* feat, const long* row_start, const int* lens, float* xs, int B, int Tmax, int D, hipStream_t s) {
    const long n = (long)B * Tmax * D;
    if (n == 0) return 0;
    long nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(gather_pad_kernel, dim3((unsigned)nb), dim3(256), 0, s, feat, row_start, lens, xs, B, Tmax, D);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
