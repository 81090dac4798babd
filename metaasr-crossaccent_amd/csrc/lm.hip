// The backoff n-gram LM of the LM-fused decoders: the host builder of the device tables (masr_lm_create) and the score
// kernel of the test entry.  The device-side lookups are lm.h's lm_context / lm_score; the searches that call them are beam_rows
// (beam.hip: masr_recog_beam_lm and masr_recog_beam_ctc_lm, which compose f(c) = fl(lp(c) + fl(lm_w * lm(c | h))) by one statement)
// and ctc_beam_sweep (ctc_beam.hip).
#include <cmath>
#include <cstring>
#include <atomic>
#include <vector>

#include "kernels.h"
#include "search.h"
#include "lm.h"
#include "../../include/masr.h"

namespace {

// grid ceil(R / 4), 256 threads: one wave per context row.  ctx [R][order - 1], oldest first, -1 in front of a shorter context
__global__ __launch_bounds__(256) void lm_score_kernel(LmDev lm, const int* __restrict__ ctx, int R, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int w = lm.order - 1;
    int tok[LM_MAX_ORDER - 1], n = 0;
#pragma unroll
    for (int i = 0; i < LM_MAX_ORDER - 1; ++i) {
        int t = 0;
        if (i < w) {
            t = ctx[(long)r * w + (w - 1 - i)];
            if (t >= 0 && t < lm.C && n == i) n = i + 1;          // the context ends at the first -1 (or bad id) from the newest end
            else t = 0;
        }
        tok[i] = t;
    }
    const LmCtx x = lm_context(lm, tok, n);
    for (int c = lane; c < lm.C; c += 64) out[(long)r * lm.C + c] = lm_score(lm, x, c);
}

std::atomic<uint32_t> g_lm_serial{1};

struct HostTable { std::vector<LmSlot> slots; uint32_t mask; int shift; };

}  // namespace

int mk_lm_score(const LmDev& lm, const int* ctx, int R, float* out, hipStream_t s) {
    hipLaunchKernelGGL(lm_score_kernel, dim3((R + 3) / 4), dim3(256), 0, s, lm, ctx, R, out);
    return LAUNCH_OK();
}

extern "C" {

masr_lm* masr_lm_create(int order, int C, const int64_t* counts, const int32_t* const* grams, const float* const* logp,
                        const float* const* backoff) {
    const char* fn = "masr_lm_create";
    auto refuse = [&](const char* why) -> masr_lm* { mk_set_error(fn, why); return nullptr; };
    if (order < 1 || order > LM_MAX_ORDER) return refuse("order must be in [1, 4]");
    if (C < 2 || C > 65535) return refuse("the number of classes must be in [2, 65535]");
    if (!counts || !grams || !logp || !backoff) return refuse("null pointer");
    const int sos = 0, eos = C - 1;
    for (int n = 1; n <= order; ++n) {
        if (counts[n - 1] < 0 || counts[n - 1] > (int64_t)1 << 30) return refuse("an n-gram count is out of range");
        if (counts[n - 1] > 0 && (!grams[n - 1] || !logp[n - 1])) return refuse("null pointer");
        if (counts[n - 1] > 0 && n < order && !backoff[n - 1]) return refuse("null pointer (backoff weights of an order below the highest)");
    }
    // every check runs on the host before anything is allocated on the device
    std::vector<float2> uni((size_t)C);
    std::vector<char> seen((size_t)C, 0);
    std::vector<HostTable> tabs((size_t)order - 1);
    int max_probe = counts[0] > 0 ? 1 : 0;
    for (int n = 1; n <= order; ++n) {
        const int64_t cnt = counts[n - 1];
        HostTable* t = nullptr;
        if (n >= 2) {
            t = &tabs[n - 2];
            uint64_t cap = 16; int bits = 4;
            while (cap < 2 * (uint64_t)cnt) { cap <<= 1; ++bits; }
            t->slots.assign(cap, LmSlot{0ull, 0.f, 0.f});
            t->mask = (uint32_t)(cap - 1); t->shift = 64 - bits;
        }
        for (int64_t i = 0; i < cnt; ++i) {
            const int32_t* g = grams[n - 1] + i * n;
            const float lp = logp[n - 1][i], bo = backoff[n - 1] ? backoff[n - 1][i] : 0.f;      // (null: the highest order only)
            if (!std::isfinite(lp) || !std::isfinite(bo) || lp > 0.f || bo > 0.f) return refuse("log-probabilities and backoff weights must be finite and <= 0");
            unsigned long long key = 0;
            for (int j = 0; j < n; ++j) {
                if (g[j] < 0 || g[j] >= C) return refuse("an n-gram holds an id outside [0, C - 1]");
                if (n > 1 && g[j] == eos && j != n - 1) return refuse("</s> may only be the last id of an n-gram");
                if (n > 1 && g[j] == sos && j != 0) return refuse("<s> may only be the first id of an n-gram");
                key = (key << 16) | (unsigned long long)(g[j] + 1);
            }
            if (n == 1) {
                if (seen[g[0]]) return refuse("duplicate n-gram");
                seen[g[0]] = 1;
                uni[g[0]] = make_float2(lp, order == 1 ? 0.f : bo);
                continue;
            }
            uint32_t at = lm_hash(key, t->shift);
            int probes = 1;
            for (;; ++at, ++probes) {                            // ends: the capacity is >= 2 x the count, an empty slot exists
                LmSlot& s = t->slots[at & t->mask];
                if (s.key == key) return refuse("duplicate n-gram");
                if (s.key == 0) { s.key = key; s.logp = lp; s.bo = n == order ? 0.f : bo; break; }
            }
            if (probes > max_probe) max_probe = probes;
        }
    }
    for (int c = 0; c < C; ++c) if (!seen[c]) return refuse("a missing unigram: order 1 must hold every class 0 .. C - 1");

    auto pad = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    int64_t bytes = pad((int64_t)C * sizeof(float2));
    for (const HostTable& t : tabs) bytes += pad((int64_t)t.slots.size() * sizeof(LmSlot));
    masr_lm* lm = new masr_lm();
    memset(&lm->dev, 0, sizeof lm->dev);
    lm->mem = nullptr; lm->bytes = bytes; lm->max_probe = max_probe; lm->serial = g_lm_serial.fetch_add(1);
    for (int n = 0; n < LM_MAX_ORDER; ++n) lm->counts[n] = n < order ? counts[n] : 0;
    auto fail = [&](hipError_t e) -> masr_lm* { mk_set_error(fn, hipGetErrorString(e)); if (lm->mem) hipFree(lm->mem); delete lm; return nullptr; };
    hipError_t e = hipMalloc(&lm->mem, (size_t)bytes);
    if (e != hipSuccess) { lm->mem = nullptr; return fail(e); }
    char* p = (char*)lm->mem;
    lm->dev.order = order; lm->dev.C = C; lm->dev.uni = (const float2*)p;
    if ((e = hipMemcpy(p, uni.data(), (size_t)C * sizeof(float2), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    p += pad((int64_t)C * sizeof(float2));
    for (int n = 2; n <= order; ++n) {
        const HostTable& t = tabs[n - 2];
        lm->dev.tab[n - 2] = LmTable{(const LmSlot*)p, t.mask, t.shift};
        if ((e = hipMemcpy(p, t.slots.data(), t.slots.size() * sizeof(LmSlot), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
        p += pad((int64_t)t.slots.size() * sizeof(LmSlot));
    }
    return lm;
}

void masr_lm_destroy(masr_lm* lm) {
    if (!lm) return;
    hipDeviceSynchronize();                                       // no decode that reads the tables is still in flight
    if (lm->mem) hipFree(lm->mem);
    delete lm;
}

int64_t masr_lm_bytes(const masr_lm* lm) {
    if (!lm) { mk_set_error("masr_lm_bytes", "null model"); return -1; }
    return lm->bytes;
}

}  // extern "C"
