// Backoff n-gram language model on the device (lm.hip): what the host builder, the kernels and the test entry points share.
// Order N <= 4 over C <= 65535 classes.  Unigrams are a dense [C] array of (logp, bo); each order n = 2 .. N has one open-addressing table
// of 16-byte slots {key, logp, bo}.  key = the n ids as id + 1 in 16-bit fields, oldest id highest -- never 0, which marks an empty slot.
// Capacity: a power of two, >= 2 x the count and >= 16, so a table always keeps an empty slot; linear probing from a multiplicative hash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int LM_MAX_ORDER = 4;

struct __attribute__((aligned(16))) LmSlot { unsigned long long key; float logp, bo; };
struct LmTable { const LmSlot* slots; uint32_t mask; int shift; };   // capacity mask + 1 = 2^(64 - shift)
struct LmDev {
    int order, C;
    const float2* uni;                                              // [C] (logp, bo)
    LmTable tab[LM_MAX_ORDER - 1];                                  // tab[n - 2]: order n
};

__host__ __device__ __forceinline__ uint32_t lm_hash(unsigned long long key, int shift) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

// (logp, bo) of the n-gram `key`, or false.  The loop ends at an empty slot and, whatever the table holds, after mask + 1 probes.
__device__ __forceinline__ bool lm_find(const LmTable& t, unsigned long long key, float& logp, float& bo) {
    uint32_t i = lm_hash(key, t.shift);
    for (uint32_t n = 0; n <= t.mask; ++n, ++i) {
        const LmSlot s = t.slots[i & t.mask];
        if (s.key == key) { logp = s.logp; bo = s.bo; return true; }
        if (s.key == 0) return false;
    }
    return false;
}

// A hypothesis's LM context, wave-uniform: the last n <= N - 1 tokens of [sos] + h (tok[0] = the newest), and per length k = 1 .. n the
// packed ids of the last k tokens with that k-gram's backoff weight (has[k - 1]: it is an n-gram of the model).
struct LmCtx {
    int n;
    unsigned long long key[LM_MAX_ORDER - 1];
    float bo[LM_MAX_ORDER - 1];
    bool has[LM_MAX_ORDER - 1];
};
__device__ __forceinline__ LmCtx lm_context(const LmDev& lm, const int (&tok)[LM_MAX_ORDER - 1], int n) {
    LmCtx x;
    x.n = n;
    unsigned long long key = 0;
#pragma unroll
    for (int k = 1; k < LM_MAX_ORDER; ++k) {
        x.key[k - 1] = 0; x.bo[k - 1] = 0.f; x.has[k - 1] = false;
        if (k > n) continue;
        key |= (unsigned long long)(tok[k - 1] + 1) << (16 * (k - 1));      // older tokens go into higher fields
        x.key[k - 1] = key;
        if (k == 1) { x.bo[0] = lm.uni[tok[0]].y; x.has[0] = true; }
        else { float lp; x.has[k - 1] = lm_find(lm.tab[k - 2], key, lp, x.bo[k - 1]); }
    }
    return x;
}
// lm(c | h): from the longest context down, the first order that holds (g, c) gives acc + logp; a context g that is an n-gram of the
// model adds its backoff weight on the way down.  fp32 additions in exactly that order (acc starts at 0.f).
__device__ __forceinline__ float lm_score(const LmDev& lm, const LmCtx& x, int c) {
    float acc = 0.f;
#pragma unroll
    for (int k = LM_MAX_ORDER - 1; k >= 1; --k) {
        if (k > x.n) continue;
        float lp, bo;
        if (lm_find(lm.tab[k - 1], (x.key[k - 1] << 16) | (unsigned long long)(c + 1), lp, bo)) return acc + lp;
        if (x.has[k - 1]) acc += x.bo[k - 1];
    }
    return acc + lm.uni[c].x;
}

// the handle of include/masr.h
struct masr_lm {
    LmDev dev;
    void* mem;                                                      // one device allocation: unigrams, then the tables
    int64_t bytes;
    int64_t counts[LM_MAX_ORDER];
    int max_probe;                                                  // the longest probe chain an insertion walked (slots examined)
    uint32_t serial;                                                // unique per created model: keys the cached step graph
};
