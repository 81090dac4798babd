// Contextual phrase biasing on the device (bias.hip): what the host builder, the CTC prefix beam and the test entry points share.
// A trie over P phrases of 1 .. 64 tokens over C <= 65535 classes: its nodes are the distinct prefixes of the phrases, the root is node 0, at
// most 2^20 nodes.  One open-addressing table of 16-byte slots {key, child} maps (node, token) -> child; key = (node + 1) << 16 | (token + 1),
// never 0, which marks an empty slot.  Capacity, hash and probing are lm.h's: a power of two, >= 2 x the edges and >= 16, so the table always
// keeps an empty slot; linear probing from lm_hash.  revoke[u] = depth(u) - e(u) is one byte per node, e(u) = the length of the longest phrase
// that is a prefix of, or equal to, u's string (0: none): the tokens of an unfinished match that no completed phrase has earned.
//
// The state of a hypothesis is (node u, credited tokens n), a function of its tokens alone, advanced by bias_step.  There are NO failure links:
// a match that breaks gives back its unearned tokens and restarts at the root with the current token (WeNet's context graph does the same), so
// overlapping restarts are missed on purpose -- the phrase `a a b` is not found in `a a a b`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lm.h"

constexpr int BIAS_MAX_PHRASE = 64, BIAS_MAX_NODES = 1 << 20, BIAS_MAX_PHRASES = 65536;

struct __attribute__((aligned(16))) BiasSlot { unsigned long long key; int child; int pad; };
struct BiasDev {
    int C, nodes;
    const BiasSlot* slots; uint32_t mask; int shift;                // capacity mask + 1 = 2^(64 - shift)
    const uint8_t* revoke;                                          // [nodes]
};

__host__ __device__ __forceinline__ unsigned long long bias_key(int node, int c) {
    return ((unsigned long long)(node + 1) << 16) | (unsigned long long)(c + 1);
}

// child(u, c), or -1.  The loop ends at an empty slot and, whatever the table holds, after mask + 1 probes.  A class outside [0, C) has no child.
__device__ __forceinline__ int bias_child(const BiasDev& d, int u, int c) {
    if (c < 0 || c >= d.C) return -1;
    const unsigned long long key = bias_key(u, c);
    uint32_t i = lm_hash(key, d.shift);
    for (uint32_t n = 0; n <= d.mask; ++n, ++i) {
        const BiasSlot s = d.slots[i & d.mask];
        if (s.key == key) return s.child;
        if (s.key == 0) return -1;
    }
    return -1;
}

// (u, n) -> the state behind token c: at most two lookups
__device__ __forceinline__ void bias_step(const BiasDev& d, int& u, int& n, int c) {
    int v = bias_child(d, u, c);
    if (v >= 0) { u = v; n += 1; return; }
    if (u != 0) {                                                   // (the root has revoke 0 and its lookup has just failed)
        n -= (int)d.revoke[u];                                      // the unfinished match is taken back, the token is retried from the root
        v = bias_child(d, 0, c);
        if (v >= 0) { u = v; n += 1; return; }
    }
    u = 0;
}
// the count at the end of the utterance
__device__ __forceinline__ int bias_final(const BiasDev& d, int u, int n) { return n - (int)d.revoke[u]; }

// the handle of include/masr.h
struct masr_bias {
    BiasDev dev;
    void* mem;                                                      // one device allocation: the table, then the revoke bytes
    int64_t bytes;
    int phrases;
    int max_probe;                                                  // the longest probe chain an insertion walked (slots examined)
    uint32_t serial;                                                // unique per created list
};
