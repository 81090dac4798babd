// The phrase automaton of contextual biasing: the host builder of the device trie (masr_bias_create) and the step kernel of the
// test entry.  The device-side lookups are bias.h's bias_child / bias_step / bias_final; the search that calls them is ctc_beam_sweep<LM, true>
// (ctc_beam.hip).
#include <cstring>
#include <atomic>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "bias.h"
#include "../../include/masr.h"

namespace {

// grid ceil(count / 256), 256 threads: one state per thread.  A node outside [0, nodes) gives (-1, -1).
__global__ __launch_bounds__(256) void bias_step_kernel(BiasDev d, const int* __restrict__ nodes_in, const int* __restrict__ n_in,
                                                        const int* __restrict__ tokens, int count, int* __restrict__ nodes_out,
                                                        int* __restrict__ n_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int u = nodes_in[i], n = n_in[i];
    if (u < 0 || u >= d.nodes) { nodes_out[i] = -1; n_out[i] = -1; return; }
    bias_step(d, u, n, tokens[i]);
    nodes_out[i] = u; n_out[i] = n;
}

std::atomic<uint32_t> g_bias_serial{1};

}  // namespace

int mk_bias_step(const BiasDev& d, const int* nodes_in, const int* n_in, const int* tokens, int count, int* nodes_out, int* n_out, hipStream_t s) {
    hipLaunchKernelGGL(bias_step_kernel, dim3((count + 255) / 256), dim3(256), 0, s, d, nodes_in, n_in, tokens, count, nodes_out, n_out);
    return LAUNCH_OK();
}

extern "C" {

masr_bias* masr_bias_create(int C, int P, const int32_t* tokens, const int64_t* off) {
    const char* fn = "masr_bias_create";
    auto refuse = [&](const char* why) -> masr_bias* { mk_set_error(fn, why); return nullptr; };
    if (!tokens || !off) return refuse("null pointer");
    if (C < 3 || C > 65535) return refuse("the number of classes must be in [3, 65535]");
    if (P < 1 || P > BIAS_MAX_PHRASES) return refuse("the number of phrases must be in [1, 65536]");
    if (off[0] < 0) return refuse("a phrase offset is negative");
    // every check runs on the host before anything is allocated on the device: the trie first, the table from its edges
    std::unordered_map<unsigned long long, int> edge;
    std::vector<int> parent(1, -1), depth(1, 0), edge_tok(1, -1);
    std::vector<char> terminal(1, 0);
    for (int i = 0; i < P; ++i) {
        const int64_t len = off[i + 1] - off[i];
        if (len < 1 || len > BIAS_MAX_PHRASE) return refuse("a phrase must hold 1 to 64 tokens");
        int u = 0;
        for (int64_t j = 0; j < len; ++j) {
            const int c = tokens[off[i] + j];
            if (c < 1 || c > C - 2) return refuse("a phrase holds a token outside [1, C - 2]");
            const auto it = edge.find(bias_key(u, c));
            if (it != edge.end()) { u = it->second; continue; }
            if ((int)parent.size() >= BIAS_MAX_NODES) return refuse("the phrases have more than 2^20 distinct prefixes");
            const int v = (int)parent.size();
            edge.emplace(bias_key(u, c), v);
            parent.push_back(u); depth.push_back(depth[u] + 1); edge_tok.push_back(c); terminal.push_back(0);
            u = v;
        }
        if (terminal[u]) return refuse("duplicate phrase");
        terminal[u] = 1;
    }
    const int nodes = (int)parent.size();
    std::vector<uint8_t> revoke((size_t)nodes, 0);
    {
        std::vector<int> earned((size_t)nodes, 0);                 // e(u); a node's parent has the lower index
        for (int u = 1; u < nodes; ++u) {
            earned[u] = terminal[u] ? depth[u] : earned[parent[u]];
            revoke[u] = (uint8_t)(depth[u] - earned[u]);
        }
    }
    const int64_t edges = nodes - 1;
    uint64_t cap = 16; int bits = 4;
    while (cap < 2 * (uint64_t)edges) { cap <<= 1; ++bits; }
    std::vector<BiasSlot> slots(cap, BiasSlot{0ull, 0, 0});
    const uint32_t mask = (uint32_t)(cap - 1); const int shift = 64 - bits;
    int max_probe = 0;
    for (int v = 1; v < nodes; ++v) {                              // in node order: the table is a function of the phrase list
        const unsigned long long key = bias_key(parent[v], edge_tok[v]);
        uint32_t at = lm_hash(key, shift);
        int probes = 1;
        for (;; ++at, ++probes) {                                 // ends: the capacity is >= 2 x the edges, an empty slot exists
            BiasSlot& s = slots[at & mask];
            if (s.key == 0) { s.key = key; s.child = v; break; }
        }
        if (probes > max_probe) max_probe = probes;
    }

    auto pad = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    const int64_t tab_bytes = pad((int64_t)cap * sizeof(BiasSlot)), bytes = tab_bytes + pad(nodes);
    masr_bias* b = new masr_bias();
    memset(&b->dev, 0, sizeof b->dev);
    b->mem = nullptr; b->bytes = bytes; b->phrases = P; b->max_probe = max_probe; b->serial = g_bias_serial.fetch_add(1);
    auto fail = [&](hipError_t e) -> masr_bias* { mk_set_error(fn, hipGetErrorString(e)); if (b->mem) hipFree(b->mem); delete b; return nullptr; };
    hipError_t e = hipMalloc(&b->mem, (size_t)bytes);
    if (e != hipSuccess) { b->mem = nullptr; return fail(e); }
    char* p = (char*)b->mem;
    b->dev.C = C; b->dev.nodes = nodes; b->dev.slots = (const BiasSlot*)p; b->dev.mask = mask; b->dev.shift = shift;
    b->dev.revoke = (const uint8_t*)(p + tab_bytes);
    if ((e = hipMemcpy(p, slots.data(), slots.size() * sizeof(BiasSlot), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p + tab_bytes, revoke.data(), (size_t)nodes, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    return b;
}

void masr_bias_destroy(masr_bias* b) {
    if (!b) return;
    hipDeviceSynchronize();                                       // no decode that reads the table is still in flight
    if (b->mem) hipFree(b->mem);
    delete b;
}

int64_t masr_bias_bytes(const masr_bias* b) {
    if (!b) { mk_set_error("masr_bias_bytes", "null phrase list"); return -1; }
    return b->bytes;
}

int masr_bias_nodes(const masr_bias* b) {
    if (!b) { mk_set_error("masr_bias_nodes", "null phrase list"); return -1; }
    return b->dev.nodes;
}

}  // extern "C"
