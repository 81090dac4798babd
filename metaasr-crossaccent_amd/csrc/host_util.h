// Host-side bookkeeping shared by the engines (engine.hip / train.hip / recog.hip, blstm.hip) and the standalone kernel entry
// points (test_abi.hip): the parameter table entry, the bump allocator of the workspace, the early-return macro.
#pragma once
#include <cstdint>
#include <string>

struct PInfo { std::string name; int64_t shape[4]; int ndim; int64_t off; int64_t numel; };

struct Arena {
    char* base; int64_t cap, off;
    template <class T> T* get(int64_t n) {
        const int64_t bytes = (n * (int64_t)sizeof(T) + 255) & ~(int64_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += bytes;
        return p;
    }
};

#define CK(expr) do { if ((expr) != 0) return -1; } while (0)

// The positions of tok [B][L] grouped by token id for the embedding backward (mk_embed_bwd): order[start[v] .. start[v + 1]) = the positions
// b * L + l that hold token v, ascending (a stable counting sort); start has V + 1 entries.  Of row b the positions 0 .. olens[b] count (all L
// when olens is null).  Every token must lie in [0, V).  (train.hip)
void group_positions_by_token(const int* tok, int B, int L, const int64_t* olens, int V, int* order, int* start);
