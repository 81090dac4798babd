// Shallow fusion of a backoff n-gram LM into the attention beam (masr_recog_beam_lm): the host builder of the device tables
// (masr_lm_create), the per-step kernel that replaces beam_row_topk in this mode's step, and the score kernel of the test entry.
//
// beam_lm_topk, one wave per live row r (hypothesis h of st - 1 tokens, score s):
//   lane 0 walks tok_hist / par_hist back for the last min(N - 1, st) tokens of [sos] + h and broadcasts them; the wave looks up the
//   context's <= N - 1 backoff weights once; row_lse over the logits; the lanes stride over the C classes: lm(c | h) from at most N - 1
//   table probes and the dense unigram, f(c) = fl(lp(c) + fl(lm_w * lm(c | h))) stored to the row of the [R][ld] fp32 workspace;
//   row_top_n over that row (f descending, class ascending; eos skipped below minlen) writes list_tok and list_score = fl(s + f).
// One launch, not a fuse launch and a top-K launch: the fused row is written and read back by the same wave (8 KB at C = 2048, it stays
// in the L1 / L2 of its CU), the row's log-sum-exp is needed by the fuse anyway, and the step graph keeps the plain beam's launch count.
// A lane's probes of its ceil(C / 64) classes are independent loads, so they overlap.
#include <cmath>
#include <cstring>
#include <atomic>
#include <vector>

#include "kernels.h"
#include "search.h"
#include "lm.h"
#include "../../include/masr.h"

namespace {

// The LM context of row r's hypothesis (st - 1 tokens), for the whole wave: token s of h is tok_hist[s - 1][row], row = the hypothesis's row
// after step s; position 0 is sos.  Lane 0 walks the histories and broadcasts.  Reads are clamped as in beam_embed_step: a stale entry can
// neither leave the class range nor the utterance's rows; n <= order - 1, so no order the LM lacks is ever indexed
__device__ __forceinline__ LmCtx row_lm_context(const BeamArgs& a, const LmDev& lm, int r, int st, int lane) {
    const int u0 = (r / a.K) * a.K;
    const int n = min(lm.order - 1, st);
    int tok[LM_MAX_ORDER - 1];
    int row = r;
#pragma unroll
    for (int i = 0; i < LM_MAX_ORDER - 1; ++i) {
        int t = a.sos;
        const int s = st - 1 - i;
        if (lane == 0 && i < n && s >= 1) {
            t = a.tok_hist[(long)(s - 1) * a.R + row];
            int par = a.par_hist[(long)(s - 1) * a.R + row];
            if (t < 0 || t >= a.C) t = a.sos;
            if (par < u0 || par >= u0 + a.K) par = row;
            row = par;
        }
        tok[i] = __shfl(t, 0, 64);
    }
    return lm_context(lm, tok, n);
}

// grid ceil(R / 4), 256 threads: one wave per row
__global__ __launch_bounds__(256) void beam_lm_topk_kernel(BeamArgs a, LmDev lm, float lm_w, const float* __restrict__ logits, long ld,
                                                          float* __restrict__ fused, long ldf) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int u = r / a.K, st = *a.step;
    if (a.fin[u]) return;
    const float ps = a.score[r];
    int* lt = a.list_tok + (long)r * a.K;
    float* ls = a.list_score + (long)r * a.K;
    if (ps == NEG_INF) {                                         // dead row: an empty list
        for (int i = lane; i < a.K; i += 64) { lt[i] = -1; ls[i] = NEG_INF; }
        return;
    }
    const LmCtx x = row_lm_context(a, lm, r, st, lane);
    const float* z = logits + (long)r * ld;
    float* fz = fused + (long)r * ldf;
    const bool no_eos = (st - 1) < a.minlen[u];                  // the hypothesis has st - 1 tokens
    const RowLse l = row_lse(z, a.C, lane);
    for (int c = lane; c < a.C; c += 64) {
        const float lp = (z[c] - l.mx) - l.log_s;
        fz[c] = __fadd_rn(lp, __fmul_rn(lm_w, lm_score(lm, x, c)));      // two roundings: no fma
    }
    __threadfence_block();                                       // lane 0 reads below what the other lanes of its wave stored
    row_top_n<false>(fz, a.C, a.K, lane, [&](int c) { return no_eos && c == a.eos; },
                     [&](int i, int c) { lt[i] = c; ls[i] = c < 0 ? NEG_INF : ps + fz[c]; });
}

// The pre-beam of the joint LM beam (masr_recog_beam_ctc_lm).  grid ceil(R / 4), 256 threads: one wave per live row.  The
// fused row g(c) = fl(lp(c) + fl(lm_w * lm(c | h))) is beam_lm_topk's f(c), composed the same way; the row's P best classes by (g
// descending, class ascending; blank never, eos once the hypothesis has minlen tokens) go to pre_tok, token -1 past the end.  Then the lanes
// share the P entries: the attention lp(c) to pre_lp and the weighted LM term fl(lm_w * lm(c | h)) to pre_lm, each computed again from
// its inputs (the same expressions: the same bits), so no second [R][Cp] row is kept for them.
__global__ __launch_bounds__(256) void beam_ctc_lm_prebeam_kernel(BeamArgs a, LmDev lm, const float* __restrict__ logits, long ld,
                                                                 float* __restrict__ fused, long ldf) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int u = r / a.K, st = *a.step;
    if (a.fin[u] || a.score[r] == NEG_INF) return;               // (the prefix kernel gives a dead row its empty list)
    const float lm_w = a.wts[2];
    int* pt = a.pre_tok + (long)r * a.P;
    const LmCtx x = row_lm_context(a, lm, r, st, lane);
    const float* z = logits + (long)r * ld;
    float* gz = fused + (long)r * ldf;
    const bool no_eos = (st - 1) < a.minlen[u];
    const RowLse l = row_lse(z, a.C, lane);
    for (int c = lane; c < a.C; c += 64) gz[c] = add_rn((z[c] - l.mx) - l.log_s, mul_rn(lm_w, lm_score(lm, x, c)));
    __threadfence_block();                                       // lane 0 reads below what the other lanes of its wave stored
    row_top_n<false>(gz, a.C, a.P, lane, [&](int c) { return c == 0 || (no_eos && c == a.eos); }, [&](int i, int c) { pt[i] = c; });
    __threadfence_block();                                       // and the lanes read what lane 0 stored
    for (int i = lane; i < a.P; i += 64) {
        const int c = pt[i];
        const bool ok = c > 0 && c < a.C;
        a.pre_lp[(long)r * a.P + i] = ok ? (z[c] - l.mx) - l.log_s : NEG_INF;
        a.pre_lm[(long)r * a.P + i] = ok ? mul_rn(lm_w, lm_score(lm, x, c)) : 0.f;
    }
}

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

int mk_beam_lm_topk(const BeamArgs& a, const LmDev& lm, float lm_w, const float* logits, long ld, float* fused, long ldf, hipStream_t s) {
    if (a.K < 1 || a.K > 64 || lm.order < 1 || lm.order > LM_MAX_ORDER || lm.C != a.C || ldf < a.C) {
        mk_set_error("mk_beam_lm_topk", "need 1 <= K <= 64, an LM of order 1 .. 4 over the beam's classes, ldf >= C"); return -1;
    }
    hipLaunchKernelGGL(beam_lm_topk_kernel, dim3((a.R + 3) / 4), dim3(256), 0, s, a, lm, lm_w, logits, ld, fused, ldf);
    return LAUNCH_OK();
}
int mk_beam_ctc_lm_prebeam(const BeamArgs& a, const LmDev& lm, const float* logits, long ld, float* fused, long ldf, hipStream_t s) {
    if (a.K < 1 || a.K > 64 || a.P < 1 || a.P > 96 || lm.order < 1 || lm.order > LM_MAX_ORDER || lm.C != a.C || ldf < a.C || !a.wts || !a.pre_lm) {
        mk_set_error("mk_beam_ctc_lm_prebeam", "need 1 <= K <= 64, 1 <= P <= 96, an LM of order 1 .. 4 over the beam's classes, ldf >= C"); return -1;
    }
    hipLaunchKernelGGL(beam_ctc_lm_prebeam_kernel, dim3((a.R + 3) / 4), dim3(256), 0, s, a, lm, logits, ld, fused, ldf);
    return LAUNCH_OK();
}
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
