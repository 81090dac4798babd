// CTC prefix beam search over a CTC output layer alone (masr_ctc_beam_search; Hannun et al. 2014, with merging).
//
//   ctc_beam_frames   one wave per valid frame row (b, t < enc_len): the row's log-sum-exp, x_t(blank) and S_t = its P best emittable
//                     classes (logit descending, class ascending -- x_t is monotone in the logit) with their log-probs
//   ctc_beam_sweep    one workgroup per utterance, serial over its frames: beam and candidates in LDS, one back-pointer record per kept
//                     entry and frame in the work buffer; its tail walks the records of the final beam and writes the N-best list
//
// x_t(c) = logit - lse with lse = max + log(sum exp(logit - max)), the same expression in both kernels, so a class scores the same whether
// it is read from S_t or gathered as a prefix's last token.  All beam arithmetic is fp32 in the written order.
//
// Prefix identity is (length, 64-bit rolling hash of the tokens): an entry carries its own hash and the hash of the prefix without its last
// token, so "h + c is the beam entry h'" is  len(h') == len(h) + 1, parent_hash(h') == hash(h), last(h') == c.  Two different prefixes of
// one beam with equal length and equal hash would be merged wrongly (DESIGN 5.3 has the odds).
//
// ctc_beam_sweep<true> is the same sweep with a backoff n-gram LM and a per-token bonus fused into the ranking (masr_ctc_beam_search_lm,
// DESIGN 5.6).  p_b and p_nb stay purely acoustic; an entry also carries lmacc(h), the fp32 sum of its tokens' fl(fl(lm_w * lm(c | h)) +
// len_bonus), and its LM context as one 64-bit word: the last <= 3 ids of [sos] + h as id + 1 in 16-bit fields, newest lowest -- the
// order-k key of lm.h is a mask of it, so no record is walked for a context.  A candidate ranks by fl(acoustic score + lmacc(prefix)).
// Per frame: every entry's <= N - 1 context backoffs are looked up once, next to the stay's gathers; after the merge, each surviving
// (entry, class) pair issues its <= N - 1 first probes and the unigram load together and resolves them from the longest order down
// (lm_score's order of additions); a merged pair needs no LM value, its target has one.  The tail adds fl(lm_w * lm(eos | h)) and re-ranks
// the final beam.  ctc_beam_sweep<false> compiles to the sweep without any of it.
#include <cmath>

#include "kernels.h"
#include "search.h"
#include "lm.h"

namespace {

constexpr int SW_THREADS = 256, SW_WAVES = SW_THREADS / 64, KMAX = 64;
constexpr unsigned long long HASH_EMPTY = 0xcbf29ce484222325ull;

__device__ __forceinline__ unsigned long long hash_push(unsigned long long h, int c) {
    h = (h ^ (unsigned long long)(c + 1)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
__device__ __forceinline__ int clamp_len(int n, int Tp) { return n < 0 ? 0 : (n > Tp ? Tp : n); }

// ---- the LM side of ctc_beam_sweep<true>
struct CtcLmArgs { LmDev lm; float lm_w, len_bonus; float* am; };      // am [B][nbest]: the acoustic totals

constexpr unsigned long long CTX_MASK = (1ull << 48) - 1;
__device__ __forceinline__ unsigned long long ctx_push(unsigned long long ctx, int c) { return ((ctx << 16) | (unsigned long long)(c + 1)) & CTX_MASK; }
__device__ __forceinline__ unsigned long long ctx_key(unsigned long long ctx, int k) { return ctx & ((1ull << (16 * k)) - 1); }   // 1 <= k <= 3
// tokens of [sos] + h that the model's order lets a context of a len-token prefix use
__device__ __forceinline__ int ctx_len(const LmDev& lm, int len) { return min(lm.order - 1, len + 1); }

// the backoff weights of the context's suffixes of length 1 .. n (lm_context's lookups, from the packed word): bo[k - 1], bit k - 1 of the
// result = that suffix is an n-gram of the model
__device__ __forceinline__ int ctx_backoffs(const LmDev& lm, unsigned long long ctx, int n, float (&bo)[LM_MAX_ORDER - 1]) {
    int has = 0;
#pragma unroll
    for (int k = 1; k < LM_MAX_ORDER; ++k) {
        bo[k - 1] = 0.f;
        if (k > n) continue;
        if (k == 1) { bo[0] = lm.uni[(int)(ctx & 0xffff) - 1].y; has |= 1; }
        else { float lp; if (lm_find(lm.tab[k - 2], ctx_key(ctx, k), lp, bo[k - 1])) has |= 1 << (k - 1); }
    }
    return has;
}
// lm_find whose first probe was loaded by the caller (key k0 and logp lp0 of the slot at index i0): the remaining probes are bounded as
// lm_find's are
__device__ __forceinline__ bool lm_find_rest(const LmTable& t, unsigned long long key, uint32_t i0, unsigned long long k0, float lp0, float& logp) {
    uint32_t i = i0;
    for (uint32_t n = 0; n <= t.mask; ++n) {
        if (k0 == key) { logp = lp0; return true; }
        if (k0 == 0) return false;
        const LmSlot s = t.slots[++i & t.mask];
        k0 = s.key; lp0 = s.logp;
    }
    return false;
}
// lm(c | h) in lm_score's order of additions, from the packed context, its n and its backoffs.  The first probes of all orders and the
// unigram are independent loads, issued before any of them is looked at.
__device__ __forceinline__ float lm_score_packed(const LmDev& lm, unsigned long long ctx, int n, const float (&bo)[LM_MAX_ORDER - 1], int has, int c) {
    unsigned long long key[LM_MAX_ORDER - 1], k0[LM_MAX_ORDER - 1];
    uint32_t i0[LM_MAX_ORDER - 1];
    float lp0[LM_MAX_ORDER - 1];
#pragma unroll
    for (int k = 1; k < LM_MAX_ORDER; ++k) {
        if (k > n) continue;                                     // (n <= order - 1: tab[k - 1] is an order the model has)
        key[k - 1] = (ctx_key(ctx, k) << 16) | (unsigned long long)(c + 1);
        i0[k - 1] = lm_hash(key[k - 1], lm.tab[k - 1].shift) & lm.tab[k - 1].mask;
        const LmSlot s0 = lm.tab[k - 1].slots[i0[k - 1]];
        k0[k - 1] = s0.key; lp0[k - 1] = s0.logp;
    }
    const float uni = lm.uni[c].x;
    float acc = 0.f;
#pragma unroll
    for (int k = LM_MAX_ORDER - 1; k >= 1; --k) {
        if (k > n) continue;
        float lp;
        if (lm_find_rest(lm.tab[k - 1], key[k - 1], i0[k - 1], k0[k - 1], lp0[k - 1], lp)) return add_rn(acc, lp);
        if (has >> (k - 1) & 1) acc = add_rn(acc, bo[k - 1]);
    }
    return add_rn(acc, uni);
}

// grid ceil(B*Tp / 4), 256 threads: one wave per frame row b*Tp + t
__global__ __launch_bounds__(256) void ctc_beam_frames_kernel(CtcBeamArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)a.B * a.Tp) return;
    const int b = (int)(row / a.Tp), t = (int)(row % a.Tp);
    if (t >= clamp_len(a.enc_lens[b], a.Tp)) return;
    const float* z = a.logits + row * a.ld;
    const RowLse l = row_lse(z, a.C, lane);
    const float lse = l.mx + l.log_s;
    if (lane == 0) { a.lse[row] = lse; a.xb[row] = z[a.blank] - lse; }
    int* sc = a.s_cls + row * a.P;
    float* sl = a.s_lp + row * a.P;
    // (the row runs out on NaN rows only: P never exceeds the emittable classes)
    row_top_n<true>(z, a.C, a.P, lane, [&](int c) { return c == a.blank || c == a.eos; },
                    [&](int i, int c) { sc[i] = c; sl[i] = c < 0 ? NEG_INF : z[c] - lse; });
}

// grid B, 256 threads.  Candidate index of frame t: parent rank k, then stay (0) or position j in S_t (1 + j): idx = k * (P + 1) + ...,
// so "score descending, index ascending" is the selection order of DESIGN 5.3.  s_sc holds each candidate's ordered score, 0 = not a
// candidate (-inf, or an extension merged into a stay).  LM: the ordered score is that of fl(score + lmacc(prefix)), s_lmx holds lmacc(h + c)
// of the extensions that are candidates, and la.am gets the acoustic totals.
template <bool LM>
__global__ __launch_bounds__(SW_THREADS) void ctc_beam_sweep_kernel(CtcBeamArgs a, CtcLmArgs la, int nbest, int* __restrict__ tokens,
                                                                    int* __restrict__ lens, float* __restrict__ scores) {
    __shared__ float s_pb[2][KMAX], s_pnb[2][KMAX];
    __shared__ int s_last[2][KMAX], s_len[2][KMAX];
    __shared__ unsigned long long s_hash[2][KMAX], s_phash[2][KMAX];
    __shared__ float s_tot[KMAX], s_stay_pb[KMAX], s_stay_pnb[KMAX], s_xl[KMAX];
    __shared__ int s_cls[KMAX], s_win[KMAX];
    __shared__ uint32_t s_sc[KMAX * (KMAX + 1)];
    __shared__ unsigned long long s_wmax[2][SW_WAVES];
    // LM only (unreferenced, hence not allocated, without it)
    __shared__ float s_lmacc[2][KMAX], s_bo[KMAX][LM_MAX_ORDER - 1], s_lmx[KMAX * (KMAX + 1)];
    __shared__ unsigned long long s_ctx[2][KMAX];
    __shared__ int s_has[KMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int K = a.K, P = a.P, P1 = P + 1, Tp = a.Tp;
    const int Tb = clamp_len(a.enc_lens[b], Tp);
    int cur = 0, n = 1;
    if (tid == 0) {
        s_pb[0][0] = 0.f; s_pnb[0][0] = NEG_INF; s_last[0][0] = -1; s_len[0][0] = 0; s_hash[0][0] = HASH_EMPTY; s_phash[0][0] = 0;
        if constexpr (LM) { s_lmacc[0][0] = 0.f; s_ctx[0][0] = 1; }          // the context [sos]: sos = 0 as id + 1
    }
    __syncthreads();
    for (int t = 0; t < Tb; ++t) {
        const long row = (long)b * Tp + t;
        const int nxt = cur ^ 1;
        // the frame's token set, and every entry's not-extended candidate
        if (tid < P) { s_cls[tid] = a.s_cls[row * P + tid]; s_xl[tid] = a.s_lp[row * P + tid]; }
        if (tid < n) {
            const float pb = s_pb[cur][tid], pnb = s_pnb[cur][tid];
            const int last = s_last[cur][tid];
            const float tot = log_add(pb, pnb);
            s_tot[tid] = tot;
            s_stay_pb[tid] = tot + a.xb[row];
            s_stay_pnb[tid] = last < 0 ? NEG_INF : pnb + (a.logits[row * a.ld + last] - a.lse[row]);
            if constexpr (LM) {
                float bo[LM_MAX_ORDER - 1];
                s_has[tid] = ctx_backoffs(la.lm, s_ctx[cur][tid], ctx_len(la.lm, s_len[cur][tid]), bo);
#pragma unroll
                for (int k = 0; k < LM_MAX_ORDER - 1; ++k) s_bo[tid][k] = bo[k];
            }
        }
        __syncthreads();
        const int ncand = n * P1;
        for (int idx = tid; idx < ncand; idx += SW_THREADS) {
            const int k = idx / P1, j = idx % P1 - 1;
            if (j < 0) continue;
            const float v = (s_cls[j] == s_last[cur][k] ? s_pb[cur][k] : s_tot[k]) + s_xl[j];
            s_sc[idx] = v == NEG_INF ? 0u : ord_f32(v);
        }
        __syncthreads();
        // merge: the extension of k that is the beam entry k2 adds to k2's stay (at most one k per k2)
        for (int p = tid; p < n * n; p += SW_THREADS) {
            const int k = p / n, k2 = p % n;
            if (s_len[cur][k2] != s_len[cur][k] + 1 || s_phash[cur][k2] != s_hash[cur][k]) continue;
            const int c = s_last[cur][k2];
            for (int j = 0; j < P; ++j) {
                if (s_cls[j] != c) continue;
                const float v = (c == s_last[cur][k] ? s_pb[cur][k] : s_tot[k]) + s_xl[j];
                s_stay_pnb[k2] = log_add(s_stay_pnb[k2], v);
                s_sc[k * P1 + 1 + j] = 0u;
                break;
            }
        }
        __syncthreads();
        if (tid < n) {
            float v = log_add(s_stay_pb[tid], s_stay_pnb[tid]);
            if constexpr (LM) v = add_rn(v, s_lmacc[cur][tid]);
            s_sc[tid * P1] = v == NEG_INF ? 0u : ord_f32(v);
        }
        if constexpr (LM) {
            // the extensions still standing (finite, not merged: their class is a real one, never the -1 of a NaN row) get their LM term
            for (int idx = tid; idx < ncand; idx += SW_THREADS) {
                const int k = idx / P1, j = idx % P1 - 1;
                if (j < 0 || !s_sc[idx]) continue;
                const int c = s_cls[j];
                if (c < 0) { s_sc[idx] = 0u; continue; }
                float bo[LM_MAX_ORDER - 1];
#pragma unroll
                for (int i = 0; i < LM_MAX_ORDER - 1; ++i) bo[i] = s_bo[k][i];
                const float lmv = lm_score_packed(la.lm, s_ctx[cur][k], ctx_len(la.lm, s_len[cur][k]), bo, s_has[k], c);
                const float acc = add_rn(s_lmacc[cur][k], add_rn(mul_rn(la.lm_w, lmv), la.len_bonus));
                const float v = add_rn((c == s_last[cur][k] ? s_pb[cur][k] : s_tot[k]) + s_xl[j], acc);
                s_lmx[idx] = acc;
                s_sc[idx] = v == NEG_INF ? 0u : ord_f32(v);
            }
        }
        __syncthreads();
        // the K best: arg-max rounds; a thread rescans its own candidates (idx = tid mod 256) only after it gave the winner
        unsigned long long mine = 0;
        for (int idx = tid; idx < ncand; idx += SW_THREADS) {
            const unsigned long long key = ((unsigned long long)s_sc[idx] << 32) | (uint32_t)(0xffffffffu - (uint32_t)idx);
            if (s_sc[idx] && key > mine) mine = key;
        }
        int kept = 0;
        for (int r = 0; r < K; ++r) {
            const unsigned long long wm = wave_max_u64(mine);
            if (lane == 0) s_wmax[r & 1][wave] = wm;
            __syncthreads();
            unsigned long long best = s_wmax[r & 1][0];
#pragma unroll
            for (int w = 1; w < SW_WAVES; ++w) { const unsigned long long v = s_wmax[r & 1][w]; best = v > best ? v : best; }
            if (best == 0) break;                                // uniform: nothing but -inf candidates is left
            const int win = (int)(0xffffffffu - (uint32_t)best);
            if (tid == 0) s_win[r] = win;
            if (win % SW_THREADS == tid) {
                s_sc[win] = 0u;
                mine = 0;
                for (int idx = tid; idx < ncand; idx += SW_THREADS) {
                    const unsigned long long key = ((unsigned long long)s_sc[idx] << 32) | (uint32_t)(0xffffffffu - (uint32_t)idx);
                    if (s_sc[idx] && key > mine) mine = key;
                }
            }
            kept = r + 1;
        }
        __syncthreads();
        // the next beam, in rank order, and its back-pointer records: parent slot | (emitted class + 1) << 8  (0 = stay)
        if (tid < kept) {
            const int win = s_win[tid], k = win / P1, j = win % P1 - 1;
            int rec = k;
            if (j < 0) {
                s_pb[nxt][tid] = s_stay_pb[k]; s_pnb[nxt][tid] = s_stay_pnb[k];
                s_last[nxt][tid] = s_last[cur][k]; s_len[nxt][tid] = s_len[cur][k];
                s_hash[nxt][tid] = s_hash[cur][k]; s_phash[nxt][tid] = s_phash[cur][k];
                if constexpr (LM) { s_lmacc[nxt][tid] = s_lmacc[cur][k]; s_ctx[nxt][tid] = s_ctx[cur][k]; }
            } else {
                const int c = s_cls[j];
                s_pb[nxt][tid] = NEG_INF;
                s_pnb[nxt][tid] = (c == s_last[cur][k] ? s_pb[cur][k] : s_tot[k]) + s_xl[j];
                s_last[nxt][tid] = c; s_len[nxt][tid] = s_len[cur][k] + 1;
                s_hash[nxt][tid] = hash_push(s_hash[cur][k], c); s_phash[nxt][tid] = s_hash[cur][k];
                if constexpr (LM) { s_lmacc[nxt][tid] = s_lmx[win]; s_ctx[nxt][tid] = ctx_push(s_ctx[cur][k], c); }
                rec |= (c + 1) << 8;
            }
            a.rec[row * K + tid] = rec;
        }
        __syncthreads();
        cur = nxt; n = kept;
    }
    // N-best list of the final beam: each live slot walks its records backwards (a prefix of len tokens meets exactly len emitting
    // records on the way); everything behind a list's length is -1
    // LM: final(h) = fl(fl(am + lmacc) + fl(lm_w * lm(eos | h))), and list position i is the entry of rank i by (final descending, beam rank
    // ascending) -- ranked on the ordered bits, so the ranks are a permutation whatever the values
    int* out = tokens + (long)b * nbest * Tp;
    if constexpr (LM) {
        if (tid < n) {
            const unsigned long long ctx = s_ctx[cur][tid];
            const int cn = ctx_len(la.lm, s_len[cur][tid]);
            float bo[LM_MAX_ORDER - 1];
            const int has = ctx_backoffs(la.lm, ctx, cn, bo);
            const float am = log_add(s_pb[cur][tid], s_pnb[cur][tid]);
            const float fin = add_rn(add_rn(am, s_lmacc[cur][tid]), mul_rn(la.lm_w, lm_score_packed(la.lm, ctx, cn, bo, has, a.eos)));
            s_tot[tid] = am; s_xl[tid] = fin; s_sc[tid] = ord_f32(fin);
        }
        __syncthreads();
        if (tid < n) {
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += s_sc[j] > s_sc[tid] || (s_sc[j] == s_sc[tid] && j < tid);
            s_cls[rank] = tid;
        }
        __syncthreads();
    }
    if (tid < nbest) {
        const bool live = tid < n;
        const int src = LM && live ? s_cls[tid] : tid;
        int pos = live ? s_len[cur][src] : 0, slot = src;
        s_win[tid] = pos;
        lens[b * nbest + tid] = live ? pos : -1;
        if constexpr (LM) {
            scores[b * nbest + tid] = live ? s_xl[src] : NEG_INF;
            la.am[b * nbest + tid] = live ? s_tot[src] : NEG_INF;
        } else {
            scores[b * nbest + tid] = live ? log_add(s_pb[cur][tid], s_pnb[cur][tid]) : NEG_INF;
        }
        for (int t = Tb - 1; t >= 0 && pos > 0; --t) {
            const int rec = a.rec[((long)b * Tp + t) * K + slot];
            if (rec >> 8) out[(long)tid * Tp + --pos] = (rec >> 8) - 1;
            slot = rec & 0xff;
        }
    }
    __syncthreads();
    for (long i = tid; i < (long)nbest * Tp; i += SW_THREADS) if ((int)(i % Tp) >= s_win[i / Tp]) out[i] = -1;
}

long align256(long v) { return (v + 255) & ~255l; }
int beam_width(int C, int K, int eos) { const int e = C - 1 - (eos >= 0 ? 1 : 0); return K < e ? K : e; }

}  // namespace

int64_t mk_ctc_beam_work_bytes(int B, int Tp, int C, int K) {
    if (B < 1 || Tp < 1 || C < 2 || C > 4096 || K < 1 || K > 64) { mk_set_error("mk_ctc_beam_work_bytes", "need B >= 1, Tp >= 1, 2 <= C <= 4096, 1 <= K <= 64"); return -1; }
    const long rows = (long)B * Tp, P = K < C - 1 ? K : C - 1;     // (sized for eos = -1, the wider token set)
    return 2 * align256(4 * rows) + 2 * align256(4 * rows * P) + align256(4 * rows * K);
}

// the checks and the two launches of both entry points; la: the LM side, or null
static int ctc_beam_run(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                        void* work, int64_t work_bytes, int* tokens, int* lens, float* scores, const CtcLmArgs* la, hipStream_t s) {
    if (!logits || !enc_lens || !work || !tokens || !lens || !scores) { mk_set_error(fn, "null pointer"); return -1; }
    if (B < 1 || Tp < 1) { mk_set_error(fn, "need B >= 1 and Tp >= 1"); return -1; }
    if (K < 1 || K > 64) { mk_set_error(fn, "beam size K must be in [1, 64]"); return -1; }
    if (nbest < 1 || nbest > K) { mk_set_error(fn, "nbest must be in [1, K]"); return -1; }
    if (C < 2 || C > 4096 || ld < C) { mk_set_error(fn, "need 2 <= C <= 4096 and ld >= C"); return -1; }
    if (blank < 0 || blank >= C) { mk_set_error(fn, "blank must be in [0, C)"); return -1; }
    if (eos < -1 || eos >= C || eos == blank) { mk_set_error(fn, "eos must be -1 or a class in [0, C) other than blank"); return -1; }
    if (la) {
        // the LM's ids are the model's: <s> shares the blank's slot 0 (never emitted), </s> is the last class
        if (blank != 0) { mk_set_error(fn, "blank must be 0 with a language model (class 0 is <s>)"); return -1; }
        if (eos != C - 1) { mk_set_error(fn, "eos must be C - 1 with a language model (the last class is </s>)"); return -1; }
        if (la->lm.C != C) { mk_set_error(fn, "the language model's classes differ from C"); return -1; }
        if (la->lm.order < 1 || la->lm.order > LM_MAX_ORDER) { mk_set_error(fn, "the language model's order must be in [1, 4]"); return -1; }
        if (!(la->lm_w >= 0.f) || !std::isfinite(la->lm_w)) { mk_set_error(fn, "lm_w must be finite and >= 0"); return -1; }
        if (!std::isfinite(la->len_bonus)) { mk_set_error(fn, "len_bonus must be finite"); return -1; }
        if (!la->am) { mk_set_error(fn, "null pointer"); return -1; }
    }
    if (work_bytes < mk_ctc_beam_work_bytes(B, Tp, C, K) || ((uintptr_t)work & 3)) {
        mk_set_error(fn, la ? "work buffer too small (masr_ctc_beam_lm_work_bytes(B, Tp, C, K)) or misaligned"
                            : "work buffer too small (masr_ctc_beam_work_bytes(B, Tp, C, K)) or misaligned");
        return -1;
    }
    CtcBeamArgs a{};
    a.logits = logits; a.ld = ld; a.enc_lens = enc_lens;
    a.B = B; a.Tp = Tp; a.C = C; a.K = K; a.P = beam_width(C, K, eos); a.blank = blank; a.eos = eos;
    const long rows = (long)B * Tp, Pmax = K < C - 1 ? K : C - 1;
    char* w = (char*)work;
    a.lse = (float*)w; w += align256(4 * rows);
    a.xb = (float*)w; w += align256(4 * rows);
    a.s_cls = (int*)w; w += align256(4 * rows * Pmax);
    a.s_lp = (float*)w; w += align256(4 * rows * Pmax);
    a.rec = (int*)w;
    hipLaunchKernelGGL(ctc_beam_frames_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a);
    if (la) hipLaunchKernelGGL(ctc_beam_sweep_kernel<true>, dim3(B), dim3(SW_THREADS), 0, s, a, *la, nbest, tokens, lens, scores);
    else hipLaunchKernelGGL(ctc_beam_sweep_kernel<false>, dim3(B), dim3(SW_THREADS), 0, s, a, CtcLmArgs{}, nbest, tokens, lens, scores);
    return LAUNCH_OK();
}

int mk_ctc_beam_search(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos, void* work,
                       int64_t work_bytes, int* tokens, int* lens, float* scores, hipStream_t s) {
    return ctc_beam_run("mk_ctc_beam_search", logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, nullptr, s);
}

// (the LM state lives in LDS: the work buffer is the plain search's)
int64_t mk_ctc_beam_lm_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_work_bytes(B, Tp, C, K); }

int mk_ctc_beam_search_lm(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const masr_lm* lm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int* tokens, int* lens, float* scores,
                          float* am, hipStream_t s) {
    const char* fn = "mk_ctc_beam_search_lm";
    if (!lm) { mk_set_error(fn, "null language model"); return -1; }
    const CtcLmArgs la{lm->dev, lm_w, len_bonus, am};
    return ctc_beam_run(fn, logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, &la, s);
}
