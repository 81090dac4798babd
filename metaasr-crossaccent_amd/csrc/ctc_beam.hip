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
// ctc_beam_sweep<true, false> is the same sweep with a backoff n-gram LM and a per-token bonus fused into the ranking (masr_ctc_beam_search_lm,
// DESIGN 5.6).  p_b and p_nb stay purely acoustic; an entry also carries lmacc(h), the fp32 sum of its tokens' fl(fl(lm_w * lm(c | h)) +
// len_bonus), and its LM context as one 64-bit word: the last <= 3 ids of [sos] + h as id + 1 in 16-bit fields, newest lowest -- the
// order-k key of lm.h is a mask of it, so no record is walked for a context.  A candidate ranks by fl(acoustic score + lmacc(prefix)).
// Per frame: every entry's <= N - 1 context backoffs are looked up once, next to the stay's gathers; after the merge, each surviving
// (entry, class) pair issues its <= N - 1 first probes and the unigram load together and resolves them from the longest order down
// (lm_score's order of additions); a merged pair needs no LM value, its target has one.  The tail adds fl(lm_w * lm(eos | h)) and re-ranks
// the final beam.  ctc_beam_sweep<false, false> compiles to the sweep without any of it.
//
// ctc_beam_sweep<LM, true> adds contextual phrase biasing (masr_ctc_beam_search_bias): each entry carries the state of the phrase
// automaton of bias.h and ranks with fl(bias_w * credited tokens) added; the comment at the kernel has the rest.
//
// masr_ctc_beam_search_nlm is the same search with an LSTM LM's term (nlm.h) in the n-gram's place.  That LM has state, so the
// search runs frame by frame across launches: ctc_beam_frame runs ONE frame of every utterance on the beam kept in the work buffer, the LM's
// carry step advances the B * K rows' states, and ctc_beam_tail writes the lists.
//
// All of it is ONE kernel text, ctc_beam_kernel<M, BIAS, PH>: the frame logic (stay and extension scores, merge, K-best rounds, next beam
// and records) and the tail (final re-rank, record walk, N-best list) are stated once, on separate __shared__ arrays with the frame loop in
// the kernel -- the sweep's form, the fast one.  M is the LM (0 none, 1 the n-gram, 2 the LSTM LM's rows), PH what a launch
// runs of it: ctc_beam_sweep<LM, BIAS> = <LM, BIAS, PH_SWEEP> starts from the empty prefix and runs every frame and the tail; ctc_beam_frame
// = <2, false, PH_FRAME> loads the beam from the work buffer, runs one frame and stores it; ctc_beam_tail = <2, false, PH_TAIL> loads and
// runs the tail.  The modes differ in lm(c | h) alone (one switch in the frame, one in the tail) and in what an entry carries.
//
// The resumable search (masr_ctc_beam_run_*) is two more phases of the plain, n-gram and biased searches: <0|1, BIAS, PH_RANGE>
// loads an utterance's beam and frame cursor from a state block in the work buffer, runs the frames [cursor, min(t_end, enc_len)) and stores
// both back; <0|1, BIAS, PH_TAIL> loads them and runs the tail from the cursor without storing anything, so a result can be read at any
// point and the search goes on.  ctc_beam_frames_kernel takes the frame range its launch covers.
#include <cmath>
#include <type_traits>

#include "kernels.h"
#include "search.h"
#include "host_util.h"
#include "lm.h"
#include "nlm.h"
#include "bias.h"

namespace {

constexpr int SW_THREADS = 256, SW_WAVES = SW_THREADS / 64, KMAX = 64;
constexpr unsigned long long HASH_EMPTY = 0xcbf29ce484222325ull;

__device__ __forceinline__ unsigned long long hash_push(unsigned long long h, int c) {
    h = (h ^ (unsigned long long)(c + 1)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
__device__ __forceinline__ int clamp_len(int n, int Tp) { return n < 0 ? 0 : (n > Tp ? Tp : n); }
__device__ __forceinline__ int clamp_live(int n, int K) { return n < 0 ? 0 : (n > K ? K : n); }

// ---- the LM side of ctc_beam_sweep<true, false>
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

// grid ceil(B*nt / 4), 256 threads: one wave per frame row b*Tp + t of the frames t_from <= t < t_from + nt <= Tp (the whole batch: 0, Tp)
__global__ __launch_bounds__(256) void ctc_beam_frames_kernel(CtcBeamArgs a, int t_from, int nt) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)a.B * nt) return;
    const int b = (int)(r / nt), t = t_from + (int)(r % nt);
    if (t >= clamp_len(a.enc_lens[b], a.Tp)) return;
    const long row = (long)b * a.Tp + t;
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

// ---- the search: ONE kernel text for the five searches.  M: 0 = no LM, 1 = the n-gram (la is a CtcLmArgs), 2 = the LSTM LM, whose rows and
// beam live in the work buffer (la is nlm.h's CtcNlmArgs).  PH: what of the text a launch runs --
//   PH_SWEEP  the empty prefix, all frames 0 .. Tb - 1, the tail                                          (M = 0, 1: one launch per call)
//   PH_FRAME  the beam of parity (st - 1) & 1 from the work buffer, the ONE frame t = st - 2, the beam to parity st & 1 with each kept
//             entry's parent row and token (-1: a stay) for the LM's carry step; with t outside [0, Tb) every live row stays in its own row
//   PH_TAIL   the beam of parity (st - 1) & 1, the tail                                                   (M = 2: st is the device step word)
// grid B, 256 threads.  Candidate index of frame t: parent rank k, then stay (0) or position j in S_t (1 + j): idx = k * (P + 1) + ...,
// so "score descending, index ascending" is the selection order of DESIGN 5.3.  s_sc holds each candidate's ordered score, 0 = not a
// candidate (-inf, or an extension merged into a stay).  LM: the ordered score is that of fl(score + lmacc(prefix)), s_lmx holds lmacc(h + c)
// of the extensions that are candidates, and la.am gets the acoustic totals.
//
// BIAS (masr_ctc_beam_search_bias): an entry also carries the phrase automaton's state (node, credited tokens n) of its prefix
// (bias.h), a function of its tokens alone like lmacc and the context.  A candidate ranks by fl(x + fl(bias_w * n(prefix))), x the ordered
// score above; the term is needed only while a candidate is scored, so no per-candidate array holds the stepped state: the <= K winners step
// again from their parent when the next beam is written.  The tail revokes the unfinished match, final = fl(y + fl(bias_w * n_final)), and
// re-ranks with or without an LM; without one la carries only am.
struct CtcBiasArgs { BiasDev bias; float bias_w; int* nbias; };        // nbias [B][nbest]: n_final, -1 = no entry

// The resumable search (M = 0, 1) keeps its beam in a state block of the work buffer between launches --
//   PH_RANGE  the beam and the frame cursor of the utterance from the state block, the frames [cursor, min(t_end, Tb)), both back.  One
//             parity: the whole beam is in LDS before anything is stored.  The launch's frame statistics cover the rows [t_from, t_end), so
//             an utterance whose cursor is behind t_from (it stopped at a shorter enc_len in an earlier call) runs nothing, whatever its
//             enc_len says now: it stays stopped, and no row is read that no launch wrote
//   PH_TAIL   the beam and the cursor, the tail with its record walk from cursor - 1 down; nothing is stored
// -- and la is then a CtcLmRunArgs: the LM side, the state block and the call's frame range.
// (plain ints, not an unnamed enum: PH == PH_SWEEP below is part of the kernel's mangled name, and an unnamed type is numbered differently in
// the host and the device pass, so the host would look up a symbol the code object does not have)
constexpr int PH_SWEEP = 0, PH_FRAME = 1, PH_TAIL = 2, PH_RANGE = 3;
// the state block, [B][K] each but for the live count and the cursor [B]; lmacc and ctx are read with an LM only, bnode and bn with BIAS only
struct CtcBeamState {
    float *pb, *pnb, *lmacc;
    int *last, *len, *bnode, *bn, *nlive, *cursor;
    unsigned long long *hash, *phash, *ctx;
};
struct CtcLmRunArgs : CtcLmArgs { CtcBeamState st; int t_from, t_end; };
template <int M, int PH> using CtcLmSide = std::conditional_t<M == 2, CtcNlmArgs, std::conditional_t<PH == PH_SWEEP, CtcLmArgs, CtcLmRunArgs>>;

template <int M, bool BIAS, int PH>
__global__ __launch_bounds__(SW_THREADS) void ctc_beam_kernel(CtcBeamArgs a, CtcLmSide<M, PH> la, CtcBiasArgs ba, int nbest, int* __restrict__ tokens,
                                                              int* __restrict__ lens, float* __restrict__ scores) {
    static_assert(M == 2 ? PH == PH_FRAME || PH == PH_TAIL : PH == PH_SWEEP || PH == PH_RANGE || PH == PH_TAIL,
                  "the LSTM LM's search runs frame by frame, the others in one sweep or over frame ranges from the state block");
    constexpr bool RUN = M != 2 && PH != PH_SWEEP;                   // the resumable search: the beam comes from la.st
    static_assert(!(M == 2 && BIAS), "biasing the LSTM LM search needs the automaton's state per entry in the work buffer (DESIGN 5.13): not built");
    constexpr bool LM = M != 0;
    __shared__ float s_pb[2][KMAX], s_pnb[2][KMAX];
    __shared__ int s_last[2][KMAX], s_len[2][KMAX];
    __shared__ unsigned long long s_hash[2][KMAX], s_phash[2][KMAX];
    __shared__ float s_tot[KMAX], s_stay_pb[KMAX], s_stay_pnb[KMAX], s_xl[KMAX];
    __shared__ int s_cls[KMAX], s_win[KMAX];
    __shared__ uint32_t s_sc[KMAX * (KMAX + 1)];
    __shared__ unsigned long long s_wmax[2][SW_WAVES];
    // LM only (unreferenced, hence not allocated, without it)
    __shared__ float s_lmacc[2][KMAX], s_lmx[KMAX * (KMAX + 1)];
    // the n-gram only: an entry's packed context and its backoffs
    __shared__ float s_bo[KMAX][LM_MAX_ORDER - 1];
    __shared__ unsigned long long s_ctx[2][KMAX];
    __shared__ int s_has[KMAX];
    // BIAS only: the automaton's state per entry
    __shared__ int s_bnode[2][KMAX], s_bn[2][KMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int K = a.K, P = a.P, P1 = P + 1, Tp = a.Tp;
    const int Tb = clamp_len(a.enc_lens[b], Tp);
    int cur = 0, n = 1, t0 = 0, t1 = Tb;                             // the beam s_*[cur] of n entries; the frames to run
    // the LM's two weights, and mode 2's step word and log-softmax rows of this utterance's K beam rows (row k at logp + k * ldp)
    float lm_w = 0.f, len_bonus = 0.f;
    int st = 0;
    const float* logp = nullptr;
    if constexpr (M == 1) { lm_w = la.lm_w; len_bonus = la.len_bonus; }
    if constexpr (M == 2) {
        st = *la.step;
        const int par = (st - 1) & 1;
        lm_w = la.wts[0]; len_bonus = la.wts[1];
        logp = la.logp + ((long)par * a.B + b) * K * la.ldp;
        const long o = ((long)par * a.B + b) * K + tid;
        n = clamp_live(la.nlive[par * a.B + b], K);
        if (tid < n) {
            s_pb[0][tid] = la.pb[o]; s_pnb[0][tid] = la.pnb[o]; s_last[0][tid] = la.last[o]; s_len[0][tid] = la.len[o];
            s_hash[0][tid] = la.hash[o]; s_phash[0][tid] = la.phash[o]; s_lmacc[0][tid] = la.lmacc[o];
        }
        t0 = st - 2; t1 = PH == PH_FRAME && t0 >= 0 && t0 < Tb ? t0 + 1 : t0;
    } else if constexpr (RUN) {
        const long o = (long)b * K + tid;
        n = clamp_live(la.st.nlive[b], K);
        if (tid < n) {
            s_pb[0][tid] = la.st.pb[o]; s_pnb[0][tid] = la.st.pnb[o]; s_last[0][tid] = la.st.last[o]; s_len[0][tid] = la.st.len[o];
            s_hash[0][tid] = la.st.hash[o]; s_phash[0][tid] = la.st.phash[o];
            if constexpr (LM) { s_lmacc[0][tid] = la.st.lmacc[o]; s_ctx[0][tid] = la.st.ctx[o]; }
            if constexpr (BIAS) { s_bnode[0][tid] = la.st.bnode[o]; s_bn[0][tid] = la.st.bn[o]; }
        }
        // (an utterance whose length fell below its cursor, or whose cursor is not where this call's rows begin, runs nothing and keeps it)
        t0 = clamp_len(la.st.cursor[b], Tp); t1 = PH == PH_RANGE && t0 == la.t_from ? max(t0, min(la.t_end, Tb)) : t0;
    } else if (tid == 0) {
        s_pb[0][0] = 0.f; s_pnb[0][0] = NEG_INF; s_last[0][0] = -1; s_len[0][0] = 0; s_hash[0][0] = HASH_EMPTY; s_phash[0][0] = 0;
        if constexpr (LM) { s_lmacc[0][0] = 0.f; s_ctx[0][0] = 1; }          // the context [sos]: sos = 0 as id + 1
        if constexpr (BIAS) { s_bnode[0][0] = 0; s_bn[0][0] = 0; }
    }
    __syncthreads();
    // The two helpers take what they read by value and capture nothing (the LDS arrays are static): a capture of cur by reference compiles
    // to other code, with more registers.
    // the score of h + c for entry k of the beam s_*[cur], c = S_t[j]
    auto ext = [](int cur, int c, int k, int j) { return (c == s_last[cur][k] ? s_pb[cur][k] : s_tot[k]) + s_xl[j]; };
    // a thread's best candidate: its key (ordered score, then the smaller index), 0 = none left
    auto scan = [](int tid, int ncand) {
        unsigned long long m = 0;
        for (int idx = tid; idx < ncand; idx += SW_THREADS) {
            const unsigned long long key = ((unsigned long long)s_sc[idx] << 32) | (uint32_t)(0xffffffffu - (uint32_t)idx);
            if (s_sc[idx] && key > m) m = key;
        }
        return m;
    };
    for (int t = t0; PH != PH_TAIL && t < t1; ++t) {
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
            if constexpr (M == 1) {
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
            const float v = ext(cur, s_cls[j], k, j);
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
                const float v = ext(cur, c, k, j);
                s_stay_pnb[k2] = log_add(s_stay_pnb[k2], v);
                s_sc[k * P1 + 1 + j] = 0u;
                break;
            }
        }
        __syncthreads();
        if (tid < n) {
            float v = log_add(s_stay_pb[tid], s_stay_pnb[tid]);
            if constexpr (LM) v = add_rn(v, s_lmacc[cur][tid]);
            if constexpr (BIAS) v = add_rn(v, mul_rn(ba.bias_w, (float)s_bn[cur][tid]));
            s_sc[tid * P1] = v == NEG_INF ? 0u : ord_f32(v);
        }
        if constexpr (LM || BIAS) {
            // the extensions still standing (finite, not merged: their class is a real one, never the -1 of a NaN row) get their LM term
            // and the bias term of the state their token leads to
            for (int idx = tid; idx < ncand; idx += SW_THREADS) {
                const int k = idx / P1, j = idx % P1 - 1;
                if (j < 0 || !s_sc[idx]) continue;
                const int c = s_cls[j];
                if (c < 0) { s_sc[idx] = 0u; continue; }
                float acc = 0.f, bo[LM_MAX_ORDER - 1];         // (bo is declared out here: in a scope of its own the LM sweeps compile to other code)
                if constexpr (LM) {
                    // lm(c | entry k): the n-gram's lookups from the entry's packed context and its backoffs, or the LSTM LM's gather
                    float lmv;
                    if constexpr (M == 1) {
#pragma unroll
                        for (int i = 0; i < LM_MAX_ORDER - 1; ++i) bo[i] = s_bo[k][i];
                        lmv = lm_score_packed(la.lm, s_ctx[cur][k], ctx_len(la.lm, s_len[cur][k]), bo, s_has[k], c);
                    } else {
                        lmv = logp[(long)k * la.ldp + c];
                    }
                    acc = add_rn(s_lmacc[cur][k], add_rn(mul_rn(lm_w, lmv), len_bonus));
                }
                float v = ext(cur, c, k, j);
                if constexpr (LM) v = add_rn(v, acc);
                if constexpr (BIAS) {
                    int u = s_bnode[cur][k], nb = s_bn[cur][k];
                    bias_step(ba.bias, u, nb, c);
                    v = add_rn(v, mul_rn(ba.bias_w, (float)nb));
                }
                if constexpr (LM) s_lmx[idx] = acc;
                s_sc[idx] = v == NEG_INF ? 0u : ord_f32(v);
            }
        }
        __syncthreads();
        // the K best: arg-max rounds; a thread rescans its own candidates (idx = tid mod 256) only after it gave the winner
        unsigned long long mine = scan(tid, ncand);
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
            if (win % SW_THREADS == tid) { s_sc[win] = 0u; mine = scan(tid, ncand); }
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
                if constexpr (LM) s_lmacc[nxt][tid] = s_lmacc[cur][k];
                if constexpr (M == 1) s_ctx[nxt][tid] = s_ctx[cur][k];
                if constexpr (BIAS) { s_bnode[nxt][tid] = s_bnode[cur][k]; s_bn[nxt][tid] = s_bn[cur][k]; }
            } else {
                const int c = s_cls[j];
                s_pb[nxt][tid] = NEG_INF;
                s_pnb[nxt][tid] = ext(cur, c, k, j);
                s_last[nxt][tid] = c; s_len[nxt][tid] = s_len[cur][k] + 1;
                s_hash[nxt][tid] = hash_push(s_hash[cur][k], c); s_phash[nxt][tid] = s_hash[cur][k];
                if constexpr (LM) s_lmacc[nxt][tid] = s_lmx[win];
                if constexpr (M == 1) s_ctx[nxt][tid] = ctx_push(s_ctx[cur][k], c);
                if constexpr (BIAS) {                               // the winner's step again, from its parent: the same bits as when it was scored
                    int u = s_bnode[cur][k], nb = s_bn[cur][k];
                    bias_step(ba.bias, u, nb, c);
                    s_bnode[nxt][tid] = u; s_bn[nxt][tid] = nb;
                }
                rec |= (c + 1) << 8;
            }
            a.rec[row * K + tid] = rec;
        }
        __syncthreads();
        cur = nxt; n = kept;
        if constexpr (PH == PH_FRAME) break;                    // one frame per launch: said here, the compiler drops the loop's registers
    }
    if constexpr (PH == PH_FRAME) {
        // the beam behind the frame to parity st & 1; s_win and s_cls are still the frame's, if one ran
        const long o = ((long)(st & 1) * a.B + b) * K + tid, r0 = (long)b * K;
        if (tid < n) {
            la.pb[o] = s_pb[cur][tid]; la.pnb[o] = s_pnb[cur][tid]; la.last[o] = s_last[cur][tid]; la.len[o] = s_len[cur][tid];
            la.hash[o] = s_hash[cur][tid]; la.phash[o] = s_phash[cur][tid]; la.lmacc[o] = s_lmacc[cur][tid];
            const bool ran = t1 > t0;
            const int j = ran ? s_win[tid] % P1 - 1 : -1;
            la.tok[r0 + tid] = j < 0 ? -1 : s_cls[j];
            la.par[r0 + tid] = (int)r0 + (ran ? s_win[tid] / P1 : tid);
        }
        if (tid == 0) la.nlive[(st & 1) * a.B + b] = n;
        return;
    }
    if constexpr (RUN && PH == PH_RANGE) {
        // the beam behind the range's last frame and the new cursor
        const long o = (long)b * K + tid;
        if (tid < n) {
            la.st.pb[o] = s_pb[cur][tid]; la.st.pnb[o] = s_pnb[cur][tid]; la.st.last[o] = s_last[cur][tid]; la.st.len[o] = s_len[cur][tid];
            la.st.hash[o] = s_hash[cur][tid]; la.st.phash[o] = s_phash[cur][tid];
            if constexpr (LM) { la.st.lmacc[o] = s_lmacc[cur][tid]; la.st.ctx[o] = s_ctx[cur][tid]; }
            if constexpr (BIAS) { la.st.bnode[o] = s_bnode[cur][tid]; la.st.bn[o] = s_bn[cur][tid]; }
        }
        if (tid == 0) { la.st.nlive[b] = n; la.st.cursor[b] = t1; }
        return;
    }
    // N-best list of the final beam (the resumable search's tail: of the beam in front of the cursor): each live slot walks its records
    // backwards (a prefix of len tokens meets exactly len emitting records on the way); everything behind a list's length is -1
    // LM: final(h) = fl(fl(am + lmacc) + fl(lm_w * lm(eos | h))), and list position i is the entry of rank i by (final descending, beam rank
    // ascending) -- ranked on the ordered bits, so the ranks are a permutation whatever the values
    // BIAS: final(h) = fl(y + fl(bias_w * n_final(h))), y the LM's final or, without one, am; s_bn becomes n_final
    int* out = tokens + (long)b * nbest * Tp;
    if constexpr (LM || BIAS) {
        if (tid < n) {
            const float am = log_add(s_pb[cur][tid], s_pnb[cur][tid]);
            float fin = am;
            if constexpr (LM) {
                // lm(eos | entry tid): the frame's switch, the context's backoffs looked up here (the backoffs, the sum, then the lookups:
                // the order the n-gram sweep has always been compiled in)
                unsigned long long ctx = 0;
                int cn = 0, has = 0;
                float bo[LM_MAX_ORDER - 1], lme;
                if constexpr (M == 1) { ctx = s_ctx[cur][tid]; cn = ctx_len(la.lm, s_len[cur][tid]); has = ctx_backoffs(la.lm, ctx, cn, bo); }
                const float y = add_rn(am, s_lmacc[cur][tid]);
                if constexpr (M == 1) lme = lm_score_packed(la.lm, ctx, cn, bo, has, a.eos);
                else lme = logp[(long)tid * la.ldp + a.eos];
                fin = add_rn(y, mul_rn(lm_w, lme));
            }
            if constexpr (BIAS) {
                const int nf = bias_final(ba.bias, s_bnode[cur][tid], s_bn[cur][tid]);
                s_bn[cur][tid] = nf;
                fin = add_rn(fin, mul_rn(ba.bias_w, (float)nf));
            }
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
        const int src = (LM || BIAS) && live ? s_cls[tid] : tid;
        int pos = live ? s_len[cur][src] : 0, slot = src;
        s_win[tid] = pos;
        lens[b * nbest + tid] = live ? pos : -1;
        if constexpr (BIAS) ba.nbias[b * nbest + tid] = live ? s_bn[cur][src] : -1;
        if constexpr (LM || BIAS) {
            scores[b * nbest + tid] = live ? s_xl[src] : NEG_INF;
            la.am[b * nbest + tid] = live ? s_tot[src] : NEG_INF;
        } else {
            scores[b * nbest + tid] = live ? log_add(s_pb[cur][tid], s_pnb[cur][tid]) : NEG_INF;
        }
        for (int t = (RUN ? t0 : Tb) - 1; t >= 0 && pos > 0; --t) {
            const int rec = a.rec[((long)b * Tp + t) * K + slot];
            if (rec >> 8) out[(long)tid * Tp + --pos] = (rec >> 8) - 1;
            slot = rec & 0xff;
        }
    }
    __syncthreads();
    for (long i = tid; i < (long)nbest * Tp; i += SW_THREADS) if ((int)(i % Tp) >= s_win[i / Tp]) out[i] = -1;
}

// ---- the LSTM LM search (masr_ctc_beam_search_nlm): frame-synchronous across launches.  The beam lives in the work buffer by
// parity of the device step word st: the beam in front of frame t = st - 2 stands at parity (st - 1) & 1 -- where the LM's states and
// log-softmax rows of step st - 1 stand (nlm.h) -- and the frame's launch writes the next one to parity st & 1.

// grid B, 256 threads: the initial beam (the empty prefix in row 0 of every utterance) at parity 1, st = 1, the two weights, htop = 0
__global__ __launch_bounds__(SW_THREADS) void ctc_beam_nlm_prepare_kernel(CtcNlmArgs q, int B, int K, float lm_w, float len_bonus, bf16* htop, long htop_n) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        const long o = ((long)B + b) * K;
        q.pb[o] = 0.f; q.pnb[o] = NEG_INF; q.last[o] = -1; q.len[o] = 0; q.hash[o] = HASH_EMPTY; q.phash[o] = 0; q.lmacc[o] = 0.f;
        q.nlive[B + b] = 1; q.nlive[b] = 0;
        if (b == 0) { q.step[0] = 1; q.step[1] = 0; q.wts[0] = lm_w; q.wts[1] = len_bonus; }
    }
    for (long i = (long)b * SW_THREADS + threadIdx.x; i < htop_n; i += (long)gridDim.x * SW_THREADS) htop[i] = (bf16)0.f;
}

// grid B, 256 threads: the resumable search's initial state, the empty prefix in slot 0 of every utterance and the cursor at frame 0
__global__ __launch_bounds__(SW_THREADS) void ctc_beam_run_init_kernel(CtcBeamState q, int K) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        const long o = (long)b * K;
        q.pb[o] = 0.f; q.pnb[o] = NEG_INF; q.last[o] = -1; q.len[o] = 0; q.hash[o] = HASH_EMPTY; q.phash[o] = 0;
        q.lmacc[o] = 0.f; q.ctx[o] = 1;                              // the context [sos]: sos = 0 as id + 1
        q.bnode[o] = 0; q.bn[o] = 0;
        q.nlive[b] = 1; q.cursor[b] = 0;
    }
}

long align256(long v) { return (v + 255) & ~255l; }
int beam_width(int C, int K, int eos) { const int e = C - 1 - (eos >= 0 ? 1 : 0); return K < e ? K : e; }

}  // namespace

int64_t mk_ctc_beam_work_bytes(int B, int Tp, int C, int K) {
    if (B < 1 || Tp < 1 || C < 2 || C > 4096 || K < 1 || K > 64) { mk_set_error("mk_ctc_beam_work_bytes", "need B >= 1, Tp >= 1, 2 <= C <= 4096, 1 <= K <= 64"); return -1; }
    const long rows = (long)B * Tp, P = K < C - 1 ? K : C - 1;     // (sized for eos = -1, the wider token set)
    return 2 * align256(4 * rows) + 2 * align256(4 * rows * P) + align256(4 * rows * K);
}

// the argument checks of the entry points, in two parts: what a search is run on (the resumable search has only this when it opens), and
// where a result goes.  with_lm: an LM is fused (either kind), whose classes are lm_C
static int ctc_beam_check_search(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int blank, int eos,
                                 const void* work, bool with_lm, int lm_C, int lm_order, float lm_w, float len_bonus) {
    if (!logits || !enc_lens || !work) { mk_set_error(fn, "null pointer"); return -1; }
    if (B < 1 || Tp < 1) { mk_set_error(fn, "need B >= 1 and Tp >= 1"); return -1; }
    if (K < 1 || K > 64) { mk_set_error(fn, "beam size K must be in [1, 64]"); return -1; }
    if (C < 2 || C > 4096 || ld < C) { mk_set_error(fn, "need 2 <= C <= 4096 and ld >= C"); return -1; }
    if (blank < 0 || blank >= C) { mk_set_error(fn, "blank must be in [0, C)"); return -1; }
    if (eos < -1 || eos >= C || eos == blank) { mk_set_error(fn, "eos must be -1 or a class in [0, C) other than blank"); return -1; }
    if (with_lm) {
        // the LM's ids are the model's: <s> shares the blank's slot 0 (never emitted), </s> is the last class
        if (blank != 0) { mk_set_error(fn, "blank must be 0 with a language model (class 0 is <s>)"); return -1; }
        if (eos != C - 1) { mk_set_error(fn, "eos must be C - 1 with a language model (the last class is </s>)"); return -1; }
        if (lm_C != C) { mk_set_error(fn, "the language model's classes differ from C"); return -1; }
        if (lm_order < 1 || lm_order > LM_MAX_ORDER) { mk_set_error(fn, "the language model's order must be in [1, 4]"); return -1; }
        if (!(lm_w >= 0.f) || !std::isfinite(lm_w)) { mk_set_error(fn, "lm_w must be finite and >= 0"); return -1; }
        if (!std::isfinite(len_bonus)) { mk_set_error(fn, "len_bonus must be finite"); return -1; }
    }
    return 0;
}
// am: the search writes acoustic totals (an LM or a phrase list is fused); nbias: it writes the credited tokens (a phrase list)
static int ctc_beam_check_result(const char* fn, int K, int nbest, const int* tokens, const int* lens, const float* scores, bool with_am, const float* am,
                                 bool with_nbias, const int* nbias) {
    if (!tokens || !lens || !scores || (with_am && !am) || (with_nbias && !nbias)) { mk_set_error(fn, "null pointer"); return -1; }
    if (nbest < 1 || nbest > K) { mk_set_error(fn, "nbest must be in [1, K]"); return -1; }
    return 0;
}
static int ctc_beam_check(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const void* work, const int* tokens, const int* lens, const float* scores, bool with_lm, int lm_C, int lm_order, float lm_w,
                          float len_bonus, const float* am) {
    CK(ctc_beam_check_search(fn, logits, ld, enc_lens, B, Tp, C, K, blank, eos, work, with_lm, lm_C, lm_order, lm_w, len_bonus));
    return ctc_beam_check_result(fn, K, nbest, tokens, lens, scores, with_lm, am, false, nullptr);
}
// the plain search's arrays, carved from the front of the work buffer
static CtcBeamArgs ctc_beam_carve(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int blank, int eos, void* work) {
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
    return a;
}
// the frame statistics of the rows (b, t_from <= t < t_end) with t < enc_len; rows outside the range are left as they are
static int ctc_beam_frames(const CtcBeamArgs& a, int t_from, int t_end, hipStream_t s) {
    const int nt = t_end - t_from;
    hipLaunchKernelGGL(ctc_beam_frames_kernel, dim3((unsigned)(((long)a.B * nt + 3) / 4)), dim3(256), 0, s, a, t_from, nt);
    return LAUNCH_OK();
}
static int ctc_beam_frames(const CtcBeamArgs& a, hipStream_t s) { return ctc_beam_frames(a, 0, a.Tp, s); }

template <bool LM, bool BIAS>
static void ctc_beam_sweep(const CtcBeamArgs& a, const CtcLmArgs& la, const CtcBiasArgs& ba, int nbest, int* tokens, int* lens, float* scores, hipStream_t s) {
    hipLaunchKernelGGL((ctc_beam_kernel<LM ? 1 : 0, BIAS, PH_SWEEP>), dim3(a.B), dim3(SW_THREADS), 0, s, a, la, ba, nbest, tokens, lens, scores);
}

// the checks of a fused phrase list
static int ctc_bias_check(const char* fn, int C, int blank, int eos, const CtcBiasArgs& ba) {
    // the phrase tokens are the model's classes 1 .. C - 2 whether an LM is fused or not
    if (blank != 0) { mk_set_error(fn, "blank must be 0 with a phrase list (class 0 is no phrase token)"); return -1; }
    if (eos != C - 1) { mk_set_error(fn, "eos must be C - 1 with a phrase list (the last class is no phrase token)"); return -1; }
    if (ba.bias.C != C) { mk_set_error(fn, "the phrase list's classes differ from C"); return -1; }
    if (!(ba.bias_w >= 0.f) || !std::isfinite(ba.bias_w)) { mk_set_error(fn, "bias_w must be finite and >= 0"); return -1; }
    return 0;
}

// the checks and the two launches of the sweep's entry points.  lm / bias: an n-gram LM / a phrase list is fused; without one its struct is
// empty, but for la.am, which the biased search without an LM writes too
static int ctc_beam_run(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                        void* work, int64_t work_bytes, int* tokens, int* lens, float* scores, bool lm, const CtcLmArgs& la, bool bias,
                        const CtcBiasArgs& ba, hipStream_t s) {
    CK(ctc_beam_check(fn, logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, tokens, lens, scores, lm, la.lm.C, la.lm.order, la.lm_w,
                      la.len_bonus, la.am));
    if (bias) {
        CK(ctc_bias_check(fn, C, blank, eos, ba));
        if (!la.am || !ba.nbias) { mk_set_error(fn, "null pointer"); return -1; }
    }
    if (work_bytes < mk_ctc_beam_work_bytes(B, Tp, C, K) || ((uintptr_t)work & 3)) {
        mk_set_error(fn, bias ? "work buffer too small (masr_ctc_beam_bias_work_bytes(B, Tp, C, K)) or misaligned"
                         : lm ? "work buffer too small (masr_ctc_beam_lm_work_bytes(B, Tp, C, K)) or misaligned"
                              : "work buffer too small (masr_ctc_beam_work_bytes(B, Tp, C, K)) or misaligned");
        return -1;
    }
    const CtcBeamArgs a = ctc_beam_carve(logits, ld, enc_lens, B, Tp, C, K, blank, eos, work);
    CK(ctc_beam_frames(a, s));
    static constexpr decltype(&ctc_beam_sweep<false, false>) sweep[2][2] = {{ctc_beam_sweep<false, false>, ctc_beam_sweep<false, true>},
                                                                            {ctc_beam_sweep<true, false>, ctc_beam_sweep<true, true>}};
    sweep[lm][bias](a, la, ba, nbest, tokens, lens, scores, s);
    return LAUNCH_OK();
}

int mk_ctc_beam_search(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos, void* work,
                       int64_t work_bytes, int* tokens, int* lens, float* scores, hipStream_t s) {
    return ctc_beam_run("mk_ctc_beam_search", logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, false,
                        CtcLmArgs{}, false, CtcBiasArgs{}, s);
}

// (the LM state lives in LDS: the work buffer is the plain search's)
int64_t mk_ctc_beam_lm_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_work_bytes(B, Tp, C, K); }

int mk_ctc_beam_search_lm(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const masr_lm* lm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int* tokens, int* lens, float* scores,
                          float* am, hipStream_t s) {
    const char* fn = "mk_ctc_beam_search_lm";
    if (!lm) { mk_set_error(fn, "null language model"); return -1; }
    return ctc_beam_run(fn, logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, true,
                        CtcLmArgs{lm->dev, lm_w, len_bonus, am}, false, CtcBiasArgs{}, s);
}

// (the automaton's state lives in LDS too)
int64_t mk_ctc_beam_bias_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_work_bytes(B, Tp, C, K); }

int mk_ctc_beam_search_bias(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                            const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work, int64_t work_bytes,
                            int* tokens, int* lens, float* scores, float* am, int* nbias, hipStream_t s) {
    const char* fn = "mk_ctc_beam_search_bias";
    if (!bias) { mk_set_error(fn, "null phrase list"); return -1; }
    return ctc_beam_run(fn, logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, lm != nullptr,
                        lm ? CtcLmArgs{lm->dev, lm_w, len_bonus, am} : CtcLmArgs{LmDev{}, 0.f, 0.f, am}, true, CtcBiasArgs{bias->dev, bias_w, nbias}, s);
}

// ---------------------------------------------------------------- the resumable search
// A host-only run object over a caller's work buffer: the plain search's arrays, then the state block (CtcBeamState: every array rounded up
// to 256 bytes, planned with or without an LM or a phrase list).  It owns no GPU memory.
struct masr_ctc_beam_run {
    CtcBeamArgs a; CtcLmArgs la; CtcBiasArgs ba; CtcBeamState st;
    bool lm, bias;
    int t_done;                                                     // the frames [0, t_done) have run
};
namespace {
int64_t ctc_beam_state_carve(char* w, int B, int K, CtcBeamState* st) {
    const int64_t R = (int64_t)B * K;
    int64_t off = 0;
    auto take = [&](auto*& p, int64_t n) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>((uintptr_t)w + (uintptr_t)off);
        off += align256((long)(sizeof(*p) * n));
    };
    CtcBeamState q{};
    take(q.hash, R); take(q.phash, R); take(q.ctx, R);
    take(q.pb, R); take(q.pnb, R); take(q.lmacc, R); take(q.last, R); take(q.len, R); take(q.bnode, R); take(q.bn, R);
    take(q.nlive, B); take(q.cursor, B);
    if (st) *st = q;
    return off;
}
template <int M, bool BIAS, int PH>
void ctc_beam_run_launch(const masr_ctc_beam_run& r, const CtcLmArgs& la, const CtcBiasArgs& ba, int t_end, int nbest, int* tokens, int* lens,
                         float* scores, hipStream_t s) {
    hipLaunchKernelGGL((ctc_beam_kernel<M, BIAS, PH>), dim3(r.a.B), dim3(SW_THREADS), 0, s, r.a, CtcLmRunArgs{la, r.st, r.t_done, t_end}, ba, nbest,
                       tokens, lens, scores);
}
using CtcRunLaunch = decltype(&ctc_beam_run_launch<0, false, PH_RANGE>);
}  // namespace

int64_t mk_ctc_beam_run_work_bytes(int B, int Tp, int C, int K) {
    const int64_t base = mk_ctc_beam_work_bytes(B, Tp, C, K);
    return base < 0 ? -1 : base + ctc_beam_state_carve(nullptr, B, K, nullptr);
}

masr_ctc_beam_run* mk_ctc_beam_run_open(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int blank, int eos,
                                        const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work,
                                        int64_t work_bytes, hipStream_t s) {
    const CtcLmArgs la = lm ? CtcLmArgs{lm->dev, lm_w, len_bonus, nullptr} : CtcLmArgs{};
    const CtcBiasArgs ba = bias ? CtcBiasArgs{bias->dev, bias_w, nullptr} : CtcBiasArgs{};
    if (ctc_beam_check_search(fn, logits, ld, enc_lens, B, Tp, C, K, blank, eos, work, lm != nullptr, la.lm.C, la.lm.order, lm_w, len_bonus) != 0)
        return nullptr;
    if (bias && ctc_bias_check(fn, C, blank, eos, ba) != 0) return nullptr;
    if (work_bytes < mk_ctc_beam_run_work_bytes(B, Tp, C, K) || ((uintptr_t)work & 7)) {
        mk_set_error(fn, "work buffer too small (masr_ctc_beam_run_work_bytes(B, Tp, C, K)) or misaligned");
        return nullptr;
    }
    masr_ctc_beam_run* r = new masr_ctc_beam_run{};
    r->a = ctc_beam_carve(logits, ld, enc_lens, B, Tp, C, K, blank, eos, work);
    r->la = la; r->ba = ba; r->lm = lm != nullptr; r->bias = bias != nullptr; r->t_done = 0;
    ctc_beam_state_carve((char*)work + mk_ctc_beam_work_bytes(B, Tp, C, K), B, K, &r->st);
    hipLaunchKernelGGL(ctc_beam_run_init_kernel, dim3(B), dim3(SW_THREADS), 0, s, r->st, K);
    if (LAUNCH_OK() != 0) { delete r; return nullptr; }
    return r;
}

int mk_ctc_beam_run_advance(const char* fn, masr_ctc_beam_run* r, int t_end, hipStream_t s) {
    if (!r) { mk_set_error(fn, "null run"); return -1; }
    if (t_end < r->t_done || t_end > r->a.Tp) { mk_set_error(fn, "t_end must lie in [the frames already run, Tp]"); return -1; }
    if (t_end == r->t_done) return 0;
    CK(ctc_beam_frames(r->a, r->t_done, t_end, s));
    static constexpr CtcRunLaunch range[2][2] = {{ctc_beam_run_launch<0, false, PH_RANGE>, ctc_beam_run_launch<0, true, PH_RANGE>},
                                                 {ctc_beam_run_launch<1, false, PH_RANGE>, ctc_beam_run_launch<1, true, PH_RANGE>}};
    range[r->lm][r->bias](*r, r->la, r->ba, t_end, 0, nullptr, nullptr, nullptr, s);
    CK(LAUNCH_OK());
    r->t_done = t_end;
    return 0;
}

int mk_ctc_beam_run_result(const char* fn, const masr_ctc_beam_run* r, int nbest, int* tokens, int* lens, float* scores, float* am, int* nbias,
                           hipStream_t s) {
    if (!r) { mk_set_error(fn, "null run"); return -1; }
    CK(ctc_beam_check_result(fn, r->a.K, nbest, tokens, lens, scores, r->lm || r->bias, am, r->bias, nbias));
    CtcLmArgs la = r->la; la.am = am;
    CtcBiasArgs ba = r->ba; ba.nbias = nbias;
    static constexpr CtcRunLaunch tail[2][2] = {{ctc_beam_run_launch<0, false, PH_TAIL>, ctc_beam_run_launch<0, true, PH_TAIL>},
                                                {ctc_beam_run_launch<1, false, PH_TAIL>, ctc_beam_run_launch<1, true, PH_TAIL>}};
    tail[r->lm][r->bias](*r, la, ba, 0, nbest, tokens, lens, scores, s);
    return LAUNCH_OK();
}

void mk_ctc_beam_run_close(masr_ctc_beam_run* r) { delete r; }

// ---------------------------------------------------------------- the LSTM LM search
// the work buffer: the plain search's arrays | step [2] | the two weights | the beam by parity [2][B][K]: p_b, p_nb, lmacc, last, len, hash,
// parent hash | live counts [2][B] | token and parent row of the frame [R] each | the LM's h, c [2][L][R][Hp], top h [R][Hp], logits [R][Cp],
// log-softmax rows [2][R][Cp]; R = B * K, Cp = C padded to 128, every entry rounded up to 256 bytes
namespace {
struct CtcNlmPlan { int64_t step, wts, pb, pnb, lmacc, last, len, hash, phash, nlive, tok, par, h, c, htop, logits, logp, total; long ldl; };
CtcNlmPlan ctc_nlm_plan(const NlmDev& d, int B, int Tp, int C, int K) {
    CtcNlmPlan p{};
    const int64_t R = (int64_t)B * K;
    p.ldl = (C + 127) / 128 * 128;
    int64_t off = mk_ctc_beam_work_bytes(B, Tp, C, K);
    auto take = [&](int64_t bytes) { const int64_t o = off; off += align256(bytes); return o; };
    p.step = take(8); p.wts = take(8);
    p.pb = take(8 * R); p.pnb = take(8 * R); p.lmacc = take(8 * R); p.last = take(8 * R); p.len = take(8 * R);
    p.hash = take(16 * R); p.phash = take(16 * R);
    p.nlive = take(8 * (int64_t)B); p.tok = take(4 * R); p.par = take(4 * R);
    p.h = take(nlm_state_elems(d, (int)R) * 2); p.c = take(nlm_state_elems(d, (int)R) * 4); p.htop = take(R * d.Hp * 2);
    p.logits = take(R * p.ldl * 4); p.logp = take(2 * R * p.ldl * 4);
    p.total = off;
    return p;
}
}  // namespace

int64_t mk_ctc_beam_nlm_work_bytes(const masr_nlm* nlm, int B, int Tp, int C, int K) {
    const char* fn = "mk_ctc_beam_nlm_work_bytes";
    if (!nlm) { mk_set_error(fn, "null language model"); return -1; }
    if (mk_ctc_beam_work_bytes(B, Tp, C, K) < 0) return -1;
    return ctc_nlm_plan(nlm->dev, B, Tp, C, K).total;
}

int mk_ctc_beam_nlm_begin(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, const int* tokens, const int* lens,
                          const float* scores, float* am, CtcNlmRun* run, hipStream_t s) {
    if (!nlm) { mk_set_error(fn, "null language model"); return -1; }
    CK(ctc_beam_check(fn, logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, tokens, lens, scores, true, nlm->dev.C, 1, lm_w, len_bonus, am));
    const NlmDev& d = nlm->dev;
    const CtcNlmPlan p = ctc_nlm_plan(d, B, Tp, C, K);
    if (work_bytes < p.total || ((uintptr_t)work & 255)) {
        mk_set_error(fn, "work buffer too small (masr_ctc_beam_nlm_work_bytes(nlm, B, Tp, C, K)) or misaligned");
        return -1;
    }
    CtcNlmRun& r = *run;
    r = CtcNlmRun{};
    r.a = ctc_beam_carve(logits, ld, enc_lens, B, Tp, C, K, blank, eos, work);
    char* w = (char*)work;
    CtcNlmArgs& q = r.q;
    q.step = (int*)(w + p.step); q.wts = (float*)(w + p.wts);
    q.pb = (float*)(w + p.pb); q.pnb = (float*)(w + p.pnb); q.lmacc = (float*)(w + p.lmacc); q.last = (int*)(w + p.last); q.len = (int*)(w + p.len);
    q.hash = (unsigned long long*)(w + p.hash); q.phash = (unsigned long long*)(w + p.phash);
    q.nlive = (int*)(w + p.nlive); q.tok = (int*)(w + p.tok); q.par = (int*)(w + p.par);
    q.logp = (float*)(w + p.logp); q.ldp = p.ldl; q.am = am;
    r.lm = d; r.logits = (float*)(w + p.logits); r.ldl = p.ldl;
    NlmStepArgs& st = r.st;
    st.step = q.step; st.R = B * K; st.K = K; st.tok_hist = q.tok; st.par_hist = q.par; st.hist_stride = 0; st.live = q.nlive;
    st.hstate = (bf16*)(w + p.h); st.cstate = (float*)(w + p.c); st.htop = (bf16*)(w + p.htop);
    CK(ctc_beam_frames(r.a, s));
    hipLaunchKernelGGL(ctc_beam_nlm_prepare_kernel, dim3(B), dim3(SW_THREADS), 0, s, q, B, K, lm_w, len_bonus, st.htop, (long)st.R * d.Hp);
    CK(LAUNCH_OK());
    return mk_nlm_step_carry(d, st, r.logits, r.ldl, q.logp, q.ldp, q.step, s);          // LM step 1: [start] from the zero state
}
int mk_ctc_beam_nlm_frame(const CtcNlmRun& r, hipStream_t s) {
    hipLaunchKernelGGL((ctc_beam_kernel<2, false, PH_FRAME>), dim3(r.a.B), dim3(SW_THREADS), 0, s, r.a, r.q, CtcBiasArgs{}, 0, nullptr, nullptr, nullptr);
    CK(LAUNCH_OK());
    return mk_nlm_step_carry(r.lm, r.st, r.logits, r.ldl, r.q.logp, r.q.ldp, r.q.step, s);
}
int mk_ctc_beam_nlm_end(const CtcNlmRun& r, int nbest, int* tokens, int* lens, float* scores, hipStream_t s) {
    hipLaunchKernelGGL((ctc_beam_kernel<2, false, PH_TAIL>), dim3(r.a.B), dim3(SW_THREADS), 0, s, r.a, r.q, CtcBiasArgs{}, nbest, tokens, lens, scores);
    return LAUNCH_OK();
}

int mk_ctc_beam_search_nlm(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                           const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int* tokens, int* lens, float* scores,
                           float* am, hipStream_t s) {
    CtcNlmRun r;
    CK(mk_ctc_beam_nlm_begin("mk_ctc_beam_search_nlm", logits, ld, enc_lens, B, Tp, C, K, nbest, blank, eos, nlm, lm_w, len_bonus, work, work_bytes,
                             tokens, lens, scores, am, &r, s));
    for (int t = 0; t < Tp; ++t) CK(mk_ctc_beam_nlm_frame(r, s));
    return mk_ctc_beam_nlm_end(r, nbest, tokens, lens, scores, s);
}
