// Beam-search decoding for MyTransformer (engine.hip: masr_recog_beam).  The decoder step of the greedy decode (decode.hip) runs
// on R = B*K rows, row r = hypothesis r % K of utterance r / K; these kernels are the per-step glue around it.
//
// Per step t (read from the device scalar step[0], so the launch sequence is parameter-identical for every step and is replayed
// as a hipGraph):
//   beam_embed_step   row r: the embedding of its last token + pe[t-1]; its self-attention slot table (key j of row r lives in
//                     cache row tab[r][j]) = its parent's table of the previous step, and tab[r][t-1] = r (the slot this step writes)
//   ... decoder layers + fp32 logits (engine.hip) ...
//   beam_rows         one wave per live row: fp32 log-softmax and the row's K best tokens (logit descending, token ascending).  The one
//                     row stage of every step beam: an n-gram LM (masr_recog_beam_lm) or a row of LSTM-LM logits
//                     (masr_recog_beam_nlm) adds its weighted term and the row is ranked by the fused increment; in the joint
//                     beams it emits the P-long pre-beam for beam_ctc_prefix instead of the K-long list, with either
//                     LM's term in its ranking.  With a phrase list it also advances the row's automaton state and adds the
//                     phrase term to the increment
//   beam_select       one wave per utterance: K-way merge of the K sorted row lists -> the K best candidates (score descending,
//                     parent rank ascending, then the row order above), ended / running bookkeeping, finished flag, step ticket
// beam_backtrace runs once after the last step.
//
// Order of candidates.  Within one parent the score is fl(ps + fl(fl(z - mx) - log s)), a monotone function of the logit z, so the
// row order (z descending, token ascending) is also score order there; a score tie inside one row that the rounding made out of two
// different logits is decided by the logit.  Hence K = 1 picks exactly the greedy arg-max (first maximal logit).
#include "kernels.h"
#include "search.h"
#include "lm.h"
#include "bias.h"
#include <type_traits>

namespace {

__global__ void beam_init_kernel(BeamArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { a.step[0] = 1; a.step[1] = 0; }
    if (i < a.R) a.score[i] = (i % a.K == 0) ? 0.f : NEG_INF;     // at t = 1 only row 0 of each utterance is live
    if (i < a.B) { a.fin[i] = 0; a.best_score[i] = NEG_INF; a.best_len[i] = 0; a.best_row[i] = i * a.K; }
    if (i < a.B * a.N) { a.nb_score[i] = NEG_INF; a.nb_len[i] = -1; a.nb_row[i] = (i / a.N) * a.K; }      // (N <= K: inside the R threads)
}
// one thread: the joint LM beam's weights, read by its step kernels from the device
__global__ void beam_set_weights_kernel(float* w, float att_w, float ctc_w, float lm_w, float len_bonus) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { w[0] = att_w; w[1] = ctc_w; w[2] = lm_w; w[3] = len_bonus; }
}
// one thread: the biased joint beam's fifth weight, behind the four
__global__ void beam_set_bias_w_kernel(float* w, float bias_w) {
    if (blockIdx.x == 0 && threadIdx.x == 0) w[4] = bias_w;
}

// grid R, 256 threads
__global__ __launch_bounds__(256) void beam_embed_step_kernel(BeamArgs a, const float* __restrict__ table, const float* __restrict__ pe,
                                                             float* __restrict__ y32, bf16* __restrict__ y16, int E) {
    const int r = blockIdx.x, st = *a.step;
    int tok = a.sos, par = r;
    if (st > 1) {                                                // (a finished utterance's rows: read in bounds, their results are never used)
        const HistEntry h = hist_entry(a.tok_hist, a.par_hist, a.R, st - 1, r, a.C, a.K, a.sos);
        tok = h.tok; par = h.par;
    }
    for (int e = threadIdx.x; e < E; e += 256) {
        const float v = table[(long)tok * E + e] + pe[(long)(st - 1) * E + e];
        y32[(long)r * E + e] = v;
        y16[(long)r * E + e] = (bf16)v;
    }
    int* cur = a.tab + (long)(st & 1) * a.R * a.Lmax + (long)r * a.Lmax;
    const int* prev = a.tab + (long)((st - 1) & 1) * a.R * a.Lmax + (long)par * a.Lmax;
    for (int j = threadIdx.x; j < st - 1; j += 256) cur[j] = prev[j];
    if (threadIdx.x == 0) cur[st - 1] = r;
}

// ---------------------------------------------------------------- the row stage: a row's logits -> its candidate list
// The LM context of row r's hypothesis (st - 1 tokens), for the whole wave: token s of h is tok_hist[s - 1][row], row = the hypothesis's row
// after step s; position 0 is sos.  Lane 0 walks the histories (hist_entry: clamped) and broadcasts; n <= order - 1, so no order the LM
// lacks is ever indexed
__device__ __forceinline__ LmCtx row_lm_context(const BeamArgs& a, const LmDev& lm, int r, int st, int lane) {
    const int n = min(lm.order - 1, st);
    int tok[LM_MAX_ORDER - 1];
    int row = r;
#pragma unroll
    for (int i = 0; i < LM_MAX_ORDER - 1; ++i) {
        int t = a.sos;
        const int s = st - 1 - i;
        if (lane == 0 && i < n && s >= 1) {
            const HistEntry h = hist_entry(a.tok_hist, a.par_hist, a.R, s, row, a.C, a.K, a.sos);
            t = h.tok; row = h.par;
        }
        tok[i] = __shfl(t, 0, 64);
    }
    return lm_context(lm, tok, n);
}

// Where the LM term of the row stage comes from.  row(..) does the wave's shared work for row r once and returns term(c) = lm(c | h), a
// log-prob <= 0; the lanes call it for their classes (the n-gram's probes of a lane's ceil(C / 64) classes are independent loads)
struct RowLmNone {                                               // no LM: nothing is fused
    static constexpr bool FUSED = false;
    __device__ auto row(const BeamArgs&, int, int, int) const { return [](int) { return 0.f; }; }
};
struct RowLmNgram {                                              // backoff n-gram tables (lm.h): the context from the history walk
    static constexpr bool FUSED = true;
    LmDev lm;
    __device__ auto row(const BeamArgs& a, int r, int st, int lane) const {
        return [&lm = lm, x = row_lm_context(a, lm, r, st, lane)](int c) { return lm_score(lm, x, c); };
    }
};
struct RowLmLogits {                                             // a row of LM logits [R][ld] (the LSTM LM of nlm.hip): its log-softmax
    static constexpr bool FUSED = true;
    const float* y; long ld;
    __device__ auto row(const BeamArgs& a, int r, int, int lane) const {
        const float* yr = y + (long)r * ld;
        return [yr, l = row_lse(yr, a.C, lane)](int c) { return (yr[c] - l.mx) - l.log_s; };
    }
};

// Contextual phrase biasing of the step beams.  A kernel takes what it needs of the list as RowBias, or, where nothing is biased,
// the empty NoBias -- the unbiased instantiations keep the argument list and the code they had.
struct NoBias {};
struct RowBias {
    BiasDev dev;
    int2* state;                                                 // [2][R] (node, credited tokens) of row r's hypothesis, step parity
    float* pre_b;                                                // [R][P] beside pre_lm: b(h, c) of the pre-beam's candidates (joint beam)
    float bias_w;                                                // the top-K's weight (its step graph is keyed on it); the pre-beam reads a.wts[4]
};
template <bool BIAS, class T = RowBias> using bias_arg = std::conditional_t<BIAS, T, NoBias>;

// Once per row: lane 0 takes the state of the row's parent (the other parity; the root at step 1) over the row's last token and stores it in
// this step's parity; the wave gets the node.  A hypothesis of these beams is one token sequence on one path, so its state follows the
// re-parenting as the LSTM LM's does.  A node outside the trie (only a caller of the test entry could set one) reads as the root
__device__ __forceinline__ int row_bias_state(const BeamArgs& a, const RowBias& b, int r, int st, int lane) {
    int u = 0;
    if (lane == 0) {
        int n = 0;
        if (st > 1) {
            const HistEntry h = hist_entry(a.tok_hist, a.par_hist, a.R, st - 1, r, a.C, a.K, a.sos);
            const int2 p = b.state[(long)((st - 1) & 1) * a.R + h.par];
            u = p.x < 0 || p.x >= b.dev.nodes ? 0 : p.x; n = p.y;
            bias_step(b.dev, u, n, h.tok);
        }
        b.state[(long)(st & 1) * a.R + r] = make_int2(u, n);
    }
    return __shfl(u, 0, 64);
}
// dn(h, c) = n' - n of bias_step from node u (rv = revoke[u]) over class c, in [-63, 1]: at most two probes.  ends: the hypothesis h + c ends as
// it is (a token at the last step), so what the new node has not earned is given back as well
__device__ __forceinline__ int row_bias_dn(const BiasDev& d, int u, int rv, int c, bool ends) {
    int v = bias_child(d, u, c), dn = 1;
    if (v < 0) {
        dn = -rv;
        v = u != 0 ? bias_child(d, 0, c) : -1;
        if (v >= 0) dn += 1; else v = 0;
    }
    if (ends) dn -= (int)d.revoke[v];
    return dn;
}

// grid ceil(R / 4), 256 threads: one wave per live row r (hypothesis h of st - 1 tokens, score ps).  lp(c) = (z_c - mx) - log_s of row_lse.
// With an LM the lanes stride over the C classes and store the fused increment f(c) = fl(lp(c) + fl(lm_w * lm(c | h))) -- two roundings,
// the one statement every LM-fused step beam composes it by -- to the row of the fp32 workspace fused [R][ldf]; the same wave reads it back
// (8 KB at C = 2048: it stays in the L1 / L2 of its CU), so the stage is one launch.  row_top_n ranks the row by f, or without an LM by the
// raw logit z (lp would merge logits that the rounding makes equal; the tie order is logit descending), class ascending.
//   top-K (PRE false)   list_tok / list_score [R][K]: the K best classes, eos skipped below minlen, score fl(ps + f(c)) or fl(ps + lp(c)),
//                       token -1 past the end; a dead row gets an empty list.  lm_w is the kernel argument (the step graph is keyed on it)
//   pre-beam (PRE)      pre_tok [R][P]: the P best, blank never, eos skipped below minlen, -1 past the end; then the lanes share the P
//                       entries: pre_lp = lp(c) and, with an LM, pre_lm = fl(lm_w * lm(c | h)), each computed again from its inputs (the
//                       same expressions: the same bits), so no second [R][Cp] row is kept.  A dead row is left alone (the prefix kernel
//                       gives it its empty list).  lm_w is a.wts[2]: no graph holds a weight of the joint LM beam
// BIAS: the row's automaton state is advanced once (row_bias_state), and the increment the row is ranked by becomes
// g(c) = fl(f(c) + b(h, c)), b = fl(bias_w * (float)dn(h, c)), f = lp without an LM -- the fused row is then needed without an LM too, and a
// row without one ranks by lp, not by the logit.  The pre-beam also leaves pre_b = b(h, c), and without an LM pre_lm = +0
template <class Lm, bool PRE, bool BIAS>
__global__ __launch_bounds__(256) void beam_rows_kernel(BeamArgs a, Lm lm, float lm_w_arg, const float* __restrict__ logits, long ld,
                                                       float* __restrict__ fused, long ldf, bias_arg<BIAS> bias) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int u = r / a.K, st = *a.step;
    if (a.fin[u]) return;
    const float ps = a.score[r];
    if (ps == NEG_INF) {                                         // dead row
        if constexpr (!PRE)
            for (int i = lane; i < a.K; i += 64) { a.list_tok[(long)r * a.K + i] = -1; a.list_score[(long)r * a.K + i] = NEG_INF; }
        return;
    }
    const auto term = lm.row(a, r, st, lane);
    const float* z = logits + (long)r * ld;
    const bool no_eos = (st - 1) < a.minlen[u];                  // the hypothesis has st - 1 tokens
    const RowLse l = row_lse(z, a.C, lane);
    auto lp = [&](int c) { return (z[c] - l.mx) - l.log_s; };
    auto skip = [&](int c) { return (PRE && c == 0) || (no_eos && c == a.eos); };
    const float* rank = z;
    float lm_w = 0.f;
    if constexpr (Lm::FUSED) lm_w = PRE ? a.wts[2] : lm_w_arg;
    auto f = [&](int c) { if constexpr (Lm::FUSED) return add_rn(lp(c), mul_rn(lm_w, term(c))); else return lp(c); };
    int bu = 0, brv = 0; float bias_w = 0.f; bool last = false;
    if constexpr (BIAS) {
        bu = row_bias_state(a, bias, r, st, lane);
        brv = (int)bias.dev.revoke[bu];
        bias_w = PRE ? a.wts[4] : bias.bias_w;
        last = st >= a.maxlen[u];
    }
    auto b = [&](int c) {                                        // (BIAS only)
        if constexpr (BIAS) return mul_rn(bias_w, (float)row_bias_dn(bias.dev, bu, brv, c, last && c != a.eos)); else return 0.f;
    };
    if constexpr (Lm::FUSED || BIAS) {
        float* fz = fused + (long)r * ldf;
        for (int c = lane; c < a.C; c += 64) { if constexpr (BIAS) fz[c] = add_rn(f(c), b(c)); else fz[c] = f(c); }
        __threadfence_block();                                   // lane 0 reads below what the other lanes of its wave stored
        rank = fz;
    }
    if constexpr (PRE) {
        int* pt = a.pre_tok + (long)r * a.P;
        row_top_n<false>(rank, a.C, a.P, lane, skip, [&](int i, int c) { pt[i] = c; });
        __threadfence_block();                                   // and the lanes read what lane 0 stored
        for (int i = lane; i < a.P; i += 64) {
            const int c = pt[i];
            const bool ok = c > 0 && c < a.C;
            a.pre_lp[(long)r * a.P + i] = ok ? lp(c) : NEG_INF;
            if constexpr (Lm::FUSED) a.pre_lm[(long)r * a.P + i] = ok ? mul_rn(lm_w, term(c)) : 0.f;
            else if constexpr (BIAS) a.pre_lm[(long)r * a.P + i] = 0.f;
            if constexpr (BIAS) bias.pre_b[(long)r * a.P + i] = ok ? b(c) : 0.f;
        }
    } else {
        int* lt = a.list_tok + (long)r * a.K;
        float* ls = a.list_score + (long)r * a.K;
        row_top_n<false>(rank, a.C, a.K, lane, skip,
                         [&](int i, int c) { lt[i] = c; ls[i] = c < 0 ? NEG_INF : ps + (Lm::FUSED || BIAS ? rank[c] : lp(c)); });
    }
}

// K-way merge of an utterance's K sorted row lists by one wave (lane k = parent rank k): the n <= K best candidates, rank order, into the
// caller's LDS arrays [64]; returns n.  Lane k's head is the best untaken entry of row r0 + k; key = (ordered score, 63 - parent, max - list
// position).  JOINT: the row lists are P long, and a candidate also brings its prefix score and the place of its CTC state
template <bool JOINT>
__device__ __forceinline__ int beam_merge_lists(const BeamArgs& a, int r0, int lane, float* s_score, int* s_tok, int* s_par, float* s_psi, int* s_slot) {
    constexpr int HB = JOINT ? 7 : 6;                            // bits of the list position in the merge key (P <= 96, K <= 64)
    const int K = a.K, W = JOINT ? a.P : K;                      // list length
    int h = 0;
    auto head_key = [&]() -> unsigned long long {
        if (lane >= K || h >= W) return 0ull;
        const float sc = a.list_score[(long)(r0 + lane) * W + h];
        if (a.list_tok[(long)(r0 + lane) * W + h] < 0 || sc == NEG_INF) return 0ull;
        return ((unsigned long long)ord_f32(sc) << 32) | (uint32_t)(((63 - lane) << HB) | ((1 << HB) - 1 - h));
    };
    unsigned long long key = head_key();
    int n = 0;
    for (; n < K; ++n) {
        const unsigned long long top = wave_max_u64(key);
        if (top == 0) break;
        const int k = 63 - (int)((top >> HB) & 63);
        if (lane == k) {
            const long e = (long)(r0 + k) * W + h;
            s_score[n] = a.list_score[e];
            s_tok[n] = a.list_tok[e];
            s_par[n] = r0 + k;
            if constexpr (JOINT) { s_psi[n] = a.list_psi[e]; s_slot[n] = a.list_slot[e]; }
            ++h;
            key = head_key();
        }
    }
    return n;
}

// grid B, 64 threads (one wave).  JOINT (masr_recog_beam_ctc): the row lists are P long, sorted by joint score, and a kept candidate also
// takes its prefix score and the place of its CTC state
// BIAS: a running hypothesis can still gain bias_w per further token, so the stop compares with the bound
// fl(run_best + fl((float)(maxlen - st) * bias_w))
template <bool JOINT, bool BIAS>
__global__ __launch_bounds__(64) void beam_select_kernel(BeamArgs a, bias_arg<BIAS, float> bias_w) {
    __shared__ float s_score[64];
    __shared__ int s_tok[64], s_par[64];
    __shared__ float s_psi[JOINT ? 64 : 1];
    __shared__ int s_slot[JOINT ? 64 : 1];
    const int u = blockIdx.x, lane = threadIdx.x, K = a.K, st = *a.step;
    if (!a.fin[u]) {
        const int r0 = u * K;
        const int n = beam_merge_lists<JOINT>(a, r0, lane, s_score, s_tok, s_par, s_psi, s_slot);
        __syncthreads();
        if (lane == 0) {
            float bs = a.best_score[u]; int bl = a.best_len[u], br = a.best_row[u];
            const int maxlen = a.maxlen[u];
            int j = 0; float run_best = NEG_INF;
            for (int i = 0; i < n; ++i) {                        // rank order: strict '>' keeps the earlier step, then the lower rank
                const float sc = s_score[i];
                if (s_tok[i] == a.eos) {                         // ended: the parent's tokens, without eos
                    if (sc > bs) { bs = sc; bl = st - 1; br = s_par[i]; }
                    continue;
                }
                const int row = r0 + j++;
                a.tok_hist[(long)(st - 1) * a.R + row] = s_tok[i];
                a.par_hist[(long)(st - 1) * a.R + row] = s_par[i];
                a.score[row] = sc;
                if constexpr (JOINT) { a.psi[row] = s_psi[i]; a.src[row] = s_par[i] * a.P + s_slot[i]; }
                if (run_best == NEG_INF) run_best = sc;
                if (st >= maxlen && sc > bs) { bs = sc; bl = st; br = row; }     // the last step: running hypotheses end as they are
            }
            for (int k = j; k < K; ++k) {                        // the beam shrank: dead rows
                a.tok_hist[(long)(st - 1) * a.R + r0 + k] = a.sos;
                a.par_hist[(long)(st - 1) * a.R + r0 + k] = r0 + k;
                a.score[r0 + k] = NEG_INF;
            }
            a.best_score[u] = bs; a.best_len[u] = bl; a.best_row[u] = br;
            // log-probabilities are <= 0: no running hypothesis can overtake an ended one that is at least as good
            if constexpr (BIAS) { if (j == 0 || st >= maxlen || bs >= add_rn(run_best, mul_rn((float)(maxlen - st), bias_w))) a.fin[u] = 1; }
            else if (j == 0 || st >= maxlen || bs >= run_best) a.fin[u] = 1;
        }
    }
    if (lane == 0) step_ticket(a.step, st, a.B);                 // the last utterance to finish advances the step
}

// The joint select with an N-best list and the bound stop rule (masr_recog_beam_ctc_lm).  grid B, 64 threads (one wave).  After
// the merge lane i owns candidate i of the n selected (rank order = score descending): ballots give a running one its row and an ended one
// (eos, or anything at st >= maxlen) its place e among the step's ne ended, which are thereby sorted too.  The list [N] is merged with them
// by rank computation: old entry l moves to l + #{new with a larger score}, new entry e to e + #{old with a score >= its own} -- an old entry
// ended at an earlier step and wins a tie.  Positions >= N fall off; empty slots (len -1) stay the last.
// Stop: nothing runs, st >= maxlen, or the list is full and its N-th score >= fl(run_best + fl((maxlen - st) * max(len_bonus, 0))): every
// other increment is <= 0, so no running hypothesis can still enter the list.  BIAS: the gain per token is at most
// fl(max(len_bonus, 0) + bias_w), bias_w = a.wts[4].
template <bool BIAS>
__global__ __launch_bounds__(64) void beam_select_nbest_kernel(BeamArgs a) {
    __shared__ float s_score[64], s_psi[64];
    __shared__ int s_tok[64], s_par[64], s_slot[64];
    __shared__ float s_es[64], s_os[64], s_ms[64];               // the step's ended / the old list / the merged list: scores
    __shared__ int s_ml[64], s_mr[64];
    const int u = blockIdx.x, lane = threadIdx.x, K = a.K, N = a.N, st = *a.step;
    if (!a.fin[u]) {
        const int r0 = u * K, maxlen = a.maxlen[u];
        const int n = beam_merge_lists<true>(a, r0, lane, s_score, s_tok, s_par, s_psi, s_slot);
        float* nbs = a.nb_score + (long)u * N; int* nbl = a.nb_len + (long)u * N; int* nbr = a.nb_row + (long)u * N;
        const float os = lane < N ? nbs[lane] : NEG_INF;
        const int ol = lane < N ? nbl[lane] : -1, orow = lane < N ? nbr[lane] : r0;
        const bool old_live = ol >= 0;
        s_os[lane] = os;
        __syncthreads();                                         // the merge's LDS stores and the old list
        const bool have = lane < n;
        const float sc = have ? s_score[lane] : NEG_INF;
        const bool is_eos = have && s_tok[lane] == a.eos, runs = have && !is_eos, ends = have && (is_eos || st >= maxlen);
        const unsigned long long below = (1ull << lane) - 1, m_run = __ballot(runs), m_end = __ballot(ends);
        const int j = __popcll(m_run & below), nrun = __popcll(m_run), e = __popcll(m_end & below), ne = __popcll(m_end);
        const int no = __popcll(__ballot(old_live));
        const int row = r0 + j;
        if (runs) {
            a.tok_hist[(long)(st - 1) * a.R + row] = s_tok[lane];
            a.par_hist[(long)(st - 1) * a.R + row] = s_par[lane];
            a.score[row] = sc;
            a.psi[row] = s_psi[lane]; a.src[row] = s_par[lane] * a.P + s_slot[lane];
        }
        if (lane >= nrun && lane < K) {                          // the beam shrank: dead rows
            a.tok_hist[(long)(st - 1) * a.R + r0 + lane] = a.sos;
            a.par_hist[(long)(st - 1) * a.R + r0 + lane] = r0 + lane;
            a.score[r0 + lane] = NEG_INF;
        }
        if (ends) s_es[e] = sc;
        __syncthreads();
        if (old_live) {
            int pos = lane;
            for (int i = 0; i < ne; ++i) pos += s_es[i] > os;
            if (pos < N) { s_ms[pos] = os; s_ml[pos] = ol; s_mr[pos] = orow; }
        }
        if (ends) {
            int pos = e;
            for (int i = 0; i < no; ++i) pos += s_os[i] >= sc;
            // ended by eos: the parent's tokens, without eos; at maxlen a running hypothesis ends as it is
            if (pos < N) { s_ms[pos] = sc; s_ml[pos] = is_eos ? st - 1 : st; s_mr[pos] = is_eos ? s_par[lane] : row; }
        }
        __syncthreads();
        const int total = min(N, no + ne);
        if (lane < total) { nbs[lane] = s_ms[lane]; nbl[lane] = s_ml[lane]; nbr[lane] = s_mr[lane]; }
        if (lane == 0) {
            bool done = nrun == 0 || st >= maxlen;
            if (!done && total == N) {
                const float run_best = s_score[__ffsll((long long)m_run) - 1];      // the first running candidate: the best one
                float gain = fmaxf(a.wts[3], 0.f);
                if constexpr (BIAS) gain = add_rn(gain, a.wts[4]);
                done = s_ms[N - 1] >= add_rn(run_best, mul_rn((float)(maxlen - st), gain));
            }
            if (done) a.fin[u] = 1;
        }
    }
    if (lane == 0) step_ticket(a.step, st, a.B);                 // the last utterance to finish advances the step
}

// ---------------------------------------------------------------- joint CTC/attention decoding (masr_recog_beam_ctc)
// The one-pass CTC prefix score (Watanabe et al. 2017; ESPnet's CTCPrefixScore).  x_t(c) = a.ctc_lp[u][c][t], blank 0, eos C - 1.
// State of hypothesis h at frame t < T_b: (r^n_t, r^b_t).  Extension by c (not blank, not eos), phi_t = logaddexp(r^n_t(h), r^b_t(h)),
// or r^b_t(h) when c is h's last token:
//   r^n_0 = x_0(c) if h is empty else -inf,  r^b_0 = -inf
//   r^n_t = logaddexp(r^n_{t-1}, phi_{t-1}) + x_t(c),  r^b_t = logaddexp(r^n_{t-1}, r^b_{t-1}) + x_t(blank)
//   psi(h+c) = logsumexp(r^n_0, phi_{t-1} + x_t(c) for 1 <= t < T_b);  psi(h+eos) = phi_{T_b-1} (no plain-phi exception)
// Joint score s(h+c) = s(h) + att_w * lp_att(c | h) + ctc_w * (psi(h+c) - psi(h)), fp32 in that order (no contraction).

// grid ceil(B*Tp / 4), 256 threads: one wave per frame row b*Tp + t of the head's fp32 logits -> lp[b][c][t] (frames t < T_b only)
__global__ __launch_bounds__(256) void beam_ctc_logsoftmax_kernel(BeamArgs a, const float* __restrict__ logits, long ld) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.B * a.Tp) return;
    const int b = row / a.Tp, t = row % a.Tp;
    if (t >= a.enc_lens[b]) return;
    const float* z = logits + (long)row * ld;
    const RowLse l = row_lse(z, a.C, lane);
    float* out = const_cast<float*>(a.ctc_lp) + (long)b * a.C * a.Tp + t;
    for (int c = lane; c < a.C; c += 64) out[(long)c * a.Tp] = (z[c] - l.mx) - l.log_s;
}

// grid B, 64 threads, after beam_init_kernel: the empty hypothesis (r^n = -inf, r^b_t = x_0(blank) + ... + x_t(blank), psi 0) in
// parity 0, row u*K, slot 0; every row's psi / src point there
__global__ __launch_bounds__(64) void beam_ctc_init_kernel(BeamArgs a) {
    const int u = blockIdx.x;
    for (int k = threadIdx.x; k < a.K; k += 64) { const int r = u * a.K + k; a.psi[r] = 0.f; a.src[r] = (u * a.K) * a.P; }
    if (threadIdx.x == 0) {
        const float* xb = a.ctc_lp + (long)u * a.C * a.Tp;        // class 0 = blank
        float2* st = a.ctc_state + (long)(u * a.K) * a.Tp * a.P;
        float acc = 0.f;
        for (int t = 0; t < a.enc_lens[u]; ++t) { acc += xb[t]; st[(long)t * a.P] = make_float2(NEG_INF, acc); }
    }
}

// grid R, 128 threads: thread i runs the chain of the row's pre-beam candidate i (i < P <= 96), serial over the T_b frames.  The parent's
// phi_t, r^b_t and x_t(blank) are staged in LDS by chunks of CTC_CH frames (every chain of the row shares them); the candidate's
// (r^n_t, r^b_t) go to ctc_state[st & 1][r][t][i], so a wave's stores at one frame are contiguous.  Then the row's candidates are
// sorted by (joint score descending, pre-beam position ascending) into list_tok / list_score / list_psi / list_slot.
// LM (masr_recog_beam_ctc_lm): the same chains; the score takes the weights from a.wts and adds the pre-beam's weighted LM
// term and, for a token, the length bonus -- five roundings, no multiply-add.  BIAS: the pre-beam's b(h, c) is added as a sixth.
constexpr int CTC_CH = 256;
template <bool LM, bool BIAS>
__global__ __launch_bounds__(128) void beam_ctc_prefix_kernel(BeamArgs a, bias_arg<BIAS, const float*> pre_b) {
    __shared__ float s_phi[CTC_CH], s_rbp[CTC_CH], s_xb[CTC_CH];
    __shared__ unsigned long long s_key[128];
    const int r = blockIdx.x, i = threadIdx.x, u = r / a.K, P = a.P;
    if (a.fin[u]) return;
    const long lo = (long)r * P;
    const float ps = a.score[r];
    if (ps == NEG_INF) {                                         // dead row: an empty list
        if (i < P) { a.list_tok[lo + i] = -1; a.list_score[lo + i] = NEG_INF; }
        return;
    }
    const int st = *a.step, Tb = a.enc_lens[u], sp = a.src[r];
    const int last = st > 1 ? a.tok_hist[(long)(st - 2) * a.R + r] : -1;
    const long plane = (long)a.R * a.Tp * P;
    const float2* prev = a.ctc_state + ((st - 1) & 1) * plane + (long)(sp / P) * a.Tp * P + sp % P;   // parent state, frame t at [t * P]
    float2* cur = a.ctc_state + (st & 1) * plane + (long)r * a.Tp * P + i;
    const float* lp = a.ctc_lp + (long)u * a.C * a.Tp;
    const int c = i < P ? a.pre_tok[lo + i] : -1;
    const bool chain = c > 0 && c != a.eos, rep = c == last;
    const float* xc = lp + (long)(chain ? c : 0) * a.Tp;
    float rn = NEG_INF, rb = NEG_INF, psi = NEG_INF, ph = NEG_INF;       // ph = phi_{t-1} as this candidate sees it
    for (int t0 = 0; t0 < Tb; t0 += CTC_CH) {
        const int n = min(CTC_CH, Tb - t0);
        __syncthreads();                                         // the previous chunk is consumed
        for (int t = i; t < n; t += 128) {
            const float2 v = prev[(long)(t0 + t) * P];
            s_phi[t] = log_add(v.x, v.y); s_rbp[t] = v.y; s_xb[t] = lp[t0 + t];
        }
        __syncthreads();
        if (chain) {
            int t = 0;
            if (t0 == 0) {
                rn = st == 1 ? xc[0] : NEG_INF;                  // (step 1: the parent is the empty hypothesis)
                psi = rn;
                cur[0] = make_float2(rn, rb);
                ph = rep ? s_rbp[0] : s_phi[0];
                t = 1;
            }
            for (; t < n; ++t) {
                const float x = xc[t0 + t];
                const float rn1 = log_add(rn, ph) + x;
                rb = log_add(rn, rb) + s_xb[t];
                psi = log_add(psi, ph + x);
                rn = rn1;
                cur[(long)(t0 + t) * P] = make_float2(rn, rb);
                ph = rep ? s_rbp[t] : s_phi[t];
            }
        }
        if (c == a.eos && t0 + n == Tb) psi = s_phi[n - 1];      // the parent's full CTC log-probability
    }
    unsigned long long key = 0;
    float js = NEG_INF;
    if (c > 0 && psi != NEG_INF) {
        const float d = __fsub_rn(psi, a.psi[r]);
        if constexpr (LM) {
            js = add_rn(add_rn(ps, mul_rn(a.wts[0], a.pre_lp[lo + i])), mul_rn(a.wts[1], d));
            js = add_rn(add_rn(js, a.pre_lm[lo + i]), c == a.eos ? 0.f : a.wts[3]);
            if constexpr (BIAS) js = add_rn(js, pre_b[lo + i]);
        } else {
            js = __fadd_rn(__fadd_rn(ps, __fmul_rn(a.att_w, a.pre_lp[lo + i])), __fmul_rn(a.ctc_w, d));
        }
        if (js != NEG_INF) key = ((unsigned long long)ord_f32(js) << 32) | (uint32_t)(127 - i);
    }
    s_key[i] = key;
    const int nv = __syncthreads_count(key != 0);
    // the nv finite candidates take positions [0, nv) by rank; every position in [nv, P) is padded by its own thread, whatever that
    // thread's candidate was (ranks are < nv: the two kinds of store never meet).  No position keeps a previous step's entry.
    if (key) {
        int rank = 0;
        for (int j = 0; j < P; ++j) rank += s_key[j] > key;
        a.list_tok[lo + rank] = c; a.list_score[lo + rank] = js; a.list_psi[lo + rank] = psi; a.list_slot[lo + rank] = i;
    }
    if (i < P && i >= nv) { a.list_tok[lo + i] = -1; a.list_score[lo + i] = NEG_INF; }
}

// n_final of the n tokens at out: the automaton run forward from the root (one thread)
__device__ __forceinline__ int bias_count(const BiasDev& d, const int* out, int n) {
    int u = 0, cnt = 0;
    for (int i = 0; i < n; ++i) bias_step(d, u, cnt, out[i]);
    return bias_final(d, u, cnt);
}
struct BackBias { BiasDev dev; int* nbias; };

// grid B, 64 threads: tokens [B][Lmax] (-1 past the end), lens [B], scores [B] of the best ended hypothesis; BIAS: nbias [B] = its n_final
template <bool BIAS>
__global__ __launch_bounds__(64) void beam_backtrace_kernel(BeamArgs a, int* __restrict__ tokens, int* __restrict__ lens, float* __restrict__ scores,
                                                            bias_arg<BIAS, BackBias> bb) {
    const int u = blockIdx.x;
    const int n = a.best_len[u];
    int* out = tokens + (long)u * a.Lmax;
    for (int i = threadIdx.x; i < a.Lmax; i += 64) if (i >= n) out[i] = -1;
    if (threadIdx.x == 0) {
        int row = a.best_row[u];
        for (int s = n; s >= 1; --s) {                           // tok_hist[s-1][row] = token s of the hypothesis in row `row` after step s
            out[s - 1] = a.tok_hist[(long)(s - 1) * a.R + row];
            row = a.par_hist[(long)(s - 1) * a.R + row];
        }
        lens[u] = n;
        scores[u] = a.best_score[u];
        if constexpr (BIAS) bb.nbias[u] = bias_count(bb.dev, out, n);
    }
}

// grid B * N, 64 threads: entry n of utterance u -> tokens [B][N][Lmax] (-1 past the end), lens / scores [B][N]; an empty slot: -1, -inf, all -1
// and nothing is walked.  The walk stays inside the Lmax history rows and the utterance's K rows whatever the list holds.  BIAS: nbias [B][N] =
// the entry's n_final, -1 in an empty slot
template <bool BIAS>
__global__ __launch_bounds__(64) void beam_backtrace_nbest_kernel(BeamArgs a, int* __restrict__ tokens, int* __restrict__ lens, float* __restrict__ scores,
                                                                  bias_arg<BIAS, BackBias> bb) {
    const int e = blockIdx.x, u0 = (e / a.N) * a.K;
    const int n = min(a.nb_len[e], a.Lmax);
    int* out = tokens + (long)e * a.Lmax;
    for (int i = threadIdx.x; i < a.Lmax; i += 64) if (i >= n) out[i] = -1;
    if (threadIdx.x == 0) {
        int row = a.nb_row[e];
        for (int s = n; s >= 1; --s) {
            if (row < u0 || row >= u0 + a.K) row = u0;
            out[s - 1] = a.tok_hist[(long)(s - 1) * a.R + row];
            row = a.par_hist[(long)(s - 1) * a.R + row];
        }
        lens[e] = n < 0 ? -1 : n;
        scores[e] = n < 0 ? NEG_INF : a.nb_score[e];
        if constexpr (BIAS) bb.nbias[e] = n < 0 ? -1 : bias_count(bb.dev, out, n);
    }
}

}  // namespace

static int refuse(const char* fn, const char* why) { mk_set_error(fn, why); return -1; }

int mk_beam_init(const BeamArgs& a, hipStream_t s) {
    const int n = a.R > a.B ? a.R : a.B;
    hipLaunchKernelGGL(beam_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
    return LAUNCH_OK();
}
int mk_beam_embed_step(const BeamArgs& a, const float* table, const float* pe, float* y32, bf16* y16, int E, hipStream_t s) {
    hipLaunchKernelGGL(beam_embed_step_kernel, dim3(a.R), dim3(256), 0, s, a, table, pe, y32, y16, E);
    return LAUNCH_OK();
}
template <class Lm, bool PRE>
static int launch_beam_rows(const BeamArgs& a, const Lm& src, const BeamRowLm& lm, const float* logits, long ld, hipStream_t s, const BeamBias* bias) {
    const dim3 grid((a.R + 3) / 4), block(256);
    if constexpr (!std::is_same_v<Lm, RowLmLogits>) if (bias) {     // (the LSTM-LM beams are not biased: no such instantiation)
        const RowBias rb{*bias->dev, bias->state, bias->pre_b, bias->bias_w};
        hipLaunchKernelGGL((beam_rows_kernel<Lm, PRE, true>), grid, block, 0, s, a, src, lm.lm_w, logits, ld, lm.fused, lm.ldf, rb);
        return LAUNCH_OK();
    }
    hipLaunchKernelGGL((beam_rows_kernel<Lm, PRE, false>), grid, block, 0, s, a, src, lm.lm_w, logits, ld, lm.fused, lm.ldf, NoBias{});
    return LAUNCH_OK();
}
// what the biased kernels of a step need beside the list: C, the state and, in the joint beam, the fifth weight and the bias terms
static int check_beam_bias(const char* fn, const BeamArgs& a, const BeamBias* bias) {
    if (!bias) return 0;
    if (!bias->dev || bias->dev->C != a.C || bias->dev->nodes < 1 || !bias->dev->slots || !bias->dev->revoke) return refuse(fn, "need a phrase list over the beam's classes");
    if (!bias->state || !a.maxlen) return refuse(fn, "biasing needs the state buffer and maxlen");
    if (a.P && (!a.N || !a.wts || !a.pre_lm || !bias->pre_b)) return refuse(fn, "the biased pre-beam needs the N-best beam, the weights, the LM terms and the bias terms");
    return 0;
}
int mk_beam_rows(const BeamArgs& a, const BeamRowLm& lm, const float* logits, long ld, hipStream_t s, const BeamBias* bias) {
    const char* fn = "mk_beam_rows";
    if (a.K < 1 || a.K > 64 || a.P < 0 || a.P > 96 || ld < a.C) return refuse(fn, "need 1 <= K <= 64, P <= 96, ld >= C");
    if (check_beam_bias(fn, a, bias)) return -1;
    const bool pre = a.P > 0;
    if (bias && lm.lm_logits) return refuse(fn, "the LSTM-LM beams are not biased");
    if ((bias || lm.ngram || lm.lm_logits) && (!lm.fused || lm.ldf < a.C)) return refuse(fn, "an LM or a phrase list needs the fused workspace, ldf >= C");
    if (!lm.ngram && !lm.lm_logits) {
        const RowLmNone src{};
        return pre ? launch_beam_rows<RowLmNone, true>(a, src, lm, logits, ld, s, bias) : launch_beam_rows<RowLmNone, false>(a, src, lm, logits, ld, s, bias);
    }
    if (lm.ngram && lm.lm_logits) return refuse(fn, "one LM at most");
    const bool pre_ok = !pre || (a.wts && a.pre_lm);
    const char* pre_need = "the fused pre-beam needs the weights and the LM terms";
    if (lm.lm_logits) {
        if (lm.ld_lm < a.C) return refuse(fn, "need ld_lm >= C");
        if (!pre_ok) return refuse(fn, pre_need);
        const RowLmLogits src{lm.lm_logits, lm.ld_lm};
        return pre ? launch_beam_rows<RowLmLogits, true>(a, src, lm, logits, ld, s, nullptr) : launch_beam_rows<RowLmLogits, false>(a, src, lm, logits, ld, s, nullptr);
    }
    if (lm.ngram->order < 1 || lm.ngram->order > LM_MAX_ORDER || lm.ngram->C != a.C) return refuse(fn, "need an LM of order 1 .. 4 over the beam's classes");
    if (!pre_ok) return refuse(fn, pre_need);
    const RowLmNgram src{*lm.ngram};
    return pre ? launch_beam_rows<RowLmNgram, true>(a, src, lm, logits, ld, s, bias) : launch_beam_rows<RowLmNgram, false>(a, src, lm, logits, ld, s, bias);
}
int mk_beam_select(const BeamArgs& a, hipStream_t s, const BeamBias* bias) {
    if (a.K < 1 || a.K > 64) return refuse("mk_beam_select", "beam size must be in [1, 64]");
    if (a.P < 0 || a.P > 96 || (a.N && !a.P)) return refuse("mk_beam_select", "need P <= 96, and the joint beam (P >= 1) for an N-best list");
    if (a.N && (a.N < 1 || a.N > a.K || !a.wts || !a.nb_score || !a.nb_len || !a.nb_row)) return refuse("mk_beam_select", "need 1 <= N <= K, the weights and the list");
    if (bias && a.P && !a.N) return refuse("mk_beam_select", "the biased joint beam is the N-best one");
    if (bias && !a.N) hipLaunchKernelGGL((beam_select_kernel<false, true>), dim3(a.B), dim3(64), 0, s, a, bias->bias_w);
    else if (bias) hipLaunchKernelGGL(beam_select_nbest_kernel<true>, dim3(a.B), dim3(64), 0, s, a);
    else if (a.N) hipLaunchKernelGGL(beam_select_nbest_kernel<false>, dim3(a.B), dim3(64), 0, s, a);
    else if (a.P) hipLaunchKernelGGL((beam_select_kernel<true, false>), dim3(a.B), dim3(64), 0, s, a, NoBias{});
    else hipLaunchKernelGGL((beam_select_kernel<false, false>), dim3(a.B), dim3(64), 0, s, a, NoBias{});
    return LAUNCH_OK();
}
int mk_beam_backtrace(const BeamArgs& a, int* tokens, int* lens, float* scores, hipStream_t s, const BiasDev* bias, int* nbias) {
    if (a.N && (a.N < 1 || a.N > a.K || !a.nb_score || !a.nb_len || !a.nb_row)) return refuse("mk_beam_backtrace", "need 1 <= N <= K and the list");
    if (bias && !nbias) return refuse("mk_beam_backtrace", "null pointer");
    if (bias) {
        const BackBias bb{*bias, nbias};
        if (a.N) hipLaunchKernelGGL(beam_backtrace_nbest_kernel<true>, dim3(a.B * a.N), dim3(64), 0, s, a, tokens, lens, scores, bb);
        else hipLaunchKernelGGL(beam_backtrace_kernel<true>, dim3(a.B), dim3(64), 0, s, a, tokens, lens, scores, bb);
    } else {
        if (a.N) hipLaunchKernelGGL(beam_backtrace_nbest_kernel<false>, dim3(a.B * a.N), dim3(64), 0, s, a, tokens, lens, scores, NoBias{});
        else hipLaunchKernelGGL(beam_backtrace_kernel<false>, dim3(a.B), dim3(64), 0, s, a, tokens, lens, scores, NoBias{});
    }
    return LAUNCH_OK();
}

int mk_beam_ctc_logsoftmax(const BeamArgs& a, const float* logits, long ld, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_logsoftmax_kernel, dim3((a.B * a.Tp + 3) / 4), dim3(256), 0, s, a, logits, ld);
    return LAUNCH_OK();
}
int mk_beam_ctc_init(const BeamArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(beam_ctc_init_kernel, dim3(a.B), dim3(64), 0, s, a);
    return LAUNCH_OK();
}
int mk_beam_ctc_prefix(const BeamArgs& a, hipStream_t s, const float* pre_b) {
    if (a.P < 1 || a.P > 96) return refuse("mk_beam_ctc_prefix", "pre-beam width must be in [1, 96]");
    if (a.N > 0 && (!a.wts || !a.pre_lm)) return refuse("mk_beam_ctc_prefix", "the LM variant needs the weights and the LM terms");
    if (pre_b && !a.N) return refuse("mk_beam_ctc_prefix", "the biased joint beam is the N-best one");
    if (pre_b) hipLaunchKernelGGL((beam_ctc_prefix_kernel<true, true>), dim3(a.R), dim3(128), 0, s, a, pre_b);
    else if (a.N > 0) hipLaunchKernelGGL((beam_ctc_prefix_kernel<true, false>), dim3(a.R), dim3(128), 0, s, a, NoBias{});
    else hipLaunchKernelGGL((beam_ctc_prefix_kernel<false, false>), dim3(a.R), dim3(128), 0, s, a, NoBias{});
    return LAUNCH_OK();
}
int mk_beam_set_weights(const BeamArgs& a, float att_w, float ctc_w, float lm_w, float len_bonus, hipStream_t s) {
    if (!a.wts) return refuse("mk_beam_set_weights", "null pointer");
    hipLaunchKernelGGL(beam_set_weights_kernel, dim3(1), dim3(64), 0, s, const_cast<float*>(a.wts), att_w, ctc_w, lm_w, len_bonus);
    return LAUNCH_OK();
}
int mk_beam_set_bias_weight(const BeamArgs& a, float bias_w, hipStream_t s) {
    if (!a.wts) return refuse("mk_beam_set_bias_weight", "null pointer");
    hipLaunchKernelGGL(beam_set_bias_w_kernel, dim3(1), dim3(64), 0, s, const_cast<float*>(a.wts), bias_w);
    return LAUNCH_OK();
}
