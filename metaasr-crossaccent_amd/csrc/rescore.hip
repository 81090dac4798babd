// Attention rescoring of an N-best list (masr_rescore_nbest / masr_recog_rescore): what surrounds the one teacher-forced
// decoder pass over all R = B*N hypotheses.
//
//   rescore_prepare   the lists -> the decoder's input [R][L] ([sos, h.., eos padding]) and gold [R][L] ([h.., eos, -1 padding]); an entry the
//                     first pass did not fill (lens < 0) becomes all-eos input and all -1 gold
//   rescore_score     one workgroup per hypothesis, one wave per decoder row: log_softmax(z)[gold] = z[gold] - (max + log sum exp(z - max)) in
//                     fp32 (search.h row_lse), then att = the rows' sum, position ascending, by one lane: the result depends on nothing but the
//                     hypothesis's own rows
//   rescore_select    one workgroup per utterance: score = att_w att + ctc_w ctc, the stable rank of each of the <= 64 entries (score
//                     descending, first-pass rank ascending, unfilled entries last), and the reordered copies
#include "kernels.h"
#include "search.h"

namespace {

constexpr int NMAX = 64;

__global__ __launch_bounds__(256) void rescore_prepare_kernel(const int* __restrict__ tok, long ld_tok, const int* __restrict__ lens, int R, int L,
                                                              int sos, int eos, int* __restrict__ tok_in, int* __restrict__ gold) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)R * L) return;
    const int r = (int)(i / L), l = (int)(i % L);
    int n = lens[r];
    if (n > L - 1) n = L - 1;                                // (the host vetted it: 1 + the longest live list is L)
    if (n < 0) { tok_in[i] = eos; gold[i] = -1; return; }
    const int* h = tok + (long)r * ld_tok;
    tok_in[i] = l == 0 ? sos : (l <= n ? h[l - 1] : eos);
    gold[i] = l < n ? h[l] : (l == n ? eos : -1);
}

// grid R, 256 threads.  row_lp [R*L]: each row's term (0 where gold < 0)
__global__ __launch_bounds__(256) void rescore_score_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ gold, int L, int C,
                                                            float* row_lp, float* __restrict__ att) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x;
    for (int l = wave; l < L; l += 4) {
        const long row = (long)r * L + l;
        const int g = gold[row];
        float v = 0.f;
        if (g >= 0 && g < C) {                               // (wave-uniform)
            const float* z = logits + row * ld;
            const RowLse s = row_lse(z, C, lane);
            v = z[g] - (s.mx + s.log_s);
        }
        if (lane == 0) row_lp[row] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        int live = 0;
        for (int l = 0; l < L; ++l) {
            const long row = (long)r * L + l;
            if (gold[row] < 0) continue;
            sum += row_lp[row]; live = 1;
        }
        att[r] = live ? sum : NEG_INF;
    }
}

struct SelectArgs {
    const int* tok_in; long ld_tok; const int* lens_in; const float* ctc_in; const float* att_in;
    int N; float att_w, ctc_w;
    int* tokens; int* lens; float* scores; float* att; float* ctc; int* order;
};

// grid B, 256 threads
__global__ __launch_bounds__(256) void rescore_select_kernel(SelectArgs a) {
    __shared__ float s_score[NMAX];
    __shared__ int s_live[NMAX], s_src[NMAX];
    const int tid = threadIdx.x, b = blockIdx.x, N = a.N;
    const long base = (long)b * N;
    if (tid < N) {
        const int live = a.lens_in[base + tid] >= 0;
        float sc = NEG_INF;
        if (live) {
            sc = __fmul_rn(a.att_w, a.att_in[base + tid]);
            if (a.ctc_w != 0.f) sc = __fadd_rn(sc, __fmul_rn(a.ctc_w, a.ctc_in[base + tid]));
        }
        s_score[tid] = sc; s_live[tid] = live; s_src[tid] = tid;
    }
    __syncthreads();
    if (tid < N) {
        const float sc = s_score[tid]; const int live = s_live[tid];
        int rank = 0;
        for (int m = 0; m < N; ++m) {
            if (m == tid) continue;
            const float sm = s_score[m]; const int lm = s_live[m];
            bool before;
            if (lm != live) before = lm > live;
            else if (live && sm > sc) before = true;
            else if (live && sc > sm) before = false;
            else before = m < tid;
            rank += before;
        }
        s_src[rank] = tid;                                   // (a total order: every rank in [0, N) is taken once; NaN scores may collide -- a slot then keeps its own index)
    }
    __syncthreads();
    if (tid < N) {
        const int n = s_src[tid], live = s_live[n];
        a.order[base + tid] = n;
        a.lens[base + tid] = live ? a.lens_in[base + n] : -1;
        a.scores[base + tid] = s_score[n];
        a.att[base + tid] = live ? a.att_in[base + n] : NEG_INF;
        a.ctc[base + tid] = a.ctc_in[base + n];
    }
    const long per = (long)N * a.ld_tok;
    for (long i = tid; i < per; i += 256) {
        const int j = (int)(i / a.ld_tok);
        a.tokens[base * a.ld_tok + i] = a.tok_in[(base + s_src[j]) * a.ld_tok + (i % a.ld_tok)];
    }
}

}  // namespace

int mk_rescore_prepare(const int* tok, long ld_tok, const int* lens, int R, int L, int sos, int eos, int* tok_in, int* gold, hipStream_t s) {
    if (R < 1 || L < 1 || ld_tok < 0) { mk_set_error("mk_rescore_prepare", "need R >= 1, L >= 1, ld_tok >= 0"); return -1; }
    const long n = (long)R * L;
    hipLaunchKernelGGL(rescore_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tok, ld_tok, lens, R, L, sos, eos, tok_in, gold);
    return LAUNCH_OK();
}
int mk_rescore_score(const float* logits, long ld, const int* gold, int R, int L, int C, float* row_lp, float* att, hipStream_t s) {
    if (R < 1 || L < 1 || C < 1 || ld < C) { mk_set_error("mk_rescore_score", "need R >= 1, L >= 1, 1 <= C <= ld"); return -1; }
    hipLaunchKernelGGL(rescore_score_kernel, dim3(R), dim3(256), 0, s, logits, ld, gold, L, C, row_lp, att);
    return LAUNCH_OK();
}
int mk_rescore_select(const int* tok_in, long ld_tok, const int* lens_in, const float* ctc_in, const float* att_in, int B, int N, float att_w,
                      float ctc_w, int* tokens, int* lens, float* scores, float* att, float* ctc, int* order, hipStream_t s) {
    if (B < 1 || N < 1 || N > NMAX || ld_tok < 0) { mk_set_error("mk_rescore_select", "need B >= 1, 1 <= N <= 64, ld_tok >= 0"); return -1; }
    SelectArgs a{tok_in, ld_tok, lens_in, ctc_in, att_in, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order};
    hipLaunchKernelGGL(rescore_select_kernel, dim3(B), dim3(256), 0, s, a);
    return LAUNCH_OK();
}
