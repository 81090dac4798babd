// libmasr: the standalone kernel entry points of include/masr_test.h (parity tests, probes).  Each fills a launcher's argument
// struct from plain pointers and calls it; none touches a masr_model.
#include <algorithm>
#include <vector>

#include "../../include/masr_test.h"
#include "kernels.h"
#include "host_util.h"
#include "lm.h"
#include "nlm.h"
#include "bias.h"

extern "C" {

int masr_test_gemm(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, int reduction_major, const float* bias,
                   int relu, float* C32, int64_t ldc, void* stream) {
    GemmArgs g = gemm_args();
    g.A = (const bf16*)A; g.lda = lda; g.B = (const bf16*)B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.reduction_major = reduction_major;
    g.bias = bias; g.relu = relu; g.C32 = C32; g.ldc = ldc;
    return mk_gemm(g, (hipStream_t)stream);
}
int masr_test_dropout_mask(uint32_t seed, uint32_t site, int64_t n, float p, float* out, void* stream) {
    return mk_dropout_mask(out, n, p, seed, site, (hipStream_t)stream);
}
int masr_test_gemm_dropout(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, float drop_p, uint32_t seed,
                           uint32_t site, float* C32, int64_t ldc, void* stream) {
    GemmArgs g = gemm_args();
    g.A = (const bf16*)A; g.lda = lda; g.B = (const bf16*)B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.drop_p = drop_p; g.seed = seed; g.site = site; g.C32 = C32; g.ldc = ldc;
    return mk_gemm(g, (hipStream_t)stream);
}
int masr_test_attention_dropout(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, float* lse, int B, int H, int Tq, int Tk,
                                int hd, float drop_p, uint32_t seed, uint32_t site, void* stream) {
    const long E = (long)H * hd;
    AttnArgs a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ldq = a.ldk = a.ldv = E; a.o = (bf16*)o; a.ldo = E; a.lse = lse;
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.drop_p = drop_p; a.seed = seed; a.site = site;
    return mk_attn_fwd(a, (hipStream_t)stream);
}
int masr_test_gemm_epi(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, const float* bias, int relu,
                       float drop_p, const float* residual, const uint16_t* mask, float* C32, uint16_t* C16, void* stream) {
    GemmArgs g = gemm_args();
    g.A = (const bf16*)A; g.lda = lda; g.B = (const bf16*)B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu = relu;
    g.drop_p = drop_p; g.seed = 1; g.site = 2; g.residual = residual; g.ldres = N; g.mask = (const bf16*)mask; g.ldmask = N;
    g.C32 = C32; g.ldc = N; g.C16 = (bf16*)C16; g.ldc16 = N;
    return mk_gemm(g, (hipStream_t)stream);
}
int masr_test_gemm_pe_acc(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, const float* bias, const float* pe,
                          int pe_period, int accumulate, float* C32, int64_t ldc, uint16_t* C16, int64_t ldc16, void* stream) {
    GemmArgs g = gemm_args();
    g.A = (const bf16*)A; g.lda = lda; g.B = (const bf16*)B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.bias = bias;
    g.pe = pe; g.pe_period = pe_period; g.accumulate = accumulate; g.C32 = C32; g.ldc = ldc; g.C16 = (bf16*)C16; g.ldc16 = ldc16;
    return mk_gemm(g, (hipStream_t)stream);
}
int masr_test_skinny_gemm(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, int M, int N, int K, const float* bias, int relu,
                          const float* residual, float* C32, uint16_t* C16, void* stream) {
    SkinnyArgs g{};
    g.A = (const bf16*)A; g.lda = lda; g.W = (const bf16*)W; g.ldw = ldw; g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu = relu;
    g.residual = residual; g.ldres = N; g.C32 = C32; g.ldc = N; g.C16 = (bf16*)C16; g.ldc16 = N;
    return mk_skinny_gemm(g, (hipStream_t)stream);
}
int masr_test_rescore_score(const float* logits, int64_t ld, const int32_t* gold, int R, int L, int C, float* row_lp, float* att, void* stream) {
    if (!logits || !gold || !row_lp || !att) { mk_set_error("masr_test_rescore_score", "null pointer"); return -1; }
    return mk_rescore_score(logits, (long)ld, gold, R, L, C, row_lp, att, (hipStream_t)stream);
}
int masr_test_rescore_select(const int32_t* tokens_in, int64_t ld_tok, const int32_t* lens_in, const float* ctc_in, const float* att_in, int B, int N,
                             float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc, int32_t* order,
                             void* stream) {
    if (!lens_in || !ctc_in || !att_in || !lens || !scores || !att || !ctc || !order || (ld_tok > 0 && (!tokens_in || !tokens))) {
        mk_set_error("masr_test_rescore_select", "null pointer"); return -1;
    }
    return mk_rescore_select(tokens_in, (long)ld_tok, lens_in, ctc_in, att_in, B, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order,
                             (hipStream_t)stream);
}
}  // extern "C"
// masr_test_ctc_prefix (pre_lm == null) and masr_test_ctc_prefix_lm
static int test_ctc_prefix(const char* fn, const float* lp, int C, int T, int last, const float* parent, float psi_par, float score, const int32_t* cand,
                           const float* att_lp, const float* pre_lm, int n, float att_w, float ctc_w, float len_bonus, int32_t* list_tok,
                           float* list_score, float* list_psi, int32_t* list_slot, float* out_state, void* stream) {
    if (!lp || !cand || !att_lp || !list_tok || !list_score || !list_psi || !list_slot || !out_state || (last >= 0 && !parent)) {
        mk_set_error(fn, "null pointer"); return -1;
    }
    if (C < 2 || T < 1 || n < 1 || n > 96 || last < -1 || last >= C) { mk_set_error(fn, "need C >= 2, T >= 1, 1 <= n <= 96, -1 <= last < C"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> hc(n);
    HIP_CHECK_RET(hipMemcpyAsync(hc.data(), cand, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    for (int v : hc) if (v == 0 || v < -1 || v >= C) { mk_set_error(fn, "candidates must lie in 1 .. C-1 or be -1"); return -1; }
    // one utterance, one row (B = K = R = 1), P = n; step 1 reads the empty state of parity 0, step 2 the given parent in parity 1
    const int st = last < 0 ? 1 : 2;
    const size_t plane = (size_t)T * n;
    char* w = nullptr;
    HIP_CHECK_RET(hipMalloc(&w, 256 + 2 * plane * sizeof(float2)));
    if (hipMemsetAsync(w, 0, 256 + 2 * plane * sizeof(float2), s) != hipSuccess) { hipFree(w); mk_set_error(fn, "memset failed"); return -1; }
    int* ints = reinterpret_cast<int*>(w);                  // step[2] | fin | enc_len | tok_hist | src
    float* flts = reinterpret_cast<float*>(w + 64);         // score | psi
    const int h_ints[6] = {st, 0, 0, T, last, 0};
    const float h_flts[2] = {score, psi_par};
    BeamArgs a{};
    a.step = ints; a.fin = ints + 2; a.enc_lens = ints + 3; a.tok_hist = ints + 4; a.src = ints + 5;
    a.score = flts; a.psi = flts + 1;
    a.B = 1; a.K = 1; a.R = 1; a.Lmax = st; a.C = C; a.sos = 0; a.eos = C - 1;
    a.P = n; a.Tp = T; a.att_w = att_w; a.ctc_w = ctc_w;
    a.ctc_lp = lp; a.ctc_state = reinterpret_cast<float2*>(w + 256);
    a.pre_tok = const_cast<int*>(cand); a.pre_lp = const_cast<float*>(att_lp);
    a.list_tok = list_tok; a.list_score = list_score; a.list_psi = list_psi; a.list_slot = list_slot;
    if (pre_lm) { a.N = 1; a.pre_lm = const_cast<float*>(pre_lm); a.wts = flts + 4; a.att_w = a.ctc_w = 0.f; }      // (N > 0: the LM kernel, which reads its weights from a.wts)
    int rc = 0;
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemcpyAsync(ints, h_ints, sizeof h_ints, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(flts, h_flts, sizeof h_flts, hipMemcpyHostToDevice, s));
        if (pre_lm) CK(mk_beam_set_weights(a, att_w, ctc_w, 0.f, len_bonus, s));
        if (last < 0) CK(mk_beam_ctc_init(a, s));            // (writes psi 0 and src 0: the empty hypothesis)
        else HIP_CHECK_RET(hipMemcpy2DAsync(a.ctc_state + plane, (size_t)n * sizeof(float2), parent, sizeof(float2), sizeof(float2), T,
                                            hipMemcpyDeviceToDevice, s));
        CK(mk_beam_ctc_prefix(a, s));
        HIP_CHECK_RET(hipMemcpyAsync(out_state, a.ctc_state + (st & 1) * plane, plane * sizeof(float2), hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    rc = run();
    hipFree(w);
    return rc;
}
extern "C" {
int masr_test_ctc_prefix(const float* lp, int C, int T, int last, const float* parent, float psi_par, float score, const int32_t* cand,
                         const float* att_lp, int n, float att_w, float ctc_w, int32_t* list_tok, float* list_score, float* list_psi,
                         int32_t* list_slot, float* out_state, void* stream) {
    return test_ctc_prefix("masr_test_ctc_prefix", lp, C, T, last, parent, psi_par, score, cand, att_lp, nullptr, n, att_w, ctc_w, 0.f, list_tok,
                           list_score, list_psi, list_slot, out_state, stream);
}
int masr_test_ctc_prefix_lm(const float* lp, int C, int T, int last, const float* parent, float psi_par, float score, const int32_t* cand,
                            const float* att_lp, const float* pre_lm, int n, float att_w, float ctc_w, float len_bonus, int32_t* list_tok,
                            float* list_score, float* list_psi, int32_t* list_slot, float* out_state, void* stream) {
    if (!pre_lm) { mk_set_error("masr_test_ctc_prefix_lm", "null pointer"); return -1; }
    return test_ctc_prefix("masr_test_ctc_prefix_lm", lp, C, T, last, parent, psi_par, score, cand, att_lp, pre_lm, n, att_w, ctc_w, len_bonus, list_tok,
                           list_score, list_psi, list_slot, out_state, stream);
}
int masr_test_ctc_align_no_trace(const float* logits, int64_t ld, const int32_t* enc_lens, const int32_t* targets, const int32_t* tgt_off,
                                 const int32_t* tgt_len, int B, int Tp, int C, int blank, int maxL, void* work, int64_t work_bytes, int32_t* frames,
                                 int32_t* start, int32_t* end, float* score, void* stream) {
    return mk_ctc_align(logits, (long)ld, enc_lens, targets, tgt_off, tgt_len, B, Tp, C, blank, maxL, work, work_bytes, frames, start, end, score,
                        (hipStream_t)stream, false);
}
int masr_test_attn_decode(const uint16_t* q, int64_t ldq, const uint16_t* k, const uint16_t* v, int64_t ldk, int64_t kv_batch_stride,
                          const uint16_t* knew, const uint16_t* vnew, int64_t ldnew, const int32_t* step, const int32_t* klens, uint16_t* o,
                          int64_t ldo, int B, int H, int hd, int Tk_cap, int rows_per_utt, const int32_t* src, int64_t ld_src, int64_t src_flip,
                          void* stream) {
    const char* fn = "masr_test_attn_decode";
    if (!q || !k || !v || !o || !step == !klens || !knew != !vnew || (src && !step)) {
        mk_set_error(fn, "null pointer (exactly one of step / klens; knew and vnew together; src with step only)"); return -1;
    }
    if (B < 1 || H < 1 || Tk_cap < 1 || rows_per_utt < 0 || (src && (ld_src < 0 || src_flip < 0))) { mk_set_error(fn, "bad sizes"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    // the rows of the key/value cache the launch can address: row b reads cache row b, or b / rows_per_utt
    const int ncache = rows_per_utt > 1 ? (B + rows_per_utt - 1) / rows_per_utt : B;
    std::vector<int> kl(ncache);
    if (step) HIP_CHECK_RET(hipMemcpyAsync(kl.data(), step, sizeof(int), hipMemcpyDeviceToHost, s));
    else HIP_CHECK_RET(hipMemcpyAsync(kl.data(), klens, sizeof(int) * ncache, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    if (step) std::fill(kl.begin(), kl.end(), kl[0]);
    for (int n : kl) if (n < 1 || n > Tk_cap) { mk_set_error(fn, "key count outside [1, Tk_cap]"); return -1; }
    if (src) {                                               // every slot-table entry the launch reads must name a cache row
        std::vector<int> row;
        for (int b = 0; b < B; ++b) {
            const int n = kl[rows_per_utt > 1 ? b / rows_per_utt : b];
            row.resize(n);
            HIP_CHECK_RET(hipMemcpy(row.data(), src + (n & 1) * src_flip + (long)b * ld_src, sizeof(int) * n, hipMemcpyDeviceToHost));
            for (int j = 0; j < n - (knew ? 1 : 0); ++j) if (row[j] < 0 || row[j] >= ncache) { mk_set_error(fn, "src entry outside the cache rows"); return -1; }
        }
    }
    AttnDecodeArgs a{};
    a.q = (const bf16*)q; a.ldq = ldq; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ldk = ldk; a.kv_batch_stride = kv_batch_stride;
    a.knew = (const bf16*)knew; a.vnew = (const bf16*)vnew; a.ldnew = ldnew; a.step = step; a.klens = klens; a.o = (bf16*)o; a.ldo = ldo;
    a.B = B; a.H = H; a.hd = hd; a.Tk_cap = Tk_cap; a.rows_per_utt = rows_per_utt; a.src = src; a.ld_src = ld_src; a.src_flip = src_flip;
    return mk_attn_decode(a, s);
}
int masr_test_logits_f32(const float* y32, const float* W32, const float* bias, float* z, int64_t ld, int rows, int C, int E, void* stream) {
    if (!y32 || !W32 || !bias || !z || C < 1 || ld < C) { mk_set_error("masr_test_logits_f32", "null pointer, C < 1 or ld < C"); return -1; }
    return mk_logits_f32(y32, W32, bias, z, ld, rows, C, E, (hipStream_t)stream);
}
int masr_test_recog_argmax_step(int32_t* step, const float* logits, int64_t ld, int32_t* out, int B, int C, void* stream) {
    if (!step || !logits || !out || B < 1 || C < 1 || ld < C) { mk_set_error("masr_test_recog_argmax_step", "null pointer, B < 1, C < 1 or ld < C"); return -1; }
    return mk_recog_argmax_step(step, logits, ld, out, B, C, (hipStream_t)stream);
}
int masr_test_beam_step(int B, int K, int C, int sos, int eos, int t, const int32_t* minlen, const int32_t* maxlen, const float* logits,
                        int64_t ld, float* score, int32_t* fin, float* best_score, int32_t* best_len, int32_t* best_row, int32_t* list_tok,
                        float* list_score, int32_t* tok_hist_row, int32_t* par_hist_row, int32_t* step_out, void* stream) {
    const char* fn = "masr_test_beam_step";
    if (!minlen || !maxlen || !logits || !score || !fin || !best_score || !best_len || !best_row || !list_tok || !list_score ||
        !tok_hist_row || !par_hist_row || !step_out) {
        mk_set_error(fn, "null pointer"); return -1;
    }
    if (K < 1 || K > 64) { mk_set_error(fn, "beam size must be in [1, 64]"); return -1; }
    if (B < 1 || C < 1 || t < 1 || ld < C || sos < 0 || sos >= C || eos < 0 || eos >= C) { mk_set_error(fn, "need B, C, t >= 1, ld >= C, sos / eos < C"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    const size_t hist = (size_t)t * R * sizeof(int);
    int* w = nullptr;                                        // step[2] | tok_hist [t][R] | par_hist [t][R]
    HIP_CHECK_RET(hipMalloc(&w, 64 + 2 * hist));
    int* tok_hist = w + 16;
    int* par_hist = tok_hist + (size_t)t * R;
    const int h_step[2] = {t, 0};
    BeamArgs a{};
    a.step = w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = sos; a.eos = eos; a.maxlen = maxlen; a.minlen = minlen;
    a.tok_hist = tok_hist; a.par_hist = par_hist; a.score = score; a.list_tok = list_tok; a.list_score = list_score; a.fin = fin;
    a.best_score = best_score; a.best_len = best_len; a.best_row = best_row;
    auto run = [&]() -> int {                                // row t-1 of the history starts as the caller's, so untouched entries show
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist + (size_t)(t - 1) * R, tok_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist + (size_t)(t - 1) * R, par_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        CK(mk_beam_rows(a, BeamRowLm{}, logits, ld, s));
        CK(mk_beam_select(a, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist_row, tok_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist_row, par_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(step_out, w, sizeof h_step, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
// ---- n-gram LM shallow fusion (lm.hip)
int masr_test_lm_score(const masr_lm* lm, const int32_t* ctx, int R, float* out, void* stream) {
    const char* fn = "masr_test_lm_score";
    if (!lm || !out || R < 1 || (lm->dev.order > 1 && !ctx)) { mk_set_error(fn, "null pointer or R < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int w = lm->dev.order - 1;
    if (w > 0) {
        std::vector<int> h((size_t)R * w);
        HIP_CHECK_RET(hipMemcpyAsync(h.data(), ctx, sizeof(int) * h.size(), hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        for (int r = 0; r < R; ++r)
            for (int i = 0; i < w; ++i) {
                const int t = h[(size_t)r * w + i];
                if (t < -1 || t >= lm->dev.C) { mk_set_error(fn, "context ids must lie in [-1, C)"); return -1; }
                if (t == -1 && i > 0 && h[(size_t)r * w + i - 1] != -1) { mk_set_error(fn, "-1 may only stand in front of a context"); return -1; }
            }
    }
    CK(mk_lm_score(lm->dev, ctx, R, out, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_lm_max_probe(const masr_lm* lm) {
    if (!lm) { mk_set_error("masr_test_lm_max_probe", "null model"); return -1; }
    return lm->max_probe;
}
// ---- contextual phrase biasing (bias.hip)
int masr_test_bias_step(const masr_bias* bias, const int32_t* nodes_in, const int32_t* n_in, const int32_t* tokens, int count, int32_t* nodes_out,
                        int32_t* n_out, void* stream) {
    const char* fn = "masr_test_bias_step";
    if (!bias || !nodes_in || !n_in || !tokens || !nodes_out || !n_out || count < 1) { mk_set_error(fn, "null pointer or count < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_bias_step(bias->dev, nodes_in, n_in, tokens, count, nodes_out, n_out, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_bias_max_probe(const masr_bias* bias) {
    if (!bias) { mk_set_error("masr_test_bias_max_probe", "null phrase list"); return -1; }
    return bias->max_probe;
}
}  // extern "C"
// masr_test_beam_lm_topk and masr_test_joint_lm_prebeam (out.P > 0): the row stage with the n-gram LM at step t on the caller's logits,
// scores and histories.  `out` brings the entry's output arrays (and P); the rest of the beam's state is filled in here.
// masr_test_beam_nlm_rows: the same with caller-given LM logit rows [R][ld_lm] over C classes in the n-gram's place (no history is read)
static int test_lm_rows(const char* fn, const masr_lm* lm, const float* lm_logits, int64_t ld_lm, int C, float lm_w, int B, int K, int t,
                        const int32_t* minlen, const float* logits, int64_t ld, const float* score, const int32_t* tok_hist, const int32_t* par_hist,
                        BeamArgs a, void* stream) {
    if ((!lm && !lm_logits) || !minlen || !logits || !score || (lm && t > 1 && (!tok_hist || !par_hist))) { mk_set_error(fn, "null pointer"); return -1; }
    if (K < 1 || K > 64) { mk_set_error(fn, "beam size must be in [1, 64]"); return -1; }
    if (lm) C = lm->dev.C;
    else if (C < 2 || ld_lm < C) { mk_set_error(fn, "need C >= 2 and ld_lm >= C"); return -1; }
    if (B < 1 || t < 1 || ld < C || (int64_t)B * K > (1 << 20)) { mk_set_error(fn, "need B, t >= 1, ld >= C, B * K <= 2^20"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    char* w = nullptr;                                       // step[2] | weights [4] | fin [B] | fused [R][ld]
    const size_t wts_off = 64, fin_off = 128, fused_off = (fin_off + sizeof(int) * (size_t)B + 255) & ~(size_t)255;
    HIP_CHECK_RET(hipMalloc(&w, fused_off + sizeof(float) * (size_t)R * ld));
    const int h_step[2] = {t, 0};
    a.step = (int*)w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = 0; a.eos = C - 1; a.minlen = minlen;
    a.tok_hist = const_cast<int*>(tok_hist); a.par_hist = const_cast<int*>(par_hist); a.score = const_cast<float*>(score);
    a.fin = (int*)(w + fin_off); a.wts = (float*)(w + wts_off);
    BeamRowLm rl{};
    if (lm) rl.ngram = &lm->dev;
    else { rl.lm_logits = lm_logits; rl.ld_lm = ld_lm; }
    rl.fused = (float*)(w + fused_off); rl.ldf = ld; rl.lm_w = lm_w;
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemsetAsync(w, 0, fused_off, s));
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        if (a.P) CK(mk_beam_set_weights(a, 0.f, 0.f, lm_w, 0.f, s));     // (the pre-beam reads its weight from the device)
        CK(mk_beam_rows(a, rl, logits, ld, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
extern "C" {
int masr_test_beam_lm_topk(const masr_lm* lm, float lm_w, int B, int K, int t, const int32_t* minlen, const float* logits, int64_t ld,
                           const float* score, const int32_t* tok_hist, const int32_t* par_hist, int32_t* list_tok, float* list_score, void* stream) {
    const char* fn = "masr_test_beam_lm_topk";
    if (!list_tok || !list_score) { mk_set_error(fn, "null pointer"); return -1; }
    BeamArgs out{};
    out.list_tok = list_tok; out.list_score = list_score;
    return test_lm_rows(fn, lm, nullptr, 0, 0, lm_w, B, K, t, minlen, logits, ld, score, tok_hist, par_hist, out, stream);
}
// ---- the joint LM beam's step kernels
int masr_test_joint_lm_prebeam(const masr_lm* lm, float lm_w, int B, int K, int t, const int32_t* minlen, const float* logits, int64_t ld,
                               const float* score, const int32_t* tok_hist, const int32_t* par_hist, int32_t* pre_tok, float* pre_lp, float* pre_lm,
                               void* stream) {
    const char* fn = "masr_test_joint_lm_prebeam";
    if (!pre_tok || !pre_lp || !pre_lm) { mk_set_error(fn, "null pointer"); return -1; }
    BeamArgs out{};
    out.P = std::max(1, 3 * K / 2); out.pre_tok = pre_tok; out.pre_lp = pre_lp; out.pre_lm = pre_lm;
    return test_lm_rows(fn, lm, nullptr, 0, 0, lm_w, B, K, t, minlen, logits, ld, score, tok_hist, par_hist, out, stream);
}
// ---- the row stage with LM logits: pre_tok given = the pre-beam form, else top-K
int masr_test_beam_nlm_rows(const float* lm_logits, int64_t ld_lm, float lm_w, int B, int K, int C, int t, const int32_t* minlen, const float* logits,
                            int64_t ld, const float* score, int32_t* list_tok, float* list_score, int32_t* pre_tok, float* pre_lp, float* pre_lm,
                            void* stream) {
    const char* fn = "masr_test_beam_nlm_rows";
    BeamArgs out{};
    if (pre_tok) {
        if (!pre_lp || !pre_lm) { mk_set_error(fn, "null pointer"); return -1; }
        out.P = std::max(1, 3 * K / 2); out.pre_tok = pre_tok; out.pre_lp = pre_lp; out.pre_lm = pre_lm;
    } else {
        if (!list_tok || !list_score) { mk_set_error(fn, "null pointer"); return -1; }
        out.list_tok = list_tok; out.list_score = list_score;
    }
    if (!lm_logits) { mk_set_error(fn, "null pointer"); return -1; }
    return test_lm_rows(fn, nullptr, lm_logits, ld_lm, C, lm_w, B, K, t, minlen, logits, ld, score, nullptr, nullptr, out, stream);
}
int masr_test_beam_select_nbest(int B, int K, int N, int C, int t, const int32_t* maxlen, float len_bonus, const int32_t* list_tok,
                                const float* list_score, const float* list_psi, const int32_t* list_slot, float* score, float* psi, int32_t* src,
                                int32_t* fin, float* nb_score, int32_t* nb_len, int32_t* nb_row, int32_t* tok_hist_row, int32_t* par_hist_row,
                                int32_t* step_out, void* stream) {
    const char* fn = "masr_test_beam_select_nbest";
    if (!maxlen || !list_tok || !list_score || !list_psi || !list_slot || !score || !psi || !src || !fin || !nb_score || !nb_len || !nb_row ||
        !tok_hist_row || !par_hist_row || !step_out) {
        mk_set_error(fn, "null pointer"); return -1;
    }
    if (K < 1 || K > 64 || N < 1 || N > K) { mk_set_error(fn, "need 1 <= N <= K <= 64"); return -1; }
    if (B < 1 || C < 2 || t < 1) { mk_set_error(fn, "need B, t >= 1, C >= 2"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    const size_t hist = (size_t)t * R * sizeof(int);
    int* w = nullptr;                                        // step[2] | weights [4] at int 16 | tok_hist [t][R] | par_hist [t][R]
    HIP_CHECK_RET(hipMalloc(&w, 128 + 2 * hist));
    int* tok_hist = w + 32;
    int* par_hist = tok_hist + (size_t)t * R;
    const int h_step[2] = {t, 0};
    BeamArgs a{};
    a.step = w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = 0; a.eos = C - 1; a.maxlen = maxlen; a.P = std::max(1, 3 * K / 2); a.N = N;
    a.tok_hist = tok_hist; a.par_hist = par_hist; a.score = score; a.psi = psi; a.src = src; a.fin = fin;
    a.list_tok = const_cast<int*>(list_tok); a.list_score = const_cast<float*>(list_score);
    a.list_psi = const_cast<float*>(list_psi); a.list_slot = const_cast<int*>(list_slot);
    a.nb_score = nb_score; a.nb_len = nb_len; a.nb_row = nb_row; a.wts = reinterpret_cast<float*>(w + 16);
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist + (size_t)(t - 1) * R, tok_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist + (size_t)(t - 1) * R, par_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        CK(mk_beam_set_weights(a, 0.f, 0.f, 0.f, len_bonus, s));
        CK(mk_beam_select(a, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist_row, tok_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist_row, par_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(step_out, w, sizeof h_step, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
static int test_read_ints(const int32_t* dev, size_t n, std::vector<int>& host, hipStream_t s);
// ---- the phrase-biased step kernels alone (tests/test_hip_bias_beam_kernels.py)
int masr_test_beam_bias_rows(const masr_lm* lm, const masr_bias* bias, float lm_w, float bias_w, int B, int K, int t, const int32_t* minlen,
                             const int32_t* maxlen, const float* logits, int64_t ld, const float* score, const int32_t* tok_hist, const int32_t* par_hist,
                             const int32_t* state_in, int32_t* state_out, int32_t* list_tok, float* list_score, int32_t* pre_tok, float* pre_lp,
                             float* pre_lm, float* pre_b, void* stream) {
    const char* fn = "masr_test_beam_bias_rows";
    if (!bias || !minlen || !maxlen || !logits || !score || !state_out || (t > 1 && (!tok_hist || !par_hist || !state_in))) { mk_set_error(fn, "null pointer"); return -1; }
    if (pre_tok ? (!pre_lp || !pre_lm || !pre_b) : (!list_tok || !list_score)) { mk_set_error(fn, "null pointer"); return -1; }
    if (K < 1 || K > 64) { mk_set_error(fn, "beam size must be in [1, 64]"); return -1; }
    const int C = bias->dev.C;
    if (lm && lm->dev.C != C) { mk_set_error(fn, "the LM's classes differ from the list's"); return -1; }
    if (B < 1 || t < 1 || ld < C || (int64_t)B * K > (1 << 20)) { mk_set_error(fn, "need B, t >= 1, ld >= C, B * K <= 2^20"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    if (t > 1) {                                             // every node the kernel starts from must be one of the trie's
        std::vector<int> hs;
        CK(test_read_ints(state_in, (size_t)2 * R, hs, s));
        for (int r = 0; r < R; ++r) if (hs[2 * r] < 0 || hs[2 * r] >= bias->dev.nodes) { mk_set_error(fn, "state node outside the trie"); return -1; }
    }
    char* w = nullptr;                                       // step[2] | weights [5] | fin [B] | states [2][R] | fused [R][ld]
    const size_t wts_off = 64, fin_off = 128, st_off = (fin_off + sizeof(int) * (size_t)B + 255) & ~(size_t)255;
    const size_t fused_off = (st_off + sizeof(int2) * 2 * (size_t)R + 255) & ~(size_t)255;
    HIP_CHECK_RET(hipMalloc(&w, fused_off + sizeof(float) * (size_t)R * ld));
    const int h_step[2] = {t, 0};
    BeamArgs a{};
    a.step = (int*)w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = 0; a.eos = C - 1; a.minlen = minlen; a.maxlen = maxlen;
    a.tok_hist = const_cast<int*>(tok_hist); a.par_hist = const_cast<int*>(par_hist); a.score = const_cast<float*>(score);
    a.fin = (int*)(w + fin_off); a.wts = (float*)(w + wts_off);
    if (pre_tok) { a.P = std::max(1, 3 * K / 2); a.N = 1; a.pre_tok = pre_tok; a.pre_lp = pre_lp; a.pre_lm = pre_lm; }
    else { a.list_tok = list_tok; a.list_score = list_score; }
    BeamRowLm rl{};
    if (lm) rl.ngram = &lm->dev;
    rl.fused = (float*)(w + fused_off); rl.ldf = ld; rl.lm_w = lm_w;
    int2* st = (int2*)(w + st_off);
    const BeamBias bb{&bias->dev, st, pre_b, bias_w};
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemsetAsync(w, 0, fused_off, s));
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        if (t > 1) HIP_CHECK_RET(hipMemcpyAsync(st + (size_t)((t - 1) & 1) * R, state_in, sizeof(int2) * R, hipMemcpyDeviceToDevice, s));
        if (a.P) { CK(mk_beam_set_weights(a, 0.f, 0.f, lm_w, 0.f, s)); CK(mk_beam_set_bias_weight(a, bias_w, s)); }
        CK(mk_beam_rows(a, rl, logits, ld, s, &bb));
        HIP_CHECK_RET(hipMemcpyAsync(state_out, st + (size_t)(t & 1) * R, sizeof(int2) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
int masr_test_beam_select_bias(int B, int K, int C, int t, const int32_t* maxlen, float bias_w, const int32_t* list_tok, const float* list_score,
                               float* score, int32_t* fin, float* best_score, int32_t* best_len, int32_t* best_row, int32_t* tok_hist_row,
                               int32_t* par_hist_row, int32_t* step_out, void* stream) {
    const char* fn = "masr_test_beam_select_bias";
    if (!maxlen || !list_tok || !list_score || !score || !fin || !best_score || !best_len || !best_row || !tok_hist_row || !par_hist_row || !step_out) {
        mk_set_error(fn, "null pointer"); return -1;
    }
    if (K < 1 || K > 64 || B < 1 || C < 2 || t < 1) { mk_set_error(fn, "need 1 <= K <= 64, B, t >= 1, C >= 2"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    const size_t hist = (size_t)t * R * sizeof(int);
    int* w = nullptr;                                        // step[2] | tok_hist [t][R] | par_hist [t][R]
    HIP_CHECK_RET(hipMalloc(&w, 64 + 2 * hist));
    int* tok_hist = w + 16;
    int* par_hist = tok_hist + (size_t)t * R;
    const int h_step[2] = {t, 0};
    BeamArgs a{};
    a.step = w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = 0; a.eos = C - 1; a.maxlen = maxlen;
    a.tok_hist = tok_hist; a.par_hist = par_hist; a.score = score; a.fin = fin;
    a.list_tok = const_cast<int*>(list_tok); a.list_score = const_cast<float*>(list_score);
    a.best_score = best_score; a.best_len = best_len; a.best_row = best_row;
    BeamBias bb{}; bb.bias_w = bias_w;
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist + (size_t)(t - 1) * R, tok_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist + (size_t)(t - 1) * R, par_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        CK(mk_beam_select(a, s, &bb));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist_row, tok_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist_row, par_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(step_out, w, sizeof h_step, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
int masr_test_beam_select_nbest_bias(int B, int K, int N, int C, int t, const int32_t* maxlen, float len_bonus, float bias_w, const int32_t* list_tok,
                                     const float* list_score, const float* list_psi, const int32_t* list_slot, float* score, float* psi, int32_t* src,
                                     int32_t* fin, float* nb_score, int32_t* nb_len, int32_t* nb_row, int32_t* tok_hist_row, int32_t* par_hist_row,
                                     int32_t* step_out, void* stream) {
    const char* fn = "masr_test_beam_select_nbest_bias";
    if (!maxlen || !list_tok || !list_score || !list_psi || !list_slot || !score || !psi || !src || !fin || !nb_score || !nb_len || !nb_row ||
        !tok_hist_row || !par_hist_row || !step_out) {
        mk_set_error(fn, "null pointer"); return -1;
    }
    if (K < 1 || K > 64 || N < 1 || N > K) { mk_set_error(fn, "need 1 <= N <= K <= 64"); return -1; }
    if (B < 1 || C < 2 || t < 1) { mk_set_error(fn, "need B, t >= 1, C >= 2"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
    const size_t hist = (size_t)t * R * sizeof(int);
    int* w = nullptr;                                        // step[2] | weights [5] at int 16 | tok_hist [t][R] | par_hist [t][R]
    HIP_CHECK_RET(hipMalloc(&w, 128 + 2 * hist));
    int* tok_hist = w + 32;
    int* par_hist = tok_hist + (size_t)t * R;
    const int h_step[2] = {t, 0};
    BeamArgs a{};
    a.step = w; a.B = B; a.K = K; a.R = R; a.Lmax = t; a.C = C; a.sos = 0; a.eos = C - 1; a.maxlen = maxlen; a.P = std::max(1, 3 * K / 2); a.N = N;
    a.tok_hist = tok_hist; a.par_hist = par_hist; a.score = score; a.psi = psi; a.src = src; a.fin = fin;
    a.list_tok = const_cast<int*>(list_tok); a.list_score = const_cast<float*>(list_score);
    a.list_psi = const_cast<float*>(list_psi); a.list_slot = const_cast<int*>(list_slot);
    a.nb_score = nb_score; a.nb_len = nb_len; a.nb_row = nb_row; a.wts = reinterpret_cast<float*>(w + 16);
    const BeamBias bb{};
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist + (size_t)(t - 1) * R, tok_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist + (size_t)(t - 1) * R, par_hist_row, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        CK(mk_beam_set_weights(a, 0.f, 0.f, 0.f, len_bonus, s));
        CK(mk_beam_set_bias_weight(a, bias_w, s));
        CK(mk_beam_select(a, s, &bb));
        HIP_CHECK_RET(hipMemcpyAsync(tok_hist_row, tok_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(par_hist_row, par_hist + (size_t)(t - 1) * R, sizeof(int) * R, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipMemcpyAsync(step_out, w, sizeof h_step, hipMemcpyDeviceToDevice, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
// ---- the training step's row kernels alone (tests/test_hip_train_row_kernels.py): each entry vets what the kernel would index with, fills the
// launcher's arguments and calls it
static int test_read_ints(const int32_t* dev, size_t n, std::vector<int>& host, hipStream_t s) {
    host.resize(n);
    HIP_CHECK_RET(hipMemcpyAsync(host.data(), dev, sizeof(int) * n, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_ls_ce(const float* logits, int64_t ld, const int32_t* gold, int rows, int C, float eps, float inv_ntotal, const float* inv_ntotal_ptr,
                    float grad_w, uint16_t* dlogits, float* row_loss, int32_t* row_correct, float* stats, void* stream) {
    const char* fn = "masr_test_ls_ce";
    if (!logits || !gold || !dlogits || !row_loss || !row_correct || !stats) { mk_set_error(fn, "null pointer"); return -1; }
    if (rows < 1 || C < 1 || ld < C) { mk_set_error(fn, "need rows >= 1, C >= 1, ld >= C"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> hg;
    CK(test_read_ints(gold, (size_t)rows, hg, s));
    for (int g : hg) if (g < -1 || g >= C) { mk_set_error(fn, "gold must lie in [0, C) or be -1"); return -1; }
    return mk_ls_ce(logits, ld, gold, rows, C, eps, inv_ntotal, (bf16*)dlogits, row_loss, row_correct, stats, s, inv_ntotal_ptr, grad_w);
}
int masr_test_embed_fwd(const int32_t* tok, const float* table, const float* pe, float* y32, uint16_t* y16, int B, int L, int E, int V, float drop_p,
                        uint32_t seed, uint32_t site, const uint32_t* seed_ptr, void* stream) {
    const char* fn = "masr_test_embed_fwd";
    if (!tok || !table || !pe || !y32 || !y16) { mk_set_error(fn, "null pointer"); return -1; }
    if (B < 1 || L < 1 || E < 1 || V < 1 || !(drop_p >= 0.f && drop_p < 1.f)) { mk_set_error(fn, "need B, L, E, V >= 1 and 0 <= drop_p < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ht;
    CK(test_read_ints(tok, (size_t)B * L, ht, s));
    for (int t : ht) if (t < 0 || t >= V) { mk_set_error(fn, "token outside [0, V)"); return -1; }
    return mk_embed_fwd(tok, table, pe, y32, (bf16*)y16, B, L, E, drop_p, seed, site, s, seed_ptr);
}
int masr_test_embed_bwd(const int32_t* tok, int n, const float* dy, float* dtable, int V, int E, int accumulate, float drop_p, uint32_t seed,
                        uint32_t site, const uint32_t* seed_ptr, void* stream) {
    const char* fn = "masr_test_embed_bwd";
    if (!tok || !dy || !dtable) { mk_set_error(fn, "null pointer"); return -1; }
    if (n < 1 || V < 1 || E < 1 || !(drop_p >= 0.f && drop_p < 1.f)) { mk_set_error(fn, "need n, V, E >= 1 and 0 <= drop_p < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ht;
    CK(test_read_ints(tok, (size_t)n, ht, s));
    for (int t : ht) if (t < 0 || t >= V) { mk_set_error(fn, "token outside [0, V)"); return -1; }
    std::vector<int> sorted((size_t)n + V + 1);                // order [n] | start [V + 1], as masr_run_batch stages them
    group_positions_by_token(ht.data(), 1, n, nullptr, V, sorted.data(), sorted.data() + n);
    int* d = nullptr;
    HIP_CHECK_RET(hipMalloc(&d, sizeof(int) * sorted.size()));
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemcpyAsync(d, sorted.data(), sizeof(int) * sorted.size(), hipMemcpyHostToDevice, s));
        CK(mk_embed_bwd(d, d + n, dy, dtable, V, E, accumulate, drop_p, seed, site, s, seed_ptr));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(d);
    return rc;
}
int masr_test_cast_dropout(const float* x, uint16_t* y, int64_t n, float drop_p, uint32_t seed, uint32_t site, const uint32_t* seed_ptr, void* stream) {
    if (!x || !y || n < 1 || n > 0x7fffffffL || !(drop_p >= 0.f && drop_p < 1.f)) {
        mk_set_error("masr_test_cast_dropout", "null pointer, n outside [1, 2^31) or drop_p outside [0, 1)"); return -1;
    }
    return mk_cast_dropout(x, (bf16*)y, (long)n, drop_p, seed, site, (hipStream_t)stream, seed_ptr);
}
int masr_test_vgg2enc_grad_unpermute(const float* g, float* dw, int E, int C, int Dp, void* stream) {
    if (!g || !dw || E < 1 || C < 1 || Dp < 1) { mk_set_error("masr_test_vgg2enc_grad_unpermute", "null pointer or E, C, Dp < 1"); return -1; }
    return mk_vgg2enc_grad_unpermute(g, dw, E, C, Dp, (hipStream_t)stream);
}
int masr_test_recog_argmax(const float* logits, int64_t ld, int32_t* out, int B, int L, int C, void* stream) {
    if (!logits || !out || B < 1 || L < 1 || C < 1 || ld < C) { mk_set_error("masr_test_recog_argmax", "null pointer, B, L, C < 1 or ld < C"); return -1; }
    return mk_recog_argmax(logits, ld, out, B, L, C, (hipStream_t)stream);
}
int masr_test_linear_shadows(const float* P, int64_t src, int N, int K, int ldt, uint16_t* k16, uint16_t* t16, void* stream) {
    if (N <= 0 || K <= 0 || ldt < N || src < 4) { mk_set_error("masr_test_linear_shadows", "N, K > 0, ldt >= N, src >= 4 (the tile pass reads up to three floats in front of a row)"); return -1; }
    ShadowJobs jobs{};
    jobs.n = 1;
    jobs.d[0] = ShadowDesc{src, SH_LINEAR, N, K, ldt, 0, 0, 0};
    jobs.blocks = mk_shadow_blocks(jobs.d[0]);
    jobs.p[0] = (bf16*)k16; jobs.p[1] = (bf16*)t16;
    return mk_all_shadows(P, jobs, (hipStream_t)stream);
}
int masr_test_conv1_fwd(const float* x, const float* w, const float* bias, uint16_t* out, uint64_t* relu_bits, int B, int H, int W, void* stream) {
    return mk_conv1_fwd(x, w, bias, (bf16*)out, B, H, W, (hipStream_t)stream, reinterpret_cast<unsigned long long*>(relu_bits));
}
int masr_test_conv3x3(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, uint16_t* out, int B, int H, int W, int CIN,
                      int COUT, void* stream) {
    ConvArgs a{}; a.in = (const bf16*)in; a.wk = (const bf16*)wk; a.bias = bias; a.relu = relu; a.out = (bf16*)out;
    a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3(a, (hipStream_t)stream);
}
int masr_test_conv3x3_ex(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, const uint16_t* mask, uint16_t* out,
                         uint16_t* pool_out, int B, int H, int W, int CIN, int COUT, void* stream) {
    ConvArgs a{}; a.in = (const bf16*)in; a.wk = (const bf16*)wk; a.bias = bias; a.relu = relu; a.mask = (const bf16*)mask; a.out = (bf16*)out;
    a.pool_out = (bf16*)pool_out; a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3(a, (hipStream_t)stream);
}
int masr_test_conv3x3_sign_bits(const uint16_t* in, const uint16_t* wk, const float* bias, int relu, const uint16_t* mask, const uint32_t* mask_bits,
                                uint16_t* out, uint32_t* out_sign_bits, int B, int H, int W, int CIN, int COUT, void* stream) {
    ConvArgs a{}; a.in = (const bf16*)in; a.wk = (const bf16*)wk; a.bias = bias; a.relu = relu; a.mask = (const bf16*)mask;
    a.mask_bits = (const unsigned long long*)mask_bits; a.out = (bf16*)out; a.out_sign_bits = (unsigned long long*)out_sign_bits;
    a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3(a, (hipStream_t)stream);
}
int masr_test_conv3x3_pool_idx(const uint16_t* in, const uint16_t* wk, const float* bias, uint16_t* out, uint16_t* pool_out, uint8_t* pool_idx,
                               int drop_out, int B, int H, int W, int CIN, int COUT, void* stream) {
    ConvArgs a{}; a.in = (const bf16*)in; a.wk = (const bf16*)wk; a.bias = bias; a.relu = 1; a.out = (bf16*)out;
    a.pool_out = (bf16*)pool_out; a.pool_idx = pool_idx; a.out_optional = drop_out; a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3(a, (hipStream_t)stream);
}
int masr_test_conv3x3_dgrad_pooled(const uint16_t* dy, const uint16_t* dy_pooled, const uint8_t* pool_idx, const uint16_t* wk, const uint32_t* mask_bits,
                                   uint16_t* out, int B, int H, int W, void* stream) {
    ConvArgs a{}; a.in = (const bf16*)dy; a.in_pooled = (const bf16*)dy_pooled; a.in_idx = pool_idx; a.wk = (const bf16*)wk;
    a.mask = (const bf16*)out; a.mask_bits = (const unsigned long long*)mask_bits; a.out = (bf16*)out;      // (mask: any non-null pointer -- the sign words are what is read)
    a.B = B; a.H = H; a.W = W; a.CIN = 128; a.COUT = 128;
    return mk_conv3x3(a, (hipStream_t)stream);
}
int64_t masr_test_conv1_wgrad_fused_slab_floats(int B, int H, int W) { return mk_conv1_wgrad_fused_slab_floats(B, H, W); }
int masr_test_conv1_wgrad_fused(const uint16_t* dy, const uint16_t* dy_pooled, const uint8_t* pool_idx, const uint16_t* wk, const uint64_t* mask_bits,
                                const float* x1, float* slab, int64_t slab_floats, float* dw1, float* db1, int B, int H, int W, void* stream) {
    if (slab_floats < mk_conv1_wgrad_fused_slab_floats(B, H, W)) { mk_set_error("masr_test_conv1_wgrad_fused", "slab too small"); return -1; }
    ConvArgs a{}; a.in = (const bf16*)dy; a.in_pooled = (const bf16*)dy_pooled; a.in_idx = pool_idx; a.wk = (const bf16*)wk;
    a.mask = (const bf16*)wk; a.mask_bits = (const unsigned long long*)mask_bits; a.x1 = x1; a.w1_slab = slab;
    a.B = B; a.H = H; a.W = W; a.CIN = 64; a.COUT = 64;
    CK(mk_conv3x3(a, (hipStream_t)stream));
    return mk_conv1_wgrad_fused_reduce(slab, B, H, W, dw1, db1, (hipStream_t)stream);
}
int64_t masr_test_conv3x3_wgrad_slab_floats(int B, int H, int W, int CIN, int COUT) { return mk_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT); }
int masr_test_conv3x3_wgrad(const uint16_t* in, const uint16_t* dy, float* dw, float* slab, int64_t slab_floats, int B, int H, int W, int CIN,
                            int COUT, void* stream) {
    if (slab_floats < mk_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT)) { mk_set_error("masr_test_conv3x3_wgrad", "slab too small"); return -1; }
    ConvWgradArgs a{}; a.in = (const bf16*)in; a.dy = (const bf16*)dy; a.dw = dw; a.slab = slab; a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3_wgrad(a, (hipStream_t)stream);
}
void masr_test_set_conv_grid_cap(int n) { mk_conv_force_grid_cap(n); }
int64_t masr_test_layernorm_slab_floats(int rows, int E) { return mk_layernorm_bwd_slab_floats(rows, E); }
int masr_test_layernorm(const float* x, const float* gamma, const float* beta, const float* dy, float* y, uint16_t* y16, float* mean,
                        float* rstd, float* dx, uint16_t* dx16, float* dgamma, float* dbeta, float* slab, int rows, int E, float drop_p,
                        uint32_t seed, uint32_t site, void* stream) {
    if (mk_layernorm_fwd(x, gamma, beta, y, (bf16*)y16, mean, rstd, rows, E, (hipStream_t)stream)) return -1;
    return mk_layernorm_bwd(dy, x, gamma, mean, rstd, dx, (bf16*)dx16, drop_p, seed, site, dgamma, dbeta, slab, rows, E, (hipStream_t)stream, nullptr);
}
int masr_test_ksplit_ln(const uint16_t* A, const uint16_t* B, int rows, int E, int K, int split, const float* bias, const float* residual, float drop_p,
                        uint32_t seed, uint32_t site, float* part, const float* gamma, const float* beta, float* sum_out, float* y32, uint16_t* y16,
                        float* mean, float* rstd, const float* x, float* dx32, uint16_t* dx16, float* slab, void* stream) {
    // the engine's k-split pair (ffn_fwd + ln_fwd / ffn_bwd + ln_bwd): C = A [rows, K] . B [E, K]^T as `split` fp32 partial products in `part`,
    // then the LayerNorm that sums them.  x == null: forward (row = sum + bias, dropout, + residual -> sum_out, y32 / y16, mean, rstd);
    // x given: backward (dy = sum + residual; mean / rstd are inputs; dx32 / dx16 and the [ceil(rows / 4)][2][E] partials of dgamma / dbeta in slab)
    GemmArgs g = gemm_args();
    g.A = (const bf16*)A; g.lda = K; g.B = (const bf16*)B; g.ldb = K; g.M = rows; g.N = E; g.K = K;
    g.C32 = part; g.ldc = E; g.split_k = split; g.split_stride = (long)rows * E;
    CK(mk_gemm(g, (hipStream_t)stream));
    if (!x) {
        const LnSumArgs sm{part, (long)rows * E, split, bias, residual, drop_p, seed, site, nullptr, sum_out};
        return mk_layernorm_fwd_sum(sm, gamma, beta, y32, (bf16*)y16, mean, rstd, rows, E, (hipStream_t)stream);
    }
    const LnSumArgs sm{part, (long)rows * E, split, nullptr, residual, 0.f, 0u, 0u, nullptr, nullptr};
    return mk_layernorm_bwd_sum(sm, x, gamma, mean, rstd, dx32, (bf16*)dx16, drop_p, seed, site, slab, rows, E, (hipStream_t)stream, nullptr);
}
int masr_test_wgrad_grouped(const uint16_t* dy, int64_t lddy, const uint16_t* x, int64_t ldx, float* dW, float* db, float* dW2, float* db2,
                            int rows, int N, int K, void* stream) {
    // two members over the same operands (the second one optional): exercises the descriptor walk of the grouped grid
    WgradGroup grp{};
    grp.n = dW2 ? 2 : 1;
    for (int i = 0; i < grp.n; ++i) {
        WgradDesc& d = grp.p[i];
        d.dy = (const bf16*)dy; d.x = (const bf16*)x; d.dW = i ? dW2 : dW; d.db = i ? db2 : db; d.lddy = (int)lddy; d.ldx = (int)ldx; d.rows = rows; d.N = N; d.K = K;
    }
    return mk_gemm_wgrad_grouped(grp, (hipStream_t)stream);
}
int masr_test_wgrad_grouped_n(const uint16_t* dy, int64_t lddy, const uint16_t* x, int64_t ldx, float* dW, int64_t member_stride, int members,
                              int first_members, int rows, int rows_rest, int N, int K, void* stream) {
    // `members` group members over the SAME operands (member i writes dW + i * member_stride; 0 = all into one buffer): what the grouped
    // launch costs when every panel is resident in L2 / the Infinity Cache (tools/wgrad_probe.py).  first_members > 0: the two-segment
    // tile list of the engine's merged launch -- members [0, first_members) reduce over `rows` rows and are dispatched first, the rest
    // over the first `rows_rest` rows
    WgradGroup grp{};
    grp.n = members < WGRAD_GROUP_MAX ? members : WGRAD_GROUP_MAX;
    for (int i = 0; i < grp.n; ++i) {
        WgradDesc& d = grp.p[i];
        d.dy = (const bf16*)dy; d.x = (const bf16*)x; d.dW = dW + (int64_t)i * member_stride; d.db = nullptr; d.lddy = (int)lddy; d.ldx = (int)ldx;
        d.rows = (first_members > 0 && i >= first_members) ? rows_rest : rows; d.N = N; d.K = K;
    }
    return mk_gemm_wgrad_grouped(grp, (hipStream_t)stream, first_members);
}
int masr_test_conv3x3_wgrad_pooled(const uint16_t* in, const uint16_t* dy_pooled, const uint8_t* pool_idx, float* dw, float* db, float* slab,
                                   int64_t slab_floats, int B, int H, int W, int CIN, int COUT, void* stream) {
    if (slab_floats < mk_conv3x3_wgrad_slab_floats(B, H, W, CIN, COUT)) { mk_set_error("masr_test_conv3x3_wgrad_pooled", "slab too small"); return -1; }
    ConvWgradArgs a{}; a.in = (const bf16*)in; a.dy_pooled = (const bf16*)dy_pooled; a.pool_idx = pool_idx; a.dw = dw; a.db = db; a.slab = slab;
    a.B = B; a.H = H; a.W = W; a.CIN = CIN; a.COUT = COUT;
    return mk_conv3x3_wgrad(a, (hipStream_t)stream);
}
int masr_test_attention_dropout_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o, uint16_t* dq, uint16_t* dk,
                                    uint16_t* dv, float* lse, const int32_t* klens, int B, int H, int Tq, int Tk, int hd, int causal, float drop_p,
                                    uint32_t seed, uint32_t site, void* stream) {
    const long E = (long)H * hd;
    AttnArgs a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ldq = a.ldk = a.ldv = E; a.o = (bf16*)o; a.ldo = E; a.lse = lse;
    a.klens = klens; a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = causal; a.drop_p = drop_p; a.seed = seed; a.site = site;
    CK(mk_attn_fwd(a, (hipStream_t)stream));
    a.dout = (const bf16*)dout; a.lddo = E; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.lddq = a.lddk = a.lddv = E;
    return mk_attn_bwd(a, (hipStream_t)stream);
}
int masr_test_attention_chunk(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o, uint16_t* dq, uint16_t* dk,
                              uint16_t* dv, float* lse, const int32_t* klens, int B, int H, int Tq, int Tk, int hd, int causal, float drop_p,
                              uint32_t seed, uint32_t site, int chunk, int left, const int32_t* chunk_dev, void* stream) {
    const long E = (long)H * hd;
    AttnArgs a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ldq = a.ldk = a.ldv = E; a.o = (bf16*)o; a.ldo = E; a.lse = lse;
    a.klens = klens; a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = causal; a.drop_p = drop_p; a.seed = seed; a.site = site;
    a.chunk = chunk; a.left = left; a.chunk_ptr = chunk_dev;
    CK(mk_attn_fwd(a, (hipStream_t)stream));
    a.dout = (const bf16*)dout; a.lddo = E; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.lddq = a.lddk = a.lddv = E;
    return mk_attn_bwd(a, (hipStream_t)stream);
}
int masr_test_attention(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* o, uint16_t* dq, uint16_t* dk,
                        uint16_t* dv, float* lse, float* delta, const int32_t* klens, int B, int H, int Tq, int Tk, int hd, int causal,
                        void* stream) {
    const long E = (long)H * hd;
    AttnArgs a{};
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.ldq = a.ldk = a.ldv = E; a.o = (bf16*)o; a.ldo = E; a.lse = lse;
    a.klens = klens; a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.hd = hd; a.causal = causal;
    CK(mk_attn_fwd(a, (hipStream_t)stream));
    if (dout) {
        a.dout = (const bf16*)dout; a.lddo = E; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.lddq = a.lddk = a.lddv = E; a.delta = delta;
        CK(mk_attn_bwd(a, (hipStream_t)stream));
    }
    return 0;
}

// ---- the streaming first pass's two kernels alone (tests/test_hip_stream_kernels.py)
int masr_test_attention_stream(const uint16_t* q, const uint16_t* knew, const uint16_t* vnew, uint16_t* kc, uint16_t* vc, uint16_t* o,
                               const int32_t* klens, int B, int H, int hd, int R, int pos, int lo, int cap, void* stream) {
    const long E = (long)H * hd;
    AttnStreamArgs a{};
    a.q = (const bf16*)q; a.ldq = E; a.knew = (const bf16*)knew; a.vnew = (const bf16*)vnew; a.ldnew = E;
    a.kc = (bf16*)kc; a.vc = (bf16*)vc; a.ldc = E; a.batch_stride = (long)cap * E; a.klens = klens; a.o = (bf16*)o; a.ldo = E;
    a.B = B; a.H = H; a.hd = hd; a.R = R; a.pos = pos; a.lo = lo; a.cap = cap;
    return mk_attn_stream(a, (hipStream_t)stream);
}
int masr_test_ctc_greedy_stream(const float* logits, int64_t ld, const int32_t* klens, int B, int R, int C, int pos, int32_t* state, int32_t* tokens,
                                int32_t* frames, int ld_out, void* stream) {
    CtcGreedyStreamArgs a{};
    a.logits = logits; a.ld = (long)ld; a.batch_stride = (long)R * ld; a.klens = klens; a.B = B; a.R = R; a.C = C; a.pos = pos;
    a.state = state; a.tokens = tokens; a.frames = frames; a.ld_out = ld_out;
    if (C > ld) { mk_set_error("masr_test_ctc_greedy_stream", "need C <= ld"); return -1; }
    return mk_ctc_greedy_stream(a, (hipStream_t)stream);
}

// ---- the BLSTM path's LSTM kernels alone (tests/test_hip_lstm_kernels.py)
static inline bool test_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int test_kp(int H) { return (H + 31) / 32 * 32; }
int masr_test_lstm_shadows(const float* wih, const float* whh, const float* bih, const float* bhh, int H, int K, int pc, int pd, uint16_t* wih16,
                           uint16_t* wihT16, uint16_t* whh16, uint16_t* whhT16, float* bias, void* stream) {
    const char* fn = "masr_test_lstm_shadows";
    if (!wih || !whh || !bih || !bhh || !wih16 || !wihT16 || !whh16 || !whhT16 || !bias) { mk_set_error(fn, "null pointer"); return -1; }
    if (H < 1 || K < 1 || pc < 0 || (pc > 0 && (pd < 1 || (int64_t)pc * pd != K))) { mk_set_error(fn, "need H, K >= 1 and, with pc > 0, K == pc * pd"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_lstm_shadows(wih, whh, bih, bhh, H, K, K, test_kp(H), (bf16*)wih16, (bf16*)wihT16, (bf16*)whh16, (bf16*)whhT16, bias, pc, pd, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_lstm_unperm(const float* src, float* dst, float* dst2, int H, int K, int pc, int pd, void* stream) {
    const char* fn = "masr_test_lstm_unperm";
    if (!src || !dst) { mk_set_error(fn, "null pointer"); return -1; }
    if (H < 1 || K < 1 || pc < 0 || (pc > 0 && (pd < 1 || (int64_t)pc * pd != K))) { mk_set_error(fn, "need H, K >= 1 and, with pc > 0, K == pc * pd"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_lstm_unperm(src, dst, dst2, H, K, pc, pd, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
// what both recurrence entries vet: sizes, lens in [1, T] (read back), the resident form's shapes
static int test_lstm_vet(const char* fn, int resident, int B, int T, int H, const int32_t* lens, bool bwd, hipStream_t s) {
    if (resident != 0 && resident != 1) { mk_set_error(fn, "resident must be 0 or 1"); return -1; }
    if (B < 1 || T < 1 || H < 1 || (int64_t)B * T * 4 * H > 0x7fffffffLL) { mk_set_error(fn, "need B, T, H >= 1 and B * T * 4H < 2^31"); return -1; }
    if (bwd && (4 * H) % 32) { mk_set_error(fn, "4H must be a multiple of 32"); return -1; }
    if (resident && !mk_lstm_rec_ok(B, H, test_kp(H))) { mk_set_error(fn, "shape not covered by the resident recurrence"); return -1; }
    std::vector<int> hl;
    CK(test_read_ints(lens, (size_t)B, hl, s));
    for (int n : hl) if (n < 1 || n > T) { mk_set_error(fn, "lens must lie in [1, T]"); return -1; }
    return 0;
}
// the entry's own scratch: h ping-pong bf16 [2][2][B][KP] | running state fp32 [2][B][H] | exchange words | the error word
struct TestLstmScratch {
    char* base = nullptr; bf16* h16[2][2]; float* cstate[2]; unsigned long long* words; int* err;
    int alloc(int B, int H, int KP, hipStream_t s) {
        const size_t hb = sizeof(bf16) * (size_t)B * KP, cb = sizeof(float) * (size_t)B * H, wb = sizeof(unsigned long long) * (size_t)mk_lstm_rec_words(B, H);
        const size_t hb_al = (hb + 255) / 256 * 256, cb_al = (cb + 255) / 256 * 256, wb_al = (wb + 255) / 256 * 256;
        const size_t total = wb_al + 4 * hb_al + 2 * cb_al + 256;
        HIP_CHECK_RET(hipMalloc(&base, total));
        if (hipMemsetAsync(base, 0, total, s) != hipSuccess) { mk_set_error("masr_test_lstm", "memset failed"); return -1; }
        char* p = base;
        words = reinterpret_cast<unsigned long long*>(p); p += wb_al;      // (the exchange words start the allocation: 16-byte loads through a buffer descriptor)
        for (int d = 0; d < 2; ++d) for (int i = 0; i < 2; ++i) { h16[d][i] = reinterpret_cast<bf16*>(p); p += hb_al; }
        for (int d = 0; d < 2; ++d) { cstate[d] = reinterpret_cast<float*>(p); p += cb_al; }
        err = reinterpret_cast<int*>(p);
        return 0;
    }
    ~TestLstmScratch() { if (base) hipFree(base); }
    // after the launch: the stream is drained, the error word read back
    int finish(const char* fn, int resident, hipStream_t s) {
        int e = 0;
        if (resident) HIP_CHECK_RET(hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        if (e != 0) { mk_set_error(fn, "the resident recurrence timed out waiting for a peer workgroup"); return -2; }
        return 0;
    }
};
int masr_test_lstm_fwd(int resident, int B, int T, int H, const int32_t* lens, const float* gx0, const float* gx1, const uint16_t* whh16_0,
                       const uint16_t* whh16_1, uint16_t* y16, float* act0, float* act1, float* c0, float* c1, void* stream) {
    const char* fn = "masr_test_lstm_fwd";
    if (!lens || !gx0 || !gx1 || !whh16_0 || !whh16_1 || !y16 || !act0 || !act1 || !c0 || !c1) { mk_set_error(fn, "null pointer"); return -1; }
    if (!test_al16(whh16_0) || !test_al16(whh16_1) || !test_al16(act0) || !test_al16(act1)) { mk_set_error(fn, "whh16 and act must be 16-byte aligned"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(test_lstm_vet(fn, resident, B, T, H, lens, false, s));
    const int KP = test_kp(H);
    TestLstmScratch w;
    CK(w.alloc(B, H, KP, s));
    LstmStepArgs a{}; a.B = B; a.T = T; a.H = H; a.KP = KP; a.lens = lens; a.y16 = (bf16*)y16;
    a.whh16[0] = (const bf16*)whh16_0; a.whh16[1] = (const bf16*)whh16_1; a.gx[0] = gx0; a.gx[1] = gx1; a.act[0] = act0; a.act[1] = act1; a.c[0] = c0; a.c[1] = c1;
    for (int d = 0; d < 2; ++d) { a.h16[d][0] = w.h16[d][0]; a.h16[d][1] = w.h16[d][1]; a.cstate[d] = w.cstate[d]; }
    if (resident) CK(mk_lstm_fwd_rec(a, w.words, w.err, s));
    else CK(mk_lstm_fwd_steps(a, s));
    return w.finish(fn, resident, s);
}
int masr_test_lstm_bwd(int resident, int B, int T, int H, const int32_t* lens, const float* dy, const float* act0, const float* act1, const float* c0,
                       const float* c1, const uint16_t* whhT16_0, const uint16_t* whhT16_1, uint16_t* dz16_0, uint16_t* dz16_1, void* stream) {
    const char* fn = "masr_test_lstm_bwd";
    if (!lens || !dy || !act0 || !act1 || !c0 || !c1 || !whhT16_0 || !whhT16_1 || !dz16_0 || !dz16_1) { mk_set_error(fn, "null pointer"); return -1; }
    if (!test_al16(whhT16_0) || !test_al16(whhT16_1) || !test_al16(act0) || !test_al16(act1) || !test_al16(dz16_0) || !test_al16(dz16_1)) {
        mk_set_error(fn, "whhT16, act and dz16 must be 16-byte aligned"); return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CK(test_lstm_vet(fn, resident, B, T, H, lens, true, s));
    const int KP = test_kp(H);
    TestLstmScratch w;
    CK(w.alloc(B, H, KP, s));
    LstmStepArgs a{}; a.B = B; a.T = T; a.H = H; a.KP = KP; a.lens = lens; a.dy = dy;
    a.whhT16[0] = (const bf16*)whhT16_0; a.whhT16[1] = (const bf16*)whhT16_1; a.act[0] = const_cast<float*>(act0); a.act[1] = const_cast<float*>(act1);
    a.c[0] = const_cast<float*>(c0); a.c[1] = const_cast<float*>(c1); a.dz16[0] = (bf16*)dz16_0; a.dz16[1] = (bf16*)dz16_1;
    for (int d = 0; d < 2; ++d) { a.h16[d][0] = w.h16[d][0]; a.h16[d][1] = w.h16[d][1]; a.cstate[d] = w.cstate[d]; }
    if (resident) CK(mk_lstm_bwd_rec(a, w.words, w.err, s));
    else CK(mk_lstm_bwd_steps(a, s));
    return w.finish(fn, resident, s);
}
int masr_test_lstm_hprev(const uint16_t* y16, uint16_t* hp0, uint16_t* hp1, int B, int T, int H, int KP, void* stream) {
    if (!y16 || !hp0 || !hp1 || B < 1 || T < 1 || H < 1 || KP < H) { mk_set_error("masr_test_lstm_hprev", "null pointer, B, T, H < 1 or KP < H"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_lstm_hprev((const bf16*)y16, (bf16*)hp0, (bf16*)hp1, B, T, H, KP, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_cast_rows_pad(const float* x, uint16_t* y, int64_t rows, int C, int Cp, void* stream) {
    if (!x || !y || rows < 1 || C < 1 || Cp < C) { mk_set_error("masr_test_cast_rows_pad", "null pointer, rows, C < 1 or Cp < C"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_cast_rows_pad(x, (bf16*)y, (long)rows, C, Cp, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_tanh(const float* x, const float* dy, float* y32, uint16_t* out16, int64_t n, void* stream) {
    if (!x || !out16 || (!dy && !y32) || n < 1) { mk_set_error("masr_test_tanh", "null pointer or n < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (dy) CK(mk_tanh_bwd(dy, x, (bf16*)out16, (long)n, s));
    else CK(mk_tanh_fwd(x, y32, (bf16*)out16, (long)n, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_mask_rows(float* x32, uint16_t* x16, const int32_t* lens, int B, int T, int C, void* stream) {
    if (!lens || B < 1 || T < 1 || C < 1) { mk_set_error("masr_test_mask_rows", "null lens or B, T, C < 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_mask_rows(x32, (bf16*)x16, lens, B, T, C, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_subsample_rows(const uint16_t* y, uint16_t* ys, const float* dys, float* dy, int B, int Tin, int Tout, int sub, int C, void* stream) {
    const char* fn = "masr_test_subsample_rows";
    if (dys ? !dy : (!y || !ys)) { mk_set_error(fn, "null pointer"); return -1; }
    if (B < 1 || Tin < 1 || C < 1) { mk_set_error(fn, "need B, Tin, C >= 1"); return -1; }
    if (dys ? (!test_al16(dys) || !test_al16(dy)) : (!test_al16(y) || !test_al16(ys))) { mk_set_error(fn, "operands must be 16-byte aligned"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (dys) CK(mk_subsample_rows_bwd(dys, dy, B, Tin, Tout, sub, C, s));
    else CK(mk_subsample_rows((const bf16*)y, (bf16*)ys, B, Tin, Tout, sub, C, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
// ---- the LSTM LM's step (nlm.hip)
int masr_test_nlm_step(const masr_nlm* nlm, int R, int K, int t, const int32_t* tok, const int32_t* par, const float* score, uint16_t* hstate,
                       float* cstate, float* logits, int64_t ld, float* logp, void* stream) {
    const char* fn = "masr_test_nlm_step";
    if (!nlm || !hstate || !cstate || !logits || (t > 1 && !tok)) { mk_set_error(fn, "null pointer"); return -1; }
    if (R < 1 || K < 1 || R % K || t < 1 || ld < nlm->dev.C || R > (1 << 20)) { mk_set_error(fn, "need 1 <= R <= 2^20, K >= 1, R % K == 0, t >= 1, ld >= C"); return -1; }
    if (!test_al16(hstate)) { mk_set_error(fn, "operands must be 16-byte aligned"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    char* w = nullptr;                                       // step[2] | htop [R][Hp]
    const size_t htop_off = 256, bytes = htop_off + sizeof(bf16) * (size_t)R * nlm->dev.Hp;
    HIP_CHECK_RET(hipMalloc(&w, bytes));
    const int h_step[2] = {t, 0};
    NlmStepArgs a{};
    a.step = (int*)w; a.R = R; a.K = K; a.tok_hist = tok; a.par_hist = par; a.hist_stride = 0; a.score = score;
    a.hstate = (bf16*)hstate; a.cstate = cstate; a.htop = (bf16*)(w + htop_off);
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemsetAsync(w, 0, bytes, s));
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        CK(mk_nlm_step(nlm->dev, a, logits, (long)ld, s));
        if (logp) CK(mk_nlm_logp(logits, (long)ld, R, nlm->dev.C, logp, (long)ld, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}
// the carry form of the same step (mk_nlm_step_carry)
int masr_test_nlm_step_carry(const masr_nlm* nlm, int R, int K, int t, const int32_t* tok, const int32_t* par, const int32_t* live, uint16_t* hstate,
                             float* cstate, float* logits, int64_t ld, float* logp, void* stream) {
    const char* fn = "masr_test_nlm_step_carry";
    if (!nlm || !hstate || !cstate || !logits || !logp || !tok || !par || !live) { mk_set_error(fn, "null pointer"); return -1; }
    if (R < 1 || K < 1 || R % K || t < 1 || ld < nlm->dev.C || R > (1 << 20)) { mk_set_error(fn, "need 1 <= R <= 2^20, K >= 1, R % K == 0, t >= 1, ld >= C"); return -1; }
    if (!test_al16(hstate)) { mk_set_error(fn, "operands must be 16-byte aligned"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    char* w = nullptr;                                       // step[2] | htop [R][Hp]
    const size_t htop_off = 256, bytes = htop_off + sizeof(bf16) * (size_t)R * nlm->dev.Hp;
    HIP_CHECK_RET(hipMalloc(&w, bytes));
    const int h_step[2] = {t, 0};
    NlmStepArgs a{};
    a.step = (int*)w; a.R = R; a.K = K; a.tok_hist = tok; a.par_hist = par; a.hist_stride = 0; a.live = live;
    a.hstate = (bf16*)hstate; a.cstate = cstate; a.htop = (bf16*)(w + htop_off);
    auto run = [&]() -> int {
        HIP_CHECK_RET(hipMemsetAsync(w, 0, bytes, s));
        HIP_CHECK_RET(hipMemcpyAsync(w, h_step, sizeof h_step, hipMemcpyHostToDevice, s));
        CK(mk_nlm_step_carry(nlm->dev, a, logits, (long)ld, logp, (long)ld, (int*)w, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(w);
    return rc;
}

// ---- the flat optimiser passes and the shadow kernels alone (optim.hip)
static int test_flat_n(const char* fn, int64_t n) {
    if (n < 1 || n > (int64_t)1 << 40) { mk_set_error(fn, "n outside [1, 2^40]"); return -1; }
    return 0;
}
int masr_test_sumsq(const float* x, int64_t n, float* out_norm, void* stream) {
    const char* fn = "masr_test_sumsq";
    if (!x || !out_norm) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    if ((uintptr_t)x & 15) { mk_set_error(fn, "x must be 16-byte aligned (the kernel reads float4 at every multiple of four floats)"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    float* slab = nullptr;
    HIP_CHECK_RET(hipMalloc(&slab, sizeof(float) * (size_t)mk_sumsq_slab_floats((long)n)));
    auto run = [&]() -> int {
        CK(mk_sumsq(x, (long)n, slab, out_norm, s));
        HIP_CHECK_RET(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = run();
    hipFree(slab);
    return rc;
}
int masr_test_clip_sgd(float* p, const float* g, float* mom, int64_t n, const float* norm, float max_norm, float lr, float momentum, int nesterov,
                       int step_flags, void* stream) {
    const char* fn = "masr_test_clip_sgd";
    if (!p || !g) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    if (step_flags < 0 || step_flags > 3) { mk_set_error(fn, "step_flags outside 0..3"); return -1; }
    if (!mom && momentum != 0.f && step_flags != 3) { mk_set_error(fn, "mom may be null only with momentum == 0 or step_flags == 3"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_clip_sgd(p, g, mom, (long)n, norm, max_norm, lr, momentum, nesterov, step_flags, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_clip_axpy(float* acc, const float* g, int64_t n, const float* norm, float max_norm, int nan_zero, void* stream) {
    const char* fn = "masr_test_clip_axpy";
    if (!acc || !g || !norm) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    hipStream_t s = (hipStream_t)stream;
    CK(mk_clip_axpy(acc, g, (long)n, norm, max_norm, s, nan_zero != 0));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_clip_scale(float* g, int64_t n, const float* norm, float max_norm, int nan_zero, void* stream) {
    const char* fn = "masr_test_clip_scale";
    if (!g || !norm) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    hipStream_t s = (hipStream_t)stream;
    CK(mk_clip_scale(g, (long)n, norm, max_norm, s, nan_zero != 0));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_adam_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr_a, int t_a, float lr_b, int t_b, float b1, float b2,
                           float eps, float weight_decay, int decoupled, const float* norm, int32_t* flags, int slot, void* stream) {
    const char* fn = "masr_test_adam_guarded";
    if (!p || !g || !m || !v || !norm || !flags) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    if (slot < 0 || slot > 1) { mk_set_error(fn, "slot must be 0 or 1"); return -1; }
    if (t_a < 1 || t_b < 1) { mk_set_error(fn, "step numbers start at 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_adam_guarded(p, g, m, v, (long)n, lr_a, t_a, lr_b, t_b, b1, b2, eps, weight_decay, decoupled, norm, flags, slot, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_shadow_jobs(const float* P, int n_jobs, const int64_t* desc, void* const* outs, void* stream) {
    const char* fn = "masr_test_shadow_jobs";
    if (!P || !desc || !outs) { mk_set_error(fn, "null pointer"); return -1; }
    if ((uintptr_t)P & 15) { mk_set_error(fn, "P must be 16-byte aligned"); return -1; }
    if (n_jobs < 1 || n_jobs > SHADOW_JOBS_MAX) { mk_set_error(fn, "n_jobs outside [1, SHADOW_JOBS_MAX]"); return -1; }
    ShadowJobs J{};
    for (int i = 0; i < n_jobs; ++i) {
        const int64_t* r = desc + 7 * (size_t)i;
        const int64_t src = r[0], type = r[1], N = r[2], K = r[3], ldt = r[4], a0 = r[5], a1 = r[6];
        void* p0 = outs[2 * i]; void* p1 = outs[2 * i + 1];
        if (type < SH_LINEAR || type > SH_COPY32) { mk_set_error(fn, "job type outside 0..3"); return -1; }
        if (src < 0) { mk_set_error(fn, "negative src"); return -1; }
        const int64_t lim = 1 << 24;                             // (every product below stays far inside an int)
        if (N < 1 || N > lim) { mk_set_error(fn, "non-positive (or oversized) N"); return -1; }
        if (type == SH_LINEAR || type == SH_CONV) {
            if (K < 1 || K > lim || N * K * 9 > 0x7fffffffLL) { mk_set_error(fn, "non-positive (or oversized) K"); return -1; }
        }
        if (type == SH_LINEAR) {
            if (src < 4) { mk_set_error(fn, "a Linear job needs src >= 4 (the tile pass reads up to three floats in front of a row)"); return -1; }
            if (ldt < N || ldt > lim) { mk_set_error(fn, "a Linear job needs ldt >= N"); return -1; }
        }
        if (type == SH_VGG2ENC) {
            if (a0 < 1 || a1 < 1 || a0 > lim || a1 > lim || a0 * a1 > lim || N * a0 * a1 > 0x7fffffffLL) { mk_set_error(fn, "non-positive (or oversized) a0 / a1"); return -1; }
        }
        if (!p0 || (type != SH_COPY32 && !p1)) { mk_set_error(fn, "null output of a job that writes it"); return -1; }
        ShadowDesc d{}; d.src = (long)src; d.type = (int)type; d.N = (int)N; d.K = (int)K; d.ldt = (int)ldt; d.a0 = (int)a0; d.a1 = (int)a1;
        d.tile_start = J.blocks;
        J.blocks += mk_shadow_blocks(d);
        J.d[J.n] = d; J.p[2 * J.n] = (bf16*)p0; J.p[2 * J.n + 1] = (bf16*)p1; ++J.n;
    }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_all_shadows(P, J, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_transpose_cast_bf16(const float* x, uint16_t* y, int R, int C, int64_t ldy, void* stream) {
    const char* fn = "masr_test_transpose_cast_bf16";
    if (!x || !y) { mk_set_error(fn, "null pointer"); return -1; }
    if (R < 1 || C < 1 || ldy < R) { mk_set_error(fn, "need R, C >= 1 and ldy >= R"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_transpose_cast_bf16(x, (bf16*)y, R, C, (long)ldy, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_cast_bf16(const float* x, uint16_t* y, int64_t n, void* stream) {
    const char* fn = "masr_test_cast_bf16";
    if (!x || !y) { mk_set_error(fn, "null pointer"); return -1; }
    CK(test_flat_n(fn, n));
    hipStream_t s = (hipStream_t)stream;
    CK(mk_cast_bf16(x, (bf16*)y, (long)n, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
int masr_test_conv_weight_shadows(const float* w, uint16_t* wk, uint16_t* wd, int CO, int CI, void* stream) {
    const char* fn = "masr_test_conv_weight_shadows";
    if (!w || !wk) { mk_set_error(fn, "null pointer"); return -1; }
    if (CO < 1 || CI < 1 || (int64_t)CO * CI * 9 > 0x7fffffffLL) { mk_set_error(fn, "need CO, CI >= 1 and CO CI 9 < 2^31"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    CK(mk_conv_weight_shadows(w, (bf16*)wk, (bf16*)wd, CO, CI, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}
// ---- the CTC loss kernels alone (ctc.hip; tests/test_hip_ctc_loss_kernels.py)
int masr_test_ctc_loss_layout(const float* logits, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int T,
                              int B, int C, int blank, float* nll, float* loss, float* grad, float* work, int maxS, void* stream, int batch_first) {
    return mk_ctc_loss(logits, targets, tgt_off, in_len, tgt_len, T, B, C, blank, nll, loss, grad, work, maxS, (hipStream_t)stream, batch_first != 0);
}
int masr_test_ctc_loss_joint(const float* logits, int64_t ld, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len,
                             const int32_t* tgt_len, int T, int B, int C, float* nll, uint16_t* grad16, float w, float* stats, float* work, int maxS,
                             void* stream) {
    const char* fn = "masr_test_ctc_loss_joint";
    if (!logits || !targets || !tgt_off || !in_len || !tgt_len || !nll || !stats || !work) { mk_set_error(fn, "null pointer"); return -1; }
    if (T < 1 || B < 1 || C < 1 || maxS < 1) { mk_set_error(fn, "need T, B, C, maxS >= 1"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    // this path has no device-side status word (the engine vets its batch on the host): what the kernels would index with is vetted here
    std::vector<int> il, tl, off, tg;
    CK(test_read_ints(in_len, (size_t)B, il, s));
    CK(test_read_ints(tgt_len, (size_t)B, tl, s));
    CK(test_read_ints(tgt_off, (size_t)B, off, s));
    for (int b = 0; b < B; ++b) {
        if (il[b] < 0 || il[b] > T || tl[b] < 0) { mk_set_error(fn, "in_len outside [0, T] or a negative tgt_len"); return -1; }
        if (tl[b] > (maxS - 1) / 2) { mk_set_error(fn, "target longer than the lattice the work buffer holds (2 tgt_len + 1 > maxS)"); return -1; }
        if (off[b] < 0) { mk_set_error(fn, "negative target offset"); return -1; }
    }
    for (int b = 0; b < B; ++b) {
        if (tl[b] == 0) continue;
        CK(test_read_ints(targets + off[b], (size_t)tl[b], tg, s));
        for (int v : tg) if (v < 1 || v >= C) { mk_set_error(fn, "target id outside [1, C)"); return -1; }
    }
    CK(mk_ctc_loss_joint(logits, (long)ld, targets, tgt_off, in_len, tgt_len, T, B, C, nll, (bf16*)grad16, w, stats, work, maxS, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
