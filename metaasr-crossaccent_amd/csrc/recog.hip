// libmasr engine, the decoders (MyTransformer.recog, mono_transformer_torch.py:143-176, and the beam searches of beam.hip): the
// literal whole-prefix re-decode, the KV-cached greedy decode, the attention beam and the joint CTC/attention beam.  Each of the
// last three captures the launch sequence of ONE step into a hipGraph of its own and replays it once per step (run_steps).  Behind them
// the two decoders without steps: the CTC prefix beam on the head alone, and attention rescoring of its N-best (one teacher-forced
// decoder pass) -- each also with the n-gram LM fused into the prefix beam -- and the forced alignment of a known
// transcript on the head.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "engine_internal.h"
#include "lm.h"
#include "nlm.h"
#include "bias.h"
#include "../../include/masr_test.h"

// The decoder layers of one incremental decode step on `rows` query rows (greedy: one per utterance; beam: B*K hypotheses): input
// a.y32[0] / a.y16[0], output a.y32[ND].  Self-attention keys/values of earlier positions live in d.qkv ([rows][slots][3E]);
// src (beam) maps row r's key j to the cache row that holds it; cross-attention row r reads utterance r / rows_per_utt.
struct DecStepGeom { int rows, slots, rows_per_utt; bf16* step_qkv; const int* src; long src_flip; };
static int decode_layers(Ctx& c, const DecStepGeom& gm) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s; const float* P = m->P;
    const int E = m->E, Fi = m->Fi, B = gm.rows;
    auto lin = [&](const bf16* x, long ldx, const bf16* wk, int N, int K, const float* bias) {
        SkinnyArgs g{}; g.A = x; g.lda = ldx; g.W = wk; g.ldw = K; g.M = B; g.N = N; g.K = K; g.bias = bias; return g;
    };
    auto att = [&]() { AttnDecodeArgs t{}; t.B = B; t.H = m->H; t.hd = m->hd; t.ldo = E; return t; };
    for (int l = 0; l < m->ND; ++l) {
        DecAct& d = a.dec[l]; const DecL& w = m->dec[l];
        // causal self-attention: keys/values of earlier positions live in d.qkv ([B][Ldec][3E], the layout of the full decode)
        SkinnyArgs g = lin(a.y16[l], E, w.sa.in.k16, 3 * E, E, P + w.sa.in.b); g.C16 = gm.step_qkv; g.ldc16 = 3 * E;
        CK(mk_skinny_gemm(g, s));
        AttnDecodeArgs t = att();
        t.q = gm.step_qkv; t.ldq = 3 * E; t.k = d.qkv + E; t.v = d.qkv + 2 * E; t.ldk = 3 * E; t.kv_batch_stride = (long)gm.slots * 3 * E;
        t.knew = gm.step_qkv + E; t.vnew = gm.step_qkv + 2 * E; t.ldnew = 3 * E; t.step = a.step_dev; t.o = d.ao; t.Tk_cap = gm.slots;
        t.src = gm.src; t.ld_src = gm.slots; t.src_flip = gm.src_flip;
        CK(mk_attn_decode(t, s));
        g = lin(d.ao, E, w.sa.out.k16, E, E, P + w.sa.out.b); g.residual = a.y32[l]; g.ldres = E; g.C32 = d.s1; g.ldc = E;
        CK(mk_skinny_gemm(g, s));
        CK(ln_fwd(c, w.n1, d.s1, d.y1_32, d.y1_16, d.m1, d.r1, B));
        // cross-attention over the encoder memory: d.kv was projected once, before the first step
        g = lin(d.y1_16, E, w.ca.q_k16, E, E, P + w.ca.in.b); g.C16 = d.q; g.ldc16 = E;
        CK(mk_skinny_gemm(g, s));
        t = att();
        t.q = d.q; t.ldq = E; t.k = d.kv; t.v = d.kv + E; t.ldk = m->NK; t.kv_batch_stride = (long)a.Tp * m->NK;
        t.klens = a.enc_lens; t.o = d.co; t.Tk_cap = a.Tp; t.rows_per_utt = gm.rows_per_utt;
        CK(mk_attn_decode(t, s));
        g = lin(d.co, E, w.ca.out.k16, E, E, P + w.ca.out.b); g.residual = d.y1_32; g.ldres = E; g.C32 = d.s2; g.ldc = E;
        CK(mk_skinny_gemm(g, s));
        CK(ln_fwd(c, w.n2, d.s2, d.y2_32, d.y2_16, d.m2, d.r2, B));
        g = lin(d.y2_16, E, w.l1.k16, Fi, E, P + w.l1.b); g.relu = 1; g.C16 = d.f; g.ldc16 = Fi;
        CK(mk_skinny_gemm(g, s));
        g = lin(d.f, Fi, w.l2.k16, E, Fi, P + w.l2.b); g.residual = d.y2_32; g.ldres = E; g.C32 = d.s3; g.ldc = E;
        CK(mk_skinny_gemm(g, s));
        CK(ln_fwd(c, w.n3, d.s3, a.y32[l + 1], a.y16[l + 1], d.m3, d.r3, B));
    }
    // the last projection in fp32 on the master weights (a selection follows: mk_logits_f32); layer 0's pre-LayerNorm sum is free by now
    float* yf32 = a.dec[0].s1;
    CK(ln_fwd(c, m->dec_norm, a.y32[m->ND], yf32, nullptr, a.mdf, a.rdf, B));
    CK(mk_logits_f32(yf32, P + m->ct.w, P + m->ct.b, a.logits, m->Cp, B, m->C, E, s));
    return 0;
}

// One incremental decode step (the newest target position of every utterance) -- SURVEY 8(f).1.  Every launch below has
// step-independent arguments; the step itself lives in *a.step_dev, so the sequence is captured once and replayed.
static int decode_step(Ctx& c, int* out) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s; const float* P = m->P;
    const int E = m->E, B = a.B;
    CK(mk_recog_embed_step(a.step_dev, out, P + m->embed_w, m->pe, a.y32[0], a.y16[0], B, E, 0, s));
    CK(decode_layers(c, DecStepGeom{B, a.L, 1, a.step_qkv, nullptr, 0}));
    CK(mk_recog_argmax_step(a.step_dev, a.logits, m->Cp, out, B, m->C, s));       // also advances *step_dev
    return 0;
}

// `n` decode steps on stream s; step() enqueues the launches of one.  Direct launches on the legacy NULL stream, while profiling, or with
// MASR_RECOG_NO_GRAPH set (read on every call).  Otherwise the step is captured once per key (key: shape, key_ptr: the buffers its launches
// were given) into `gc` and replayed n times; a new key waits for the last replay of the old graph before that is destroyed.
template <class Step>
static int run_steps(masr_model* m, DecodeGraph& gc, const int (&key)[6], const void* const (&key_ptr)[3], int n, hipStream_t s, const char* fn,
                     const char* capture_err, Step step) {
    const bool use_graph = s != nullptr && !m->prof && !getenv("MASR_RECOG_NO_GRAPH");
    if (!use_graph) {
        for (int i = 0; i < n; ++i) CK(step());
        return 0;
    }
    const bool hit = gc.exec && !memcmp(key, gc.key, sizeof key) && !memcmp(key_ptr, gc.key_ptr, sizeof key_ptr);
    if (!hit) {
        if (gc.done) HIP_CHECK_RET(hipEventSynchronize(gc.done));      // no replay of the old graph in flight
        else HIP_CHECK_RET(hipEventCreateWithFlags(&gc.done, hipEventDisableTiming));
        if (gc.exec) { hipGraphExecDestroy(gc.exec); gc.exec = nullptr; }
        if (gc.graph) { hipGraphDestroy(gc.graph); gc.graph = nullptr; }
        HIP_CHECK_RET(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = step();
        const hipError_t e = hipStreamEndCapture(s, &gc.graph);
        if (rc || e != hipSuccess) { mk_set_error(fn, capture_err); return -1; }
        HIP_CHECK_RET(hipGraphInstantiate(&gc.exec, gc.graph, nullptr, nullptr, 0));
        memcpy(gc.key, key, sizeof key); memcpy(gc.key_ptr, key_ptr, sizeof key_ptr);
    }
    for (int i = 0; i < n; ++i) HIP_CHECK_RET(hipGraphLaunch(gc.exec, s));
    HIP_CHECK_RET(hipEventRecord(gc.done, s));
    return 0;
}

// argument checks of the entry points: 0, or -1 with the message recorded under the caller's name
static int fail(const char* fn, const char* msg) { mk_set_error(fn, msg); return -1; }
static int check_model(const char* fn, const masr_model* m) { return m ? 0 : fail(fn, "null model"); }
static int check_ctc_head(const char* fn, const masr_model* m) { return m->ctc_w > 0.f ? 0 : fail(fn, "the model has no CTC head (masr_create_ctc)"); }
static int check_beam_size(const char* fn, int K) { return K >= 1 && K <= 64 ? 0 : fail(fn, "beam size K must be in [1, 64]"); }
// `name`: what the entry point calls its list length (nbest in the CTC beam's, N elsewhere)
static int check_nbest(const char* fn, const char* name, int N, int K) {
    return N >= 1 && N <= K ? 0 : fail(fn, (std::string(name) + " must be in [1, K]").c_str());
}
// a weight is finite and, strict, > 0, else >= 0
static int check_weight(const char* fn, const char* name, float v, bool strict) {
    if (std::isfinite(v) && (strict ? v > 0.f : v >= 0.f)) return 0;
    return fail(fn, (std::string(name) + " must be finite and " + (strict ? "> 0" : ">= 0")).c_str());
}
// What is fused into a search: an LM (n-gram or LSTM, at most one) with its weight and the bonus per emitted token, and a phrase list (DESIGN
// 5.13, 5.14) with its weight and where the hypotheses' credited tokens (n_final) go.  Null pointers: not fused.
struct Fusion {
    const masr_lm* lm = nullptr; const masr_nlm* nlm = nullptr; float lm_w = 0.f, len_bonus = 0.f;
    const masr_bias* bias = nullptr; float bias_w = 0.f; int32_t* nbias = nullptr;
};
static Fusion fuse_lm(const masr_lm* lm, float lm_w, float len_bonus = 0.f) { Fusion f; f.lm = lm; f.lm_w = lm_w; f.len_bonus = len_bonus; return f; }
static Fusion fuse_nlm(const masr_nlm* nlm, float lm_w, float len_bonus = 0.f) { Fusion f; f.nlm = nlm; f.lm_w = lm_w; f.len_bonus = len_bonus; return f; }
static Fusion fuse_bias(Fusion f, const masr_bias* bias, float bias_w, int32_t* nbias) { f.bias = bias; f.bias_w = bias_w; f.nbias = nbias; return f; }
static int check_bias(const char* fn, const masr_model* m, const Fusion& f) {
    if (!f.bias) return fail(fn, "null phrase list");
    if (f.bias->dev.C != m->C) return fail(fn, "the phrase list's classes differ from the model's odim");
    return check_weight(fn, "bias_w", f.bias_w, false);
}
// LM fusion: the LM of either kind, its weight and, where the search has one (with_bonus), the per-token bonus
static int check_lm(const char* fn, const masr_model* m, const Fusion& f, bool with_bonus) {
    if (!f.lm && !f.nlm) return fail(fn, "null language model");
    if ((f.lm ? f.lm->dev.C : f.nlm->dev.C) != m->C) return fail(fn, "the language model's classes differ from the model's odim");
    CK(check_weight(fn, "lm_w", f.lm_w, false));
    return !with_bonus || std::isfinite(f.len_bonus) ? 0 : fail(fn, "len_bonus must be finite");
}
static int check_pointers(const char* fn, const float* xs, const int64_t* ilens, const int32_t* tokens, const int32_t* lens, const float* scores) {
    return xs && ilens && tokens && lens && scores ? 0 : fail(fn, "null pointer");
}
// every ilens[b] in [4, T]; each(b, enc) gets the encoder length ilens[b] / 4 of the utterances up to the first that is not
template <class Each>
static int check_ilens(const char* fn, const int64_t* ilens, int B, int T, Each each) {
    for (int b = 0; b < B; ++b) {
        if (ilens[b] < 4 || ilens[b] > T) return fail(fn, "ilens must be in [4, T]");
        each(b, (int)(ilens[b] / 4));
    }
    return 0;
}
// what the workspace queries need: every beam's, the rescoring's, the alignment's (how each says so: DecodeSpec::need)
static bool shape_ok(int B, int T, int K) { return B > 0 && T >= 4 && K >= 1 && K <= 64; }
static bool rescore_shape_ok(int B, int T, int K, int N, int Lmax) { return shape_ok(B, T, K) && N >= 1 && N <= K && Lmax >= 0 && Lmax < MASR_PE_ROWS; }
static bool align_shape_ok(int B, int T, int maxL) { return B > 0 && T >= 4 && maxL >= 0 && 2 * (int64_t)maxL + 1 <= 2048; }

// What a decoder plans into the arena: the activations, then its own state behind them.  plan_decode both sizes the workspace (a null
// arena) and places the buffers in the bound one.
// A spec is built by the constructor of its kind alone, which also sets the texts of the public query that sizes the workspace for it (and is
// answered from the same spec): `query`, the call, and `need`, its refusal of arguments out of range.
//   greedy (greedy_spec): Ldec decoder positions per utterance, nothing else
//   beam (step_beam_spec, G_BEAM: masr_recog_beam): K*Lmax decoder positions per utterance = Lmax slots for each of the B*K hypothesis rows, then the beam state
//   LM fusion (step_beam_spec, G_LM: masr_recog_beam_lm, fused): the beam's plan, then the fp32 fused rows [B*K][Cp]
//   LSTM LM fusion (step_beam_spec, G_NLM: masr_recog_beam_nlm, fused, nlm): the beam's plan, then the fused rows, the LM logits [B*K][Cp], the
//   LM's states h bf16 and c fp32 [2][L][B*K][Hp] each, and the top layer's new h [B*K][Hp]
//   joint CTC/attention (step_beam_spec, G_JOINT: masr_recog_beam_ctc, P = floor(3K/2) > 0): the row lists are P long, and the CTC head's
//   logits [B*Tp][Cp], its log-probs [B][C][Tp] and the candidates' prefix states [2][R][Tp][P] follow everything else
//   joint with LM, bonus and N-best (step_beam_spec, G_JOINT_LM: masr_recog_beam_ctc_lm, P > 0, fused, NB > 0): both of the above, then the
//   candidates' LM terms [R][P], the four weights and the N-best list [B][NB]
//   joint with the LSTM LM (step_beam_spec, G_JOINT_NLM: masr_recog_beam_ctc_nlm, P > 0, fused, nlm, NB > 0): the joint LM beam's plan with
//   the LSTM LM fusion's buffers behind the shared fused rows
//   phrase biasing of either step beam (step_beam_spec, G_BIAS / G_JOINT_BIAS: masr_recog_beam_bias, masr_recog_beam_ctc_bias, bias; DESIGN
//   5.14): the LM variant's plan -- the fused rows are needed without an LM too -- then the automaton states [2][R] and, in the joint beam,
//   the candidates' bias terms [R][P]; the joint beam's weights are five
//   CTC-only beam (ctc_beam_spec: masr_recog_ctc_beam and its _lm / _bias forms): one decoder position per utterance; the head's logits
//   [B*Tp][Cp] and the search's work buffer follow -- with the LSTM LM (masr_recog_ctc_beam_nlm, nlm) the larger one of
//   masr_ctc_beam_nlm_work_bytes, here and in the first pass of the rescoring plan
//   attention rescoring (rescore_spec: masr_recog_rescore* / masr_rescore_nbest, N > 0): N * (Lmax + 1) decoder positions per utterance = the
//   B*N hypotheses of up to Lmax tokens behind their sos; with a first pass (K > 0) the CTC-only beam's buffers and its N-best list follow,
//   then the second pass's scores
//   CTC forced alignment (align_spec: masr_recog_ctc_align): one decoder position per utterance; the head's logits, the targets [B*maxL] with
//   their offsets [B] and lengths [B], and the alignment's work buffer follow
enum class Decoder { greedy, step_beam, ctc_beam, rescore, align };
struct DecodeSpec {
    Decoder kind; const char *query, *need;
    int K = 0, Lmax = 0, P = 0, NB = 0, N = 0, maxL = 0; bool fused = false, bias = false; const masr_nlm* nlm = nullptr;
    std::string too_small() const { return std::string("workspace too small (") + query + ")"; }
};
static int beam_prebeam_width(int K) { return 3 * K / 2; }         // ESPnet's CTC_SCORING_RATIO 1.5

// the step beams, one row per graph slot G_BEAM .. G_JOINT_BIAS: the slot's workspace query and what its search has
struct BeamVariant { const char* query; bool joint, nbest, fused, bias; };
static const BeamVariant BEAM_VARIANTS[] = {
    {"masr_beam_workspace_bytes(B, T, K, Lmax)", false, false, false, false},
    {"masr_beam_ctc_workspace_bytes(B, T, K, Lmax)", true, false, false, false},
    {"masr_beam_lm_workspace_bytes(B, T, K, Lmax)", false, false, true, false},
    {"masr_beam_nlm_workspace_bytes(nlm, B, T, K, Lmax)", false, false, true, false},
    {"masr_beam_ctc_lm_workspace_bytes(B, T, K, N, Lmax)", true, true, true, false},
    {"masr_beam_ctc_nlm_workspace_bytes(nlm, B, T, K, N, Lmax)", true, true, true, false},
    {"masr_beam_bias_workspace_bytes(B, T, K, Lmax)", false, false, true, true},
    {"masr_beam_ctc_bias_workspace_bytes(B, T, K, N, Lmax)", true, true, true, true},
};
static const BeamVariant& beam_variant(GraphSlot g) { return BEAM_VARIANTS[g - G_BEAM]; }

static DecodeSpec greedy_spec() { return DecodeSpec{Decoder::greedy, "masr_workspace_bytes(B, T, max(ilens)/4)", ""}; }
// N: the length of the N-best list where the slot has one; nlm: the LSTM LM of G_NLM and G_JOINT_NLM
static DecodeSpec step_beam_spec(GraphSlot g, int K, int Lmax, int N, const masr_nlm* nlm) {
    const BeamVariant& v = beam_variant(g);
    DecodeSpec d{Decoder::step_beam, v.query, v.nbest ? "need B >= 1, T >= 4, 1 <= N <= K <= 64, Lmax >= 1" : "need B >= 1, T >= 4, 1 <= K <= 64, Lmax >= 1"};
    d.K = K; d.Lmax = Lmax; d.P = v.joint ? beam_prebeam_width(K) : 0; d.NB = v.nbest ? N : 0; d.fused = v.fused; d.bias = v.bias; d.nlm = nlm;
    return d;
}
static DecodeSpec ctc_beam_spec(int K, const masr_nlm* nlm) {        // (an n-gram LM or a phrase list in the search changes nothing of the plan)
    DecodeSpec d{Decoder::ctc_beam, nlm ? "masr_ctc_beam_nlm_workspace_bytes(nlm, B, T, K)" : "masr_ctc_beam_workspace_bytes(B, T, K)",
                 "need B >= 1, T >= 4, 1 <= K <= 64"};
    d.K = K; d.nlm = nlm; return d;
}
static DecodeSpec rescore_spec(int K, int N, int Lmax, const masr_nlm* nlm) {      // K = 0: no first pass (masr_rescore_nbest)
    DecodeSpec d{Decoder::rescore, nlm ? "masr_rescore_nlm_workspace_bytes(nlm, B, T, K, N, Lmax), Lmax >= the longest hypothesis"
                                       : "masr_rescore_workspace_bytes(B, T, K, N, Lmax), Lmax >= the longest hypothesis",
                 "need B >= 1, T >= 4, 1 <= N <= K <= 64, 0 <= Lmax < 3000"};
    d.K = K; d.N = N; d.Lmax = Lmax; d.nlm = nlm; return d;
}
static DecodeSpec align_spec(int maxL) {
    DecodeSpec d{Decoder::align, "masr_ctc_align_workspace_bytes(B, T, maxL)", "need B >= 1, T >= 4, maxL >= 0 and 2 * maxL + 1 <= 2048"};
    d.maxL = maxL; return d;
}
struct DecodeBufs {
    BeamArgs beam; bf16* step_qkv; float* ctc_logits; void* work; int64_t work_bytes;
    float* lm_fused;                                                    // LM fusion: the rows' fused increments [R][Cp]
    float* nlm_logits; bf16 *nlm_h, *nlm_htop; float* nlm_c;            // LSTM LM fusion: LM logits [R][Cp], states [2][L][R][Hp], top h [R][Hp]
    int *rs_tok, *rs_lens; float *rs_ctc, *rs_att, *rs_row_lp;          // rescoring: first-pass list [B][N][Tp] / [B][N] / [B][N], att [B*N], row terms [B*N*(Lmax+1)]
    int* al_tgt;                                                        // alignment: targets [B*maxL], then tgt_off [B], then tgt_len [B]
    int2* bias_state; float* bias_pre;                                  // phrase biasing: states [2][R], the joint beam's bias terms [R][P]
};

static DecodeBufs plan_beam(const masr_model* m, Arena& ar, int B, int Tp, const DecodeSpec& d) {
    const int R = B * d.K, L = d.Lmax, P = d.P, W = P ? P : d.K;
    DecodeBufs o{};
    BeamArgs& a = o.beam;
    a.B = B; a.K = d.K; a.R = R; a.Lmax = L; a.C = m->C; a.sos = 0; a.eos = m->C - 1;
    o.step_qkv = ar.get<bf16>((int64_t)R * 3 * m->E);
    a.tab = ar.get<int>(2 * (int64_t)R * L);
    a.tok_hist = ar.get<int>((int64_t)L * R); a.par_hist = ar.get<int>((int64_t)L * R);
    a.score = ar.get<float>(R);
    a.list_tok = ar.get<int>((int64_t)R * W); a.list_score = ar.get<float>((int64_t)R * W);
    int* lens = ar.get<int>(2 * (int64_t)B); a.maxlen = lens; a.minlen = lens + B;
    a.fin = ar.get<int>(B); a.best_score = ar.get<float>(B); a.best_len = ar.get<int>(B); a.best_row = ar.get<int>(B);
    if (d.fused) o.lm_fused = ar.get<float>((int64_t)R * m->Cp);
    if (d.nlm) {
        o.nlm_logits = ar.get<float>((int64_t)R * m->Cp);
        o.nlm_h = ar.get<bf16>(nlm_state_elems(d.nlm->dev, R)); o.nlm_c = ar.get<float>(nlm_state_elems(d.nlm->dev, R));
        o.nlm_htop = ar.get<bf16>((int64_t)R * d.nlm->dev.Hp);
    }
    if (d.bias) o.bias_state = ar.get<int2>(2 * (int64_t)R);
    if (!P) return o;
    a.P = P; a.Tp = Tp;
    o.ctc_logits = ar.get<float>((int64_t)B * Tp * m->Cp);
    a.ctc_lp = ar.get<float>((int64_t)B * m->C * Tp);
    a.ctc_state = ar.get<float2>(2 * (int64_t)R * Tp * P);
    a.psi = ar.get<float>(R); a.src = ar.get<int>(R);
    a.pre_tok = ar.get<int>((int64_t)R * P); a.pre_lp = ar.get<float>((int64_t)R * P);
    a.list_slot = ar.get<int>((int64_t)R * P); a.list_psi = ar.get<float>((int64_t)R * P);
    if (!d.NB) return o;
    a.N = d.NB;
    a.pre_lm = ar.get<float>((int64_t)R * P); a.wts = ar.get<float>(d.bias ? 5 : 4);
    if (d.bias) o.bias_pre = ar.get<float>((int64_t)R * P);
    a.nb_score = ar.get<float>((int64_t)B * d.NB); a.nb_len = ar.get<int>((int64_t)B * d.NB); a.nb_row = ar.get<int>((int64_t)B * d.NB);
    return o;
}
static DecodeBufs plan_ctc_beam(const masr_model* m, Arena& ar, int B, int Tp, int K, const masr_nlm* nlm) {
    DecodeBufs o{};
    o.ctc_logits = ar.get<float>((int64_t)B * Tp * m->Cp);
    o.work_bytes = nlm ? mk_ctc_beam_nlm_work_bytes(nlm, B, Tp, m->C, K) : mk_ctc_beam_work_bytes(B, Tp, m->C, K);
    o.work = ar.get<char>(o.work_bytes);
    return o;
}
static DecodeBufs plan_ctc_align(const masr_model* m, Arena& ar, int B, int Tp, int maxL) {
    DecodeBufs o{};
    o.ctc_logits = ar.get<float>((int64_t)B * Tp * m->Cp);
    o.al_tgt = ar.get<int>((int64_t)B * maxL + 2 * B);
    o.work_bytes = mk_ctc_align_work_bytes(B, Tp, maxL);
    o.work = ar.get<char>(o.work_bytes);
    return o;
}
static DecodeBufs plan_rescore(const masr_model* m, Arena& ar, int B, int Tp, const DecodeSpec& d) {
    DecodeBufs o{};
    const int64_t R = (int64_t)B * d.N;
    if (d.K) {
        o = plan_ctc_beam(m, ar, B, Tp, d.K, d.nlm);
        o.rs_tok = ar.get<int>(R * Tp); o.rs_lens = ar.get<int>(R); o.rs_ctc = ar.get<float>(R);
    }
    o.rs_att = ar.get<float>(R); o.rs_row_lp = ar.get<float>(R * (d.Lmax + 1));
    return o;
}
static DecodeBufs plan_decode(const masr_model* m, Arena& ar, Acts& a, int B, int T, int Ldec, const DecodeSpec& d) {
    switch (d.kind) {                                       // the decoder positions per utterance, then the decoder's own state
    case Decoder::greedy: plan_acts(m, ar, a, B, T, Ldec, false); break;
    case Decoder::step_beam: plan_acts(m, ar, a, B, T, d.K * d.Lmax, false); return plan_beam(m, ar, B, T / 4, d);
    case Decoder::ctc_beam: plan_acts(m, ar, a, B, T, 1, false); return plan_ctc_beam(m, ar, B, T / 4, d.K, d.nlm);
    case Decoder::rescore: plan_acts(m, ar, a, B, T, d.N * (d.Lmax + 1), false); return plan_rescore(m, ar, B, T / 4, d);
    case Decoder::align: plan_acts(m, ar, a, B, T, 1, false); return plan_ctc_align(m, ar, B, T / 4, d.maxL);
    }
    return DecodeBufs{};
}
// a decoder's workspace size, answered under the name of the spec's query; args_ok: B, T and the spec are in range (else the error d.need)
static int64_t decode_workspace_bytes(const masr_model* m, bool args_ok, int B, int T, const DecodeSpec& d) {
    const std::string name(d.query, strchr(d.query, '(')); const char* fn = name.c_str();      // the query's name
    if (!m || !args_ok) return fail(fn, d.need);
    if (d.kind == Decoder::step_beam ? d.P > 0 : d.kind != Decoder::greedy) CK(check_ctc_head(fn, m));      // (a step beam needs the head when joint)
    Arena ar{nullptr, 0, 0};
    Acts a;
    plan_decode(m, ar, a, B, T, 0, d);
    return m->persist_bytes + ar.off + 4096;
}

// n ints to dst on stream s through the next of the four pinned staging slots: fill(h) writes them once the slot's last copy has landed
template <class Fill>
static int stage_upload(masr_model* m, int* dst, int n, hipStream_t s, Fill fill) {
    const int slot = m->stage_slot; m->stage_slot = (slot + 1) & 3;
    HIP_CHECK_RET(hipEventSynchronize(m->stage_ev[slot]));
    int* h = m->h_stage + (int64_t)slot * m->stage_ints;
    fill(h);
    HIP_CHECK_RET(hipMemcpyAsync(dst, h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_CHECK_RET(hipEventRecord(m->stage_ev[slot], s));
    return 0;
}

static Ctx decode_ctx(masr_model* m, hipStream_t s) { return Ctx{m, s, 0u, false, 0.f, 0.f}; }      // no dropout, no training
// shared front half of the decoders: argument checks, the plan, enc_lens upload, encoder.  bufs: where the plan put the decoder's state;
// Ldec_out: the longest encoder length (the greedy decoders' step count)
static int recog_prepare(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, hipStream_t s, const DecodeSpec& d,
                         DecodeBufs* bufs = nullptr, int* Ldec_out = nullptr) {
    if (!m->P) { mk_set_error("masr_recog", "not bound"); return -1; }
    if (B <= 0 || T < 4) { mk_set_error("masr_recog", "need B >= 1 and T >= 4"); return -1; }
    int Ldec = 0;
    CK(check_ilens("masr_recog", ilens, B, T, [&](int, int enc) { Ldec = std::max(Ldec, enc); }));
    Arena ar{m->ws, m->ws_bytes, m->persist_bytes};
    stream_close(m);
    const DecodeBufs planned = plan_decode(m, ar, m->acts, B, T, Ldec, d);
    if (bufs) *bufs = planned;
    if (ar.off > m->ws_bytes) { mk_set_error("masr_recog", d.too_small().c_str()); return -2; }
    Acts& a = m->acts; m->have_acts = true;
    CK(stage_upload(m, a.enc_lens, B, s, [&](int* h) { for (int b = 0; b < B; ++b) h[b] = (int)(ilens[b] / 4); }));
    Ctx c = decode_ctx(m, s);
    CK(forward_encoder(c, xs));
    if (Ldec_out) *Ldec_out = Ldec;
    return 0;
}

extern "C" {

int masr_recog_full(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int32_t* out, void* stream) {
    // MyTransformer.recog (mono_transformer_torch.py:143-176) literally: the encoder runs once; then, for step = 1 .. max(enc_lens),
    // the WHOLE prefix [sos, out_0 .. out_{step-2}] is decoded again (no KV cache, exactly as the reference) and every
    // position's arg-max becomes the new `out`.  The result after the last step is out[Ldec][B].
    hipStream_t s = (hipStream_t)stream; int Ldec = 0;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, greedy_spec(), nullptr, &Ldec); if (rc) return rc; }
    Acts& a = m->acts;
    Ctx c = decode_ctx(m, s);
    CK(project_memory_kv(c));                               // (the memory does not change between steps)
    for (int step = 1; step <= Ldec; ++step) {
        a.L = step; a.rows_d = B * step;
        CK(mk_recog_build_tok(a.tok_in, out, B, step, 0, s));
        CK(forward_decoder(c, false, true));
        CK(mk_recog_argmax(a.logits, m->Cp, out, B, step, m->C, s));
    }
    m->have_acts = false;                                   // logits/gold views are not meaningful after a decode
    return 0;
}

int masr_recog(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int32_t* out, void* stream) {
    // Same token sequences as masr_recog_full with O(L) instead of O(L^2) decoder work: the target mask is causal, so the
    // re-decode of earlier positions reproduces what is already in `out`; only the newest position is computed per step,
    // against cached self-attention keys/values and encoder-memory keys/values projected once.  The per-step launch
    // sequence is captured into a hipGraph and replayed Ldec times (run_steps).
    hipStream_t s = (hipStream_t)stream; int Ldec = 0;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, greedy_spec(), nullptr, &Ldec); if (rc) return rc; }
    Acts& a = m->acts;
    Ctx c = decode_ctx(m, s);
    CK(project_memory_kv(c));
    CK(mk_recog_step_set(a.step_dev, 1, 0, s));
    const int key[6] = {B, T, Ldec, 0, 0, 0}; const void* const kp[3] = {m->ws, m->P, out};
    CK(run_steps(m, m->decode_graphs[G_GREEDY], key, kp, Ldec, s, "masr_recog", "stream capture of the decode step failed", [&] { return decode_step(c, out); }));
    m->have_acts = false;
    return 0;
}

}  // extern "C"

// once per decode, shared by the joint beam and the CTC first pass: the CTC head over the encoder memory (training's GEMM: bf16 operands,
// fp32 logits [B*Tp][Cp])
static int ctc_head_logits(Ctx& c, float* ctc_logits) {
    masr_model* m = c.m; Acts& a = m->acts;
    GemmArgs g = lin_fwd_args(a.mem16, m->E, m->ctc.k16, a.rows_e, m->C, m->E, m->P + m->ctc.b);
    g.C32 = ctc_logits; g.ldc = m->Cp;
    return gemm(c, g);
}

// the step beams' workspace queries: one predicate (N is read by the N-best variants alone)
static int64_t beam_workspace_bytes(GraphSlot g, const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int N, int Lmax) {
    const bool ok = shape_ok(B, T, K) && Lmax >= 1 && (!beam_variant(g).nbest || (N >= 1 && N <= K));
    return decode_workspace_bytes(m, ok, B, T, step_beam_spec(g, K, Lmax, N, nlm));
}

// One beam-search step on the B*K hypothesis rows (beam.hip).  Step-independent arguments throughout, like decode_step.  The launchers
// pick their kernels by ba.P (joint CTC/attention: the pre-beam, the prefix scores, the joint select) and ba.N (the joint LM beam,
// DESIGN 5.7 and, with the LSTM LM, 5.11: the prefix scores with the LM term and the bonus, the select with the N-best list; the weights are
// read from ba.wts), the row stage by `lm`.  LSTM LM fusion (nlm): the LM's layer stack and output projection on the rows' last
// tokens and parent states (nlm.hip; it reads only what the previous step's select wrote, so it sits in front of the decoder layers) fill
// lm.lm_logits.
// Phrase biasing (bias): the row stage, the prefix scores and the select take their biased forms.
static int beam_step(Ctx& c, const DecodeBufs& bufs, const BeamRowLm& lm, const masr_nlm* nlm, const NlmStepArgs& nlm_args, const BeamBias* bias = nullptr) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s;
    const BeamArgs& ba = bufs.beam;
    CK(mk_beam_embed_step(ba, m->P + m->embed_w, m->pe, a.y32[0], a.y16[0], m->E, s));
    if (nlm) CK(mk_nlm_step(nlm->dev, nlm_args, bufs.nlm_logits, m->Cp, s));
    CK(decode_layers(c, DecStepGeom{ba.R, ba.Lmax, ba.K, bufs.step_qkv, ba.tab, (long)ba.R * ba.Lmax}));
    CK(mk_beam_rows(ba, lm, a.logits, m->Cp, s, bias));
    if (ba.P) CK(mk_beam_ctc_prefix(ba, s, bias ? bias->pre_b : nullptr));
    return mk_beam_select(ba, s, bias);                         // also advances *step_dev
}

// which step beam, named by its graph slot (the entry point says which it is: beam_variant has what that search consists of), and its
// arguments: the joint beams' two weights, the N-best beams' list length, and what is fused (in the biased beams the LM may be absent)
struct BeamMode { GraphSlot slot = G_BEAM; float att_w = 0.f, ctc_w = 0.f; int N = 0; Fusion f; };
static BeamMode beam_mode(GraphSlot g, const Fusion& f, float att_w = 0.f, float ctc_w = 0.f, int N = 0) {
    BeamMode b; b.slot = g; b.f = f; b.att_w = att_w; b.ctc_w = ctc_w; b.N = N; return b;
}
// what the four joint beams' entry points vet first
static int check_joint(const char* fn, const masr_model* m, float att_w, float ctc_w) {
    CK(check_model(fn, m));
    CK(check_ctc_head(fn, m));
    CK(check_weight(fn, "ctc_w", ctc_w, true));
    return check_weight(fn, "att_w", att_w, false);
}

// What the step graph of `mode` is keyed on -- the one place that writes key words; the table is in engine_internal.h.  Whatever a captured
// launch holds by value is in the key, so that another LM, list or weight never replays this one's pointers: an LM's or list's serial
// number, and a weight's bits unless the weight is a device value written in front of the replays (all weights of the N-best beams).
struct StepKey { int w[6]; const void* p[3]; };
static StepKey beam_graph_key(const masr_model* m, const BeamMode& mode, int B, int T, int K, int Lmax) {
    const Fusion& f = mode.f;
    const auto bits = [](float v) { uint32_t u; memcpy(&u, &v, sizeof u); return u; };
    const auto list = [&](float w) { return (const void*)(uintptr_t)(((uint64_t)f.bias->serial << 32) | bits(w)); };
    const int lm_serial = f.lm ? (int)f.lm->serial : f.nlm ? (int)f.nlm->serial : 0;
    StepKey k{{B, T, K, Lmax, 0, 0}, {m->ws, m->P, nullptr}};
    switch (mode.slot) {
    case G_JOINT: k.w[4] = (int)bits(mode.att_w); k.w[5] = (int)bits(mode.ctc_w); break;
    case G_LM: case G_NLM: k.w[4] = (int)bits(f.lm_w); k.w[5] = lm_serial; break;
    case G_JOINT_LM: case G_JOINT_NLM: k.w[4] = mode.N; k.w[5] = lm_serial; break;
    case G_BIAS: k.w[4] = f.lm ? (int)bits(f.lm_w) : 0; k.w[5] = lm_serial; k.p[2] = list(f.bias_w); break;
    case G_JOINT_BIAS: k.w[4] = mode.N; k.w[5] = lm_serial; k.p[2] = list(0.f); break;
    default: break;                                             // (G_BEAM: the shape alone)
    }
    return k;
}

static int recog_beam_impl(const char* fn, masr_model* m, const BeamMode& mode, const float* xs, const int64_t* ilens, int B, int T, int K,
                           float min_step_ratio, float max_step_ratio, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    // Beam search over the KV-cached decoder step (semantics: beam.hip and DESIGN 9).  maxlen / minlen per utterance from
    // enc_len = ilens / 4 as the ESPnet rule; the step is captured once per key (beam_graph_key) and replayed Lmax times -- utterances that
    // finish earlier idle through the remaining replays.
    const BeamVariant& v = beam_variant(mode.slot); const Fusion& f = mode.f;
    CK(check_beam_size(fn, K));
    CK(check_pointers(fn, xs, ilens, tokens, lens, scores));
    if (f.bias && !f.nbias) return fail(fn, "null pointer");
    if (B <= 0) return fail(fn, "need B >= 1");
    std::vector<int> mx_len(B), mn_len(B);
    int Lmax = 0;
    CK(check_ilens(fn, ilens, B, T, [&](int b, int enc) {
        const int ml = max_step_ratio <= 0.f ? enc : std::max(1, (int)std::floor((double)max_step_ratio * enc));
        mx_len[b] = std::min(ml, MASR_PE_ROWS);
        mn_len[b] = std::max(0, (int)std::floor((double)min_step_ratio * enc));
        Lmax = std::max(Lmax, mx_len[b]);
    }));
    hipStream_t s = (hipStream_t)stream; DecodeBufs bufs;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, step_beam_spec(mode.slot, K, Lmax, mode.N, f.nlm), &bufs); if (rc) return rc; }
    BeamArgs& ba = bufs.beam;
    Acts& a = m->acts;
    ba.step = a.step_dev;
    // per-utterance maxlen / minlen through the next staging slot (the one behind recog_prepare's enc_lens)
    CK(stage_upload(m, const_cast<int*>(ba.maxlen), 2 * B, s, [&](int* h) { for (int b = 0; b < B; ++b) { h[b] = mx_len[b]; h[B + b] = mn_len[b]; } }));
    Ctx c = decode_ctx(m, s);
    CK(project_memory_kv(c));
    CK(mk_beam_init(ba, s));
    if (v.joint) {
        // once per decode: the CTC head over the memory, its log-softmax per frame, the empty hypothesis's state
        ba.att_w = mode.att_w; ba.ctc_w = mode.ctc_w; ba.enc_lens = a.enc_lens;
        CK(ctc_head_logits(c, bufs.ctc_logits));
        CK(mk_beam_ctc_logsoftmax(ba, bufs.ctc_logits, m->Cp, s));
        CK(mk_beam_ctc_init(ba, s));
    }
    BeamRowLm rl{};
    rl.lm_w = v.nbest ? 0.f : f.lm_w;                           // (the N-best beams read ba.wts: their graphs hold no weight)
    if (v.fused) { rl.fused = bufs.lm_fused; rl.ldf = m->Cp; }
    if (f.lm) rl.ngram = &f.lm->dev;
    NlmStepArgs na{};
    if (f.nlm) {
        rl.lm_logits = bufs.nlm_logits; rl.ld_lm = m->Cp;
        na.step = ba.step; na.R = ba.R; na.K = ba.K; na.tok_hist = ba.tok_hist; na.par_hist = ba.par_hist;
        na.hist_stride = ba.R; na.score = ba.score; na.fin = ba.fin;
        na.hstate = bufs.nlm_h; na.cstate = bufs.nlm_c; na.htop = bufs.nlm_htop;
    }
    if (v.nbest) CK(mk_beam_set_weights(ba, mode.att_w, mode.ctc_w, f.lm_w, f.len_bonus, s));
    BeamBias bb{};
    if (f.bias) {
        bb.dev = &f.bias->dev; bb.state = bufs.bias_state; bb.pre_b = bufs.bias_pre; bb.bias_w = v.nbest ? 0.f : f.bias_w;
        if (v.nbest) CK(mk_beam_set_bias_weight(ba, f.bias_w, s));
    }
    const BeamBias* bias = f.bias ? &bb : nullptr;
    const StepKey key = beam_graph_key(m, mode, B, T, K, Lmax);
    CK(run_steps(m, m->decode_graphs[mode.slot], key.w, key.p, Lmax, s, fn, "stream capture of the beam step failed",
                 [&] { return beam_step(c, bufs, rl, f.nlm, na, bias); }));
    CK(mk_beam_backtrace(ba, tokens, lens, scores, s, f.bias ? &f.bias->dev : nullptr, f.nbias));
    m->have_acts = false;
    return 0;
}

// the CTC prefix beam over the head's logits of the encoder memory (ctc_beam.hip), with an LM the fused sweep: the first pass of
// masr_recog_ctc_beam(_lm) and masr_recog_rescore(_lm).  With the LSTM LM the search is frame-synchronous: ONE frame is captured
// as a hipGraph of its own and replayed Tp times (utterances past their enc_len idle through the rest).  Keyed on (B, T, K, the LM) and on
// where the plan put what the frame's launches read (enc_lens, the logits, the work buffer); lm_w and len_bonus are device values written in
// front of the replays, so a call with other weights replays the same graph and never an old value.
static int ctc_first_pass(const char* fn, Ctx& c, const DecodeBufs& bufs, int B, int Tp, int K, int N, const Fusion& f, int32_t* tokens, int32_t* lens,
                          float* scores, float* am) {
    masr_model* m = c.m; Acts& a = m->acts;
    CK(ctc_head_logits(c, bufs.ctc_logits));
    if (f.bias) return mk_ctc_beam_search_bias(bufs.ctc_logits, m->Cp, a.enc_lens, B, Tp, m->C, K, N, 0, m->C - 1, f.lm, f.lm_w, f.len_bonus, f.bias, f.bias_w,
                                               bufs.work, bufs.work_bytes, tokens, lens, scores, am, f.nbias, c.s);
    if (f.nlm) {
        CtcNlmRun run;
        CK(mk_ctc_beam_nlm_begin(fn, bufs.ctc_logits, m->Cp, a.enc_lens, B, Tp, m->C, K, N, 0, m->C - 1, f.nlm, f.lm_w, f.len_bonus, bufs.work,
                                 bufs.work_bytes, tokens, lens, scores, am, &run, c.s));
        const int key[6] = {B, Tp, K, (int)f.nlm->serial, (int)(((char*)a.enc_lens - (char*)m->ws) >> 2), (int)(((char*)bufs.ctc_logits - (char*)m->ws) >> 2)};
        const void* const kp[3] = {m->ws, m->P, bufs.work};
        CK(run_steps(m, m->decode_graphs[G_CTC_NLM], key, kp, Tp, c.s, fn, "stream capture of the CTC beam's frame failed",
                     [&] { return mk_ctc_beam_nlm_frame(run, c.s); }));
        return mk_ctc_beam_nlm_end(run, N, tokens, lens, scores, c.s);
    }
    if (f.lm) return mk_ctc_beam_search_lm(bufs.ctc_logits, m->Cp, a.enc_lens, B, Tp, m->C, K, N, 0, m->C - 1, f.lm, f.lm_w, f.len_bonus, bufs.work,
                                           bufs.work_bytes, tokens, lens, scores, am, c.s);
    return mk_ctc_beam_search(bufs.ctc_logits, m->Cp, a.enc_lens, B, Tp, m->C, K, N, 0, m->C - 1, bufs.work, bufs.work_bytes, tokens, lens, scores, c.s);
}

// what every CTC prefix beam's entry point vets first; `name`: what it calls its list length
static int check_ctc_search(const char* fn, const masr_model* m, int K, const char* name, int N) {
    CK(check_model(fn, m));
    CK(check_ctc_head(fn, m));
    CK(check_beam_size(fn, K));
    return check_nbest(fn, name, N, K);
}
// the masr_recog_ctc_beam* entry points behind their checks of K, nbest and `f`: the pointers (am and nbias where `f` fills them), one
// encoder pass, the head GEMM, one sweep over the T/4 frames
static int recog_ctc_beam_impl(const char* fn, masr_model* m, const Fusion& f, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest,
                               int32_t* tokens, int32_t* lens, float* scores, float* am, void* stream) {
    CK(check_pointers(fn, xs, ilens, tokens, lens, scores));
    if ((f.lm || f.nlm || f.bias) && !am) return fail(fn, "null pointer");
    if (f.bias && !f.nbias) return fail(fn, "null pointer");
    hipStream_t s = (hipStream_t)stream; DecodeBufs bufs;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, ctc_beam_spec(K, f.nlm), &bufs); if (rc) return rc; }
    Ctx c = decode_ctx(m, s);
    CK(ctc_first_pass(fn, c, bufs, B, T / 4, K, nbest, f, tokens, lens, scores, am));
    m->have_acts = false;
    return 0;
}

// ---------------------------------------------------------------- attention rescoring
static int check_rescore_weights(const char* fn, float att_w, float ctc_w) {
    CK(check_weight(fn, "att_w", att_w, true));
    return check_weight(fn, "ctc_w", ctc_w, false);
}
// what every rescoring entry point with a first pass vets first
static int check_rescore_search(const char* fn, const masr_model* m, int K, int N, float att_w, float ctc_w) {
    CK(check_ctc_search(fn, m, K, "N", N));
    return check_rescore_weights(fn, att_w, ctc_w);
}
// The second pass over the lists tok [B*N][ld_tok] / lens / ctc (device), the encoder done: the decoder ONCE, teacher-forced, on B*N sequences
// of L = 1 + the longest live list positions (the eval pass's bf16-operand logits GEMM), each list's attention score, and the re-ranked copies
static int rescore_second_pass(Ctx& c, const DecodeBufs& bufs, const int* tok, long ld_tok, const int* lens, const float* ctc, int B, int N, int L,
                               float att_w, float ctc_w, int32_t* tokens, int32_t* lens_out, float* scores, float* att, float* ctc_out, int32_t* order) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s;
    const int R = B * N;
    CK(mk_rescore_prepare(tok, ld_tok, lens, R, L, 0, m->C - 1, a.tok_in, a.gold, s));
    const DecoderGeom gm{R, L};
    CK(forward_decoder(c, true, false, &gm));
    CK(mk_rescore_score(a.logits, m->Cp, a.gold, R, L, m->C, bufs.rs_row_lp, bufs.rs_att, s));
    CK(mk_rescore_select(tok, ld_tok, lens, ctc, bufs.rs_att, B, N, att_w, ctc_w, tokens, lens_out, scores, att, ctc_out, order, s));
    m->last_rescore = {a.logits, a.gold, R, L};
    m->have_acts = false;
    return 0;
}

// the masr_recog_rescore* entry points behind their checks of K, N, the weights and `f`: the two-pass decode on one encoder pass; with an LM
// the first pass is the fused search, its fused scores the c(b, n) of the second pass, and its acoustic totals land in the plan's scratch
// (rs_att, free until the second pass)
static int recog_rescore_impl(const char* fn, masr_model* m, const Fusion& f, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float att_w,
                              float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc, int32_t* order, void* stream) {
    CK(check_pointers(fn, xs, ilens, tokens, lens, scores));
    if (!att || !ctc || !order) return fail(fn, "null pointer");
    if (B <= 0 || T < 4) return fail(fn, "need B >= 1 and T >= 4");
    int Lcap = 0;                                           // a CTC hypothesis has at most enc_len tokens
    CK(check_ilens(fn, ilens, B, T, [&](int, int enc) { Lcap = std::max(Lcap, enc); }));
    Lcap = std::min(Lcap, MASR_PE_ROWS - 1);
    hipStream_t s = (hipStream_t)stream; DecodeBufs bufs;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, rescore_spec(K, N, Lcap, f.nlm), &bufs); if (rc) return rc; }
    Ctx c = decode_ctx(m, s);
    const int Tp = T / 4, R = B * N;
    // (a biased first pass leaves its n_final in the row-term scratch, which like rs_att is free until the second pass: R <= R * (Lmax + 1))
    Fusion first = f; first.nbias = (int32_t*)bufs.rs_row_lp;
    CK(ctc_first_pass(fn, c, bufs, B, Tp, K, N, first, bufs.rs_tok, bufs.rs_lens, bufs.rs_ctc, bufs.rs_att));
    // the one host synchronisation of the decode: the list lengths decide how many positions the decoder pass has
    std::vector<int> h_lens(R);
    HIP_CHECK_RET(hipMemcpyAsync(h_lens.data(), bufs.rs_lens, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    int mx = 0;
    for (int v : h_lens) mx = std::max(mx, v);
    if (mx > Lcap) return fail(fn, "a first-pass hypothesis is longer than the positions planned for");
    return rescore_second_pass(c, bufs, bufs.rs_tok, Tp, bufs.rs_lens, bufs.rs_ctc, B, N, mx + 1, att_w, ctc_w, tokens, lens, scores, att, ctc, order);
}

// masr_test_ctc_beam_logits / _ctc_align_logits: where the decoder of `d` (masr_recog_ctc_beam, masr_recog_ctc_align) put the head's logits and
// enc_lens in the bound workspace -- the same plan, run again
static int planned_logits(const char* fn, masr_model* m, bool args_ok, int B, int T, const DecodeSpec& d, float** logits, int64_t* ld, int32_t** enc_lens) {
    if (!m || !m->P || !logits || !ld || !enc_lens) return fail(fn, "null pointer or model not bound");
    CK(check_ctc_head(fn, m));
    if (!args_ok) return fail(fn, d.need);
    Arena ar{m->ws, m->ws_bytes, m->persist_bytes};
    Acts a;
    const DecodeBufs bufs = plan_decode(m, ar, a, B, T, 0, d);
    if (ar.off > m->ws_bytes) return fail(fn, d.too_small().c_str());
    *logits = bufs.ctc_logits; *ld = m->Cp; *enc_lens = a.enc_lens;
    return 0;
}

extern "C" {

int64_t masr_beam_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax) { return beam_workspace_bytes(G_BEAM, m, nullptr, B, T, K, 0, Lmax); }
int64_t masr_beam_ctc_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax) { return beam_workspace_bytes(G_JOINT, m, nullptr, B, T, K, 0, Lmax); }
int64_t masr_beam_lm_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax) { return beam_workspace_bytes(G_LM, m, nullptr, B, T, K, 0, Lmax); }
int64_t masr_beam_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int Lmax) {
    if (!nlm) return fail("masr_beam_nlm_workspace_bytes", "null language model");
    return beam_workspace_bytes(G_NLM, m, nlm, B, T, K, 0, Lmax);
}
int64_t masr_beam_ctc_lm_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax) {
    return beam_workspace_bytes(G_JOINT_LM, m, nullptr, B, T, K, N, Lmax);
}
int64_t masr_beam_ctc_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int N, int Lmax) {
    if (!nlm) return fail("masr_beam_ctc_nlm_workspace_bytes", "null language model");
    return beam_workspace_bytes(G_JOINT_NLM, m, nlm, B, T, K, N, Lmax);
}
int64_t masr_beam_bias_workspace_bytes(const masr_model* m, int B, int T, int K, int Lmax) { return beam_workspace_bytes(G_BIAS, m, nullptr, B, T, K, 0, Lmax); }
int64_t masr_beam_ctc_bias_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax) {
    return beam_workspace_bytes(G_JOINT_BIAS, m, nullptr, B, T, K, N, Lmax);
}
int64_t masr_ctc_beam_workspace_bytes(const masr_model* m, int B, int T, int K) {
    return decode_workspace_bytes(m, shape_ok(B, T, K), B, T, ctc_beam_spec(K, nullptr));
}
int64_t masr_ctc_beam_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K) {
    if (!nlm) return fail("masr_ctc_beam_nlm_workspace_bytes", "null language model");
    return decode_workspace_bytes(m, shape_ok(B, T, K), B, T, ctc_beam_spec(K, nlm));
}
int64_t masr_rescore_nlm_workspace_bytes(const masr_model* m, const masr_nlm* nlm, int B, int T, int K, int N, int Lmax) {
    if (!nlm) return fail("masr_rescore_nlm_workspace_bytes", "null language model");
    return decode_workspace_bytes(m, rescore_shape_ok(B, T, K, N, Lmax), B, T, rescore_spec(K, N, Lmax, nlm));
}
int64_t masr_rescore_workspace_bytes(const masr_model* m, int B, int T, int K, int N, int Lmax) {
    return decode_workspace_bytes(m, rescore_shape_ok(B, T, K, N, Lmax), B, T, rescore_spec(K, N, Lmax, nullptr));
}

int masr_recog_beam(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio, float max_step_ratio,
                    int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    const char* fn = "masr_recog_beam";
    CK(check_model(fn, m));
    return recog_beam_impl(fn, m, beam_mode(G_BEAM, Fusion{}), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_ctc(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio, float max_step_ratio,
                        float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    // joint CTC/attention beam (beam.hip): the attention beam's search with the CTC prefix score of the head's log-probs
    const char* fn = "masr_recog_beam_ctc";
    CK(check_joint(fn, m, att_w, ctc_w));
    return recog_beam_impl(fn, m, beam_mode(G_JOINT, Fusion{}, att_w, ctc_w), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio,
                       float max_step_ratio, float lm_w, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    // n-gram LM shallow fusion into the attention beam: masr_recog_beam with the n-gram term fused into its row stage
    const char* fn = "masr_recog_beam_lm"; const Fusion f = fuse_lm(lm, lm_w);
    CK(check_model(fn, m));
    CK(check_lm(fn, m, f, false));
    return recog_beam_impl(fn, m, beam_mode(G_LM, f), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, float min_step_ratio,
                        float max_step_ratio, float lm_w, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    // LSTM LM shallow fusion into the attention beam (nlm.hip): masr_recog_beam with the LM's step in front of the decoder layers
    // and its term fused into the row stage
    const char* fn = "masr_recog_beam_nlm"; const Fusion f = fuse_nlm(nlm, lm_w);
    CK(check_model(fn, m));
    CK(check_lm(fn, m, f, false));
    return recog_beam_impl(fn, m, beam_mode(G_NLM, f), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_ctc_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float min_step_ratio,
                           float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, int32_t* tokens, int32_t* lens, float* scores,
                           void* stream) {
    // the joint beam with the n-gram LM in the pre-beam and the score, a bonus per emitted token and an N-best list
    const char* fn = "masr_recog_beam_ctc_lm"; const Fusion f = fuse_lm(lm, lm_w, len_bonus);
    CK(check_joint(fn, m, att_w, ctc_w));
    CK(check_lm(fn, m, f, true));
    CK(check_beam_size(fn, K));
    CK(check_nbest(fn, "N", N, K));
    return recog_beam_impl(fn, m, beam_mode(G_JOINT_LM, f, att_w, ctc_w, N), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_ctc_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float min_step_ratio,
                            float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, int32_t* tokens, int32_t* lens, float* scores,
                            void* stream) {
    // masr_recog_beam_ctc_lm with the LSTM LM's term in the pre-beam and the score: the LM's step in front of the decoder layers,
    // as in masr_recog_beam_nlm
    const char* fn = "masr_recog_beam_ctc_nlm"; const Fusion f = fuse_nlm(nlm, lm_w, len_bonus);
    CK(check_joint(fn, m, att_w, ctc_w));
    CK(check_lm(fn, m, f, true));
    CK(check_beam_size(fn, K));
    CK(check_nbest(fn, "N", N, K));
    return recog_beam_impl(fn, m, beam_mode(G_JOINT_NLM, f, att_w, ctc_w, N), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K,
                         float min_step_ratio, float max_step_ratio, float lm_w, float bias_w, int32_t* tokens, int32_t* lens, float* scores,
                         int32_t* nbias, void* stream) {
    // contextual phrase biasing of the attention beam: masr_recog_beam(_lm) with the automaton's term in the row increment
    const char* fn = "masr_recog_beam_bias"; const Fusion f = fuse_bias(fuse_lm(lm, lm ? lm_w : 0.f), bias, bias_w, nbias);
    CK(check_model(fn, m));
    if (lm) CK(check_lm(fn, m, f, false));
    CK(check_bias(fn, m, f));
    return recog_beam_impl(fn, m, beam_mode(G_BIAS, f), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_beam_ctc_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K, int N,
                             float min_step_ratio, float max_step_ratio, float att_w, float ctc_w, float lm_w, float len_bonus, float bias_w,
                             int32_t* tokens, int32_t* lens, float* scores, int32_t* nbias, void* stream) {
    // contextual phrase biasing of the joint beam: masr_recog_beam_ctc_lm with the automaton's term in the pre-beam and the score
    const char* fn = "masr_recog_beam_ctc_bias"; const Fusion f = fuse_bias(fuse_lm(lm, lm ? lm_w : 0.f, len_bonus), bias, bias_w, nbias);
    CK(check_joint(fn, m, att_w, ctc_w));
    if (lm) CK(check_lm(fn, m, f, true));
    else if (!std::isfinite(len_bonus)) return fail(fn, "len_bonus must be finite");
    CK(check_bias(fn, m, f));
    CK(check_beam_size(fn, K));
    CK(check_nbest(fn, "N", N, K));
    return recog_beam_impl(fn, m, beam_mode(G_JOINT_BIAS, f, att_w, ctc_w, N), xs, ilens, B, T, K, min_step_ratio, max_step_ratio, tokens, lens, scores, stream);
}

int masr_recog_ctc_beam(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, int32_t* tokens, int32_t* lens,
                        float* scores, void* stream) {
    // CTC prefix beam search on the head alone (ctc_beam.hip)
    const char* fn = "masr_recog_ctc_beam";
    CK(check_ctc_search(fn, m, K, "nbest", nbest));
    return recog_ctc_beam_impl(fn, m, Fusion{}, xs, ilens, B, T, K, nbest, tokens, lens, scores, nullptr, stream);
}

int masr_recog_ctc_beam_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, float lm_w,
                           float len_bonus, int32_t* tokens, int32_t* lens, float* scores, float* am, void* stream) {
    // masr_recog_ctc_beam with the LM-fused sweep (ctc_beam.hip): the same plan, encoder pass and head GEMM
    const char* fn = "masr_recog_ctc_beam_lm"; const Fusion f = fuse_lm(lm, lm_w, len_bonus);
    CK(check_ctc_search(fn, m, K, "nbest", nbest));
    CK(check_lm(fn, m, f, true));
    return recog_ctc_beam_impl(fn, m, f, xs, ilens, B, T, K, nbest, tokens, lens, scores, am, stream);
}

int masr_recog_ctc_beam_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K,
                             int nbest, float lm_w, float len_bonus, float bias_w, int32_t* tokens, int32_t* lens, float* scores, float* am,
                             int32_t* nbias, void* stream) {
    // masr_recog_ctc_beam with the phrase-biased sweep (ctc_beam.hip), the n-gram LM fused in when one is given: the same plan
    const char* fn = "masr_recog_ctc_beam_bias"; const Fusion f = fuse_bias(fuse_lm(lm, lm_w, len_bonus), bias, bias_w, nbias);
    CK(check_ctc_search(fn, m, K, "nbest", nbest));
    if (lm) CK(check_lm(fn, m, f, true));
    CK(check_bias(fn, m, f));
    return recog_ctc_beam_impl(fn, m, f, xs, ilens, B, T, K, nbest, tokens, lens, scores, am, stream);
}

int masr_recog_ctc_beam_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int nbest, float lm_w,
                            float len_bonus, int32_t* tokens, int32_t* lens, float* scores, float* am, void* stream) {
    // masr_recog_ctc_beam with the LSTM LM's frame-synchronous search (ctc_beam.hip): the same encoder pass and head GEMM
    const char* fn = "masr_recog_ctc_beam_nlm"; const Fusion f = fuse_nlm(nlm, lm_w, len_bonus);
    CK(check_model(fn, m));
    if (!nlm) return fail(fn, "null language model");
    CK(check_ctc_search(fn, m, K, "nbest", nbest));
    CK(check_lm(fn, m, f, true));
    return recog_ctc_beam_impl(fn, m, f, xs, ilens, B, T, K, nbest, tokens, lens, scores, am, stream);
}

int masr_test_ctc_beam_logits(masr_model* m, int B, int T, int K, float** logits, int64_t* ld, int32_t** enc_lens) {
    return planned_logits("masr_test_ctc_beam_logits", m, shape_ok(B, T, K), B, T, ctc_beam_spec(K, nullptr), logits, ld, enc_lens);
}

int64_t masr_ctc_align_workspace_bytes(const masr_model* m, int B, int T, int maxL) {
    return decode_workspace_bytes(m, align_shape_ok(B, T, maxL), B, T, align_spec(maxL));
}

int masr_recog_ctc_align(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, const int64_t* ys_flat, const int64_t* olens, int maxL,
                         int32_t* frames, int32_t* start, int32_t* end, float* score, void* stream) {
    // forced alignment of each utterance's transcript on the CTC head (ctc_align.hip): the encoder pass and the head GEMM of
    // masr_recog_ctc_beam, then masr_ctc_align with blank 0.  Lengths and tokens the operator refuses on the device are passed on as they
    // are (clamped into int32): the refusal is the operator's.
    const char* fn = "masr_recog_ctc_align";
    CK(check_model(fn, m));
    CK(check_ctc_head(fn, m));
    if (!xs || !ilens || !olens || !frames || !start || !end || !score) return fail(fn, "null pointer");
    if (!align_shape_ok(B, T, maxL)) return fail(fn, align_spec(maxL).need);
    int64_t total = 0;                                      // tokens uploaded: those of the utterances whose length is in range
    for (int b = 0; b < B; ++b) if (olens[b] > 0 && olens[b] <= maxL) total += olens[b];
    if (total > 0 && !ys_flat) return fail(fn, "null pointer");
    if ((int64_t)B * maxL + 2 * B > m->stage_ints) return fail(fn, ("B * (maxL + 2) exceeds the staging buffer (" + std::to_string(m->stage_ints) + " ints)").c_str());
    hipStream_t s = (hipStream_t)stream; DecodeBufs bufs;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, align_spec(maxL), &bufs); if (rc) return rc; }
    const auto i32 = [](int64_t v) { return (int)std::max<int64_t>(std::min<int64_t>(v, INT32_MAX), INT32_MIN); };
    int* tgt = bufs.al_tgt; int* off = tgt + (int64_t)B * maxL; int* len = off + B;
    CK(stage_upload(m, tgt, B * maxL + 2 * B, s, [&](int* h) {
        // ys_flat holds olens[b] tokens per utterance with olens[b] > 0, whatever the operator will make of that length
        int64_t src = 0; int dst = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t n = olens[b];
            h[B * maxL + b] = dst; h[B * maxL + B + b] = i32(n);
            if (n > 0 && n <= maxL) for (int64_t i = 0; i < n; ++i) h[dst++] = i32(ys_flat[src + i]);
            if (n > 0) src += n;
        }
        for (; dst < B * maxL; ++dst) h[dst] = 0;
    }));
    Ctx c = decode_ctx(m, s);
    CK(ctc_head_logits(c, bufs.ctc_logits));
    CK(mk_ctc_align(bufs.ctc_logits, m->Cp, m->acts.enc_lens, tgt, off, len, B, T / 4, m->C, 0, maxL, bufs.work, bufs.work_bytes, frames, start, end, score, s));
    m->have_acts = false;
    return 0;
}

int masr_test_ctc_align_logits(masr_model* m, int B, int T, int maxL, float** logits, int64_t* ld, int32_t** enc_lens) {
    return planned_logits("masr_test_ctc_align_logits", m, align_shape_ok(B, T, maxL), B, T, align_spec(maxL), logits, ld, enc_lens);
}

int masr_recog_rescore(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float att_w, float ctc_w, int32_t* tokens,
                       int32_t* lens, float* scores, float* att, float* ctc, int32_t* order, void* stream) {
    const char* fn = "masr_recog_rescore";
    CK(check_rescore_search(fn, m, K, N, att_w, ctc_w));
    return recog_rescore_impl(fn, m, Fusion{}, xs, ilens, B, T, K, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order, stream);
}

int masr_recog_rescore_lm(masr_model* m, const masr_lm* lm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float lm_w,
                          float len_bonus, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc,
                          int32_t* order, void* stream) {
    const char* fn = "masr_recog_rescore_lm"; const Fusion f = fuse_lm(lm, lm_w, len_bonus);
    CK(check_rescore_search(fn, m, K, N, att_w, ctc_w));
    CK(check_lm(fn, m, f, true));
    return recog_rescore_impl(fn, m, f, xs, ilens, B, T, K, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order, stream);
}

int masr_recog_rescore_bias(masr_model* m, const masr_lm* lm, const masr_bias* bias, const float* xs, const int64_t* ilens, int B, int T, int K, int N,
                            float lm_w, float len_bonus, float bias_w, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores,
                            float* att, float* ctc, int32_t* order, void* stream) {
    const char* fn = "masr_recog_rescore_bias"; const Fusion f = fuse_bias(fuse_lm(lm, lm_w, len_bonus), bias, bias_w, nullptr);    // (the impl finds room for n_final)
    CK(check_rescore_search(fn, m, K, N, att_w, ctc_w));
    if (lm) CK(check_lm(fn, m, f, true));
    CK(check_bias(fn, m, f));
    return recog_rescore_impl(fn, m, f, xs, ilens, B, T, K, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order, stream);
}

int masr_recog_rescore_nlm(masr_model* m, const masr_nlm* nlm, const float* xs, const int64_t* ilens, int B, int T, int K, int N, float lm_w,
                           float len_bonus, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att, float* ctc,
                           int32_t* order, void* stream) {
    const char* fn = "masr_recog_rescore_nlm"; const Fusion f = fuse_nlm(nlm, lm_w, len_bonus);
    CK(check_model(fn, m));
    if (!nlm) return fail(fn, "null language model");
    CK(check_rescore_search(fn, m, K, N, att_w, ctc_w));
    CK(check_lm(fn, m, f, true));
    return recog_rescore_impl(fn, m, f, xs, ilens, B, T, K, N, att_w, ctc_w, tokens, lens, scores, att, ctc, order, stream);
}

int masr_rescore_nbest(masr_model* m, const float* xs, const int64_t* ilens, int B, int T, int N, const int32_t* tokens_in, int64_t ld_tok,
                       const int32_t* lens_in, const float* ctc_in, float att_w, float ctc_w, int32_t* tokens, int32_t* lens, float* scores, float* att,
                       float* ctc, int32_t* order, void* stream) {
    const char* fn = "masr_rescore_nbest";
    CK(check_model(fn, m));
    CK(check_ctc_head(fn, m));
    if (N < 1 || N > 64) return fail(fn, "N must be in [1, 64]");
    CK(check_rescore_weights(fn, att_w, ctc_w));
    CK(check_pointers(fn, xs, ilens, tokens, lens, scores));
    if (!att || !ctc || !order || !lens_in || !ctc_in || (ld_tok > 0 && !tokens_in)) return fail(fn, "null pointer");
    if (B <= 0 || T < 4 || ld_tok < 0 || ld_tok >= MASR_PE_ROWS) return fail(fn, "need B >= 1, T >= 4 and 0 <= ld_tok < 3000");
    hipStream_t s = (hipStream_t)stream;
    // the one host synchronisation of the call: the lists come to the host, where their lengths decide the decoder's positions and every
    // token is vetted (it indexes the embedding table)
    const int R = B * N;
    std::vector<int> h_lens(R), h_tok((size_t)R * ld_tok);
    HIP_CHECK_RET(hipMemcpyAsync(h_lens.data(), lens_in, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
    if (ld_tok) HIP_CHECK_RET(hipMemcpyAsync(h_tok.data(), tokens_in, sizeof(int) * h_tok.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    int mx = 0;
    for (int r = 0; r < R; ++r) {
        const int n = h_lens[r];
        if (n < 0) continue;
        if (n > ld_tok) return fail(fn, "a list is longer than ld_tok");
        for (int i = 0; i < n; ++i) {
            const int t = h_tok[(size_t)r * ld_tok + i];
            if (t < 1 || t > m->C - 2) return fail(fn, "tokens must lie in [1, odim - 2] (no sos / blank, no eos)");
        }
        mx = std::max(mx, n);
    }
    DecodeBufs bufs;
    { const int rc = recog_prepare(m, xs, ilens, B, T, s, rescore_spec(0, N, mx, nullptr), &bufs); if (rc) return rc; }
    Ctx c = decode_ctx(m, s);
    return rescore_second_pass(c, bufs, tokens_in, (long)ld_tok, lens_in, ctc_in, B, N, mx + 1, att_w, ctc_w, tokens, lens, scores, att, ctc, order);
}

int masr_test_rescore_logits(masr_model* m, float** logits, int64_t* ld, int32_t** gold, int* R, int* L) {
    const char* fn = "masr_test_rescore_logits";
    if (!m || !logits || !ld || !gold || !R || !L) return fail(fn, "null pointer");
    if (!m->last_rescore.logits) return fail(fn, "no rescoring call yet");
    *logits = m->last_rescore.logits; *ld = m->Cp; *gold = m->last_rescore.gold; *R = m->last_rescore.R; *L = m->last_rescore.L;
    return 0;
}

}  // extern "C"
