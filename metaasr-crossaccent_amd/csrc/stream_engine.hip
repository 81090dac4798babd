// libmasr engine, the streaming first pass: the chunk-masked encoder of masr_set_chunk run incrementally -- the front-end on
// input windows, every encoder layer on the chunk's rows against a per-layer K|V cache (stream.hip) --, a greedy CTC decode that carries its
// state across chunks, the full-utterance CTC prefix beam (ctc_beam.hip, unchanged) on the logits the stream left behind, and the resumable
// prefix beam (ctc_beam.hip's run object) that follows the chunks feed by feed once masr_stream_beam_open has opened one.
//
// Chunk n covers the encoder frames [s, e) = [n c, min((n + 1) c, T / 4)).  Encoder frame t reads the input frames 4t - 6 .. 4t + 9, so the
// four convs and vgg2enc on the input window [max(0, 4s - 8), min(T, 4e + 8)) give the chunk's rows exactly: the window starts at a multiple
// of 4 (the pools line up), a window clipped at 0 or T sees the true zero padding, and inside the utterance the layers' padding at the window
// edge spoils halo frames only.  A chunk runs as soon as its window is complete, so what is emitted does not depend on how the audio was cut.
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "engine_internal.h"

namespace {

constexpr int STREAM_MAX_FRAMES = 4 * MASR_PE_ROWS;       // the positional-encoding table has 3000 rows
constexpr int STREAM_BEAM_K = 64;                         // the final beam's work buffer is planned for the widest beam

struct StreamLayer { bf16* kv; };                         // [B][cap][2E]: K | V of every frame emitted so far
struct StreamBufs {
    int cap, Rmax, Wmax;                                  // cache rows, rows of a step, input frames of a window
    int *lens, *state, *tokens, *frames;                  // lens [2][B]: frames received | klen = frames / 4; state [2][B]: previous arg-max | len
    float *xbuf, *win, *v32, *s1, *x1_32, *s2, *mean, *rstd, *step_logits, *logits;
    bf16 *a1, *p1, *a3, *p2, *qkv, *ao, *x1_16, *f, *mem16;
    std::vector<float*> x32; std::vector<bf16*> x16; std::vector<StreamLayer> layer;
    void* work; int64_t work_bytes;
    void* beam_work; int64_t beam_work_bytes;             // the resumable beam's own work buffer and state block
};

void plan_stream(const masr_model* m, Arena& ar, StreamBufs& sb, int B, int max_frames, int c) {
    const int E = m->E, D = m->D;
    sb.cap = max_frames / 4; sb.Rmax = std::min(c, sb.cap); sb.Wmax = std::min(4 * sb.Rmax + 16, max_frames);
    const int64_t rows = (int64_t)B * sb.Rmax, H2 = sb.Wmax / 2, W2 = D / 2, Wp = H2 / 2;
    sb.lens = ar.get<int>(2 * B); sb.state = ar.get<int>(2 * B);
    sb.tokens = ar.get<int>((int64_t)B * sb.cap); sb.frames = ar.get<int>((int64_t)B * sb.cap);
    sb.xbuf = ar.get<float>((int64_t)B * max_frames * D); sb.win = ar.get<float>((int64_t)B * sb.Wmax * D);
    sb.a1 = ar.get<bf16>((int64_t)B * sb.Wmax * D * 64); sb.p1 = ar.get<bf16>((int64_t)B * H2 * W2 * 64);
    sb.a3 = ar.get<bf16>((int64_t)B * H2 * W2 * 128); sb.p2 = ar.get<bf16>((int64_t)B * Wp * m->F);
    sb.v32 = ar.get<float>((int64_t)B * Wp * E);
    sb.x32.resize(m->NE + 1); sb.x16.resize(m->NE + 1); sb.layer.resize(m->NE);
    for (int l = 0; l <= m->NE; ++l) { sb.x32[l] = ar.get<float>(rows * E); sb.x16[l] = ar.get<bf16>(rows * E); }
    sb.qkv = ar.get<bf16>(rows * 3 * E); sb.ao = ar.get<bf16>(rows * E); sb.s1 = ar.get<float>(rows * E);
    sb.x1_32 = ar.get<float>(rows * E); sb.x1_16 = ar.get<bf16>(rows * E); sb.f = ar.get<bf16>(rows * m->Fi); sb.s2 = ar.get<float>(rows * E);
    sb.mean = ar.get<float>(rows); sb.rstd = ar.get<float>(rows); sb.mem16 = ar.get<bf16>(rows * E);
    sb.step_logits = ar.get<float>(rows * m->Cp);
    for (auto& L : sb.layer) L.kv = ar.get<bf16>((int64_t)B * sb.cap * 2 * E);
    sb.logits = ar.get<float>((int64_t)B * sb.cap * m->Cp);
    sb.work_bytes = mk_ctc_beam_work_bytes(B, sb.cap, m->C, STREAM_BEAM_K);
    sb.work = ar.get<char>(sb.work_bytes);
    // behind everything else, so that no other offset moves: masr_stream_ctc_beam may run beside an open beam
    sb.beam_work_bytes = mk_ctc_beam_run_work_bytes(B, sb.cap, m->C, STREAM_BEAM_K);
    sb.beam_work = ar.get<char>(sb.beam_work_bytes);
}

int sfail(const char* fn, const char* msg) { mk_set_error(fn, msg); return -1; }

// the open stream of m and the plan of its buffers; -1 with "no open stream"
int open_stream(const char* fn, masr_model* m, StreamBufs& sb) {
    if (!m) return sfail(fn, "null model");
    if (!m->stream.open) return sfail(fn, "no open stream (masr_stream_begin; any other call that plans the workspace ends one)");
    Arena ar{m->ws, m->ws_bytes, m->persist_bytes};
    plan_stream(m, ar, sb, m->stream.B, m->stream.max_frames, m->stream.c);
    return 0;
}

int sgemm(masr_model* m, GemmArgs g, hipStream_t s) { g.lean = m->slots > 1; return mk_gemm(g, s); }
int sln(masr_model* m, const Norm& n, const float* x, float* y32, bf16* y16, const StreamBufs& sb, int rows, hipStream_t s) {
    return mk_layernorm_fwd(x, m->P + n.w, m->P + n.b, y32, y16, sb.mean, sb.rstd, rows, m->E, s);
}

// one chunk step: the encoder frames [s0, e) of every utterance, `recv` input frames buffered
int stream_step(masr_model* m, const StreamBufs& sb, int s0, int e, hipStream_t s) {
    const masr_model::Stream& st = m->stream; const float* P = m->P;
    const int B = st.B, E = m->E, D = m->D, R = e - s0;
    const int w0 = std::max(0, 4 * s0 - 8), w1 = std::min(st.recv, 4 * e + 8), W = w1 - w0, H2 = W / 2, W2 = D / 2, Wp = H2 / 2, off = s0 - w0 / 4;
    if (R < 1 || R > sb.Rmax || W > sb.Wmax || off + R > Wp) return sfail("masr_stream_feed", "internal: a window outside the plan");
    const int* klens = sb.lens + B;
    // the front-end on the window (forward_encoder's launches on B x W x D)
    CK(mk_stream_window(sb.xbuf, sb.lens, sb.win, B, W, D, w0, st.max_frames, s));
    CK(mk_conv1_fwd(sb.win, P + m->conv[0].w, P + m->conv[0].b, sb.a1, B, W, D, s, nullptr));
    auto conv = [&](const bf16* in, const Conv& cv, bf16* out, int H, int Wd, bf16* pooled) -> int {
        ConvArgs ca{}; ca.sched = m->conv_sched; ca.in = in; ca.wk = cv.k16; ca.bias = P + cv.b; ca.relu = 1; ca.out = out;
        ca.B = B; ca.H = H; ca.W = Wd; ca.CIN = cv.CI; ca.COUT = cv.CO; ca.pool_out = pooled;
        if (pooled) ca.out_optional = 1;
        return mk_conv3x3(ca, s);
    };
    CK(conv(sb.a1, m->conv[1], nullptr, W, D, sb.p1));
    CK(conv(sb.p1, m->conv[2], sb.a3, H2, W2, nullptr));
    CK(conv(sb.a3, m->conv[3], nullptr, H2, W2, sb.p2));
    {
        GemmArgs g = lin_fwd_args(sb.p2, m->F, m->v2e_k, B * Wp, E, m->F, P + m->v2e.b);
        g.C32 = sb.v32; g.ldc = E;
        CK(sgemm(m, g, s));
    }
    CK(mk_stream_centre_pe(sb.v32, m->pe, sb.x32[0], sb.x16[0], B, R, E, Wp, off, s0, s));
    const int rows = B * R, n = s0 / st.c;
    const int lo = st.left < 0 ? 0 : std::max(0, (n - st.left) * st.c);
    for (int l = 0; l < m->NE; ++l) {
        const EncL& w = m->enc[l];
        GemmArgs g = lin_fwd_args(sb.x16[l], E, w.sa.in.k16, rows, 3 * E, E, P + w.sa.in.b); g.C16 = sb.qkv; g.ldc16 = 3 * E;
        CK(sgemm(m, g, s));
        AttnStreamArgs a{};
        a.q = sb.qkv; a.ldq = 3 * E; a.knew = sb.qkv + E; a.vnew = sb.qkv + 2 * E; a.ldnew = 3 * E;
        a.kc = sb.layer[l].kv; a.vc = sb.layer[l].kv + E; a.ldc = 2 * E; a.batch_stride = (long)sb.cap * 2 * E;
        a.klens = klens; a.o = sb.ao; a.ldo = E; a.B = B; a.H = m->H; a.hd = m->hd; a.R = R; a.pos = s0; a.lo = lo; a.cap = sb.cap;
        CK(mk_attn_stream(a, s));
        GemmArgs o = lin_fwd_args(sb.ao, E, w.sa.out.k16, rows, E, E, P + w.sa.out.b);
        o.residual = sb.x32[l]; o.ldres = E; o.C32 = sb.s1; o.ldc = E;
        CK(sgemm(m, o, s));
        CK(sln(m, w.n1, sb.s1, sb.x1_32, sb.x1_16, sb, rows, s));
        GemmArgs f1 = lin_fwd_args(sb.x1_16, E, w.l1.k16, rows, m->Fi, E, P + w.l1.b); f1.relu = 1; f1.C16 = sb.f; f1.ldc16 = m->Fi;
        CK(sgemm(m, f1, s));
        GemmArgs f2 = lin_fwd_args(sb.f, m->Fi, w.l2.k16, rows, E, m->Fi, P + w.l2.b);
        f2.residual = sb.x1_32; f2.ldres = E; f2.C32 = sb.s2; f2.ldc = E;
        CK(sgemm(m, f2, s));
        CK(sln(m, w.n2, sb.s2, sb.x32[l + 1], sb.x16[l + 1], sb, rows, s));
    }
    CK(sln(m, m->enc_norm, sb.x32[m->NE], nullptr, sb.mem16, sb, rows, s));
    {
        GemmArgs g = lin_fwd_args(sb.mem16, E, m->ctc.k16, rows, m->C, E, P + m->ctc.b);
        g.C32 = sb.step_logits; g.ldc = m->Cp;
        CK(sgemm(m, g, s));
    }
    CtcGreedyStreamArgs ga{};
    ga.logits = sb.step_logits; ga.ld = m->Cp; ga.batch_stride = (long)R * m->Cp; ga.klens = klens; ga.B = B; ga.R = R; ga.C = m->C; ga.pos = s0;
    ga.state = sb.state; ga.tokens = sb.tokens; ga.frames = sb.frames; ga.ld_out = sb.cap;
    CK(mk_ctc_greedy_stream(ga, s));
    // the step's rows into the accumulated logits [B][cap][Cp] (the layout masr_ctc_beam_search reads)
    const size_t rb = sizeof(float) * (size_t)R * m->Cp;
    HIP_CHECK_RET(hipMemcpy2DAsync(sb.logits + (int64_t)s0 * m->Cp, sizeof(float) * (size_t)sb.cap * m->Cp, sb.step_logits, rb, rb, B,
                                   hipMemcpyDeviceToDevice, s));
    return 0;
}

bool stream_shape_ok(int B, int max_frames) { return B >= 1 && B <= 65535 && max_frames >= 4 && max_frames <= STREAM_MAX_FRAMES; }

}  // namespace

extern "C" {

int64_t masr_stream_workspace_bytes(const masr_model* m, int B, int max_frames) {
    const char* fn = "masr_stream_workspace_bytes";
    if (!m) return sfail(fn, "null model");
    if (!stream_shape_ok(B, max_frames)) return sfail(fn, "need 1 <= B <= 65535 and 4 <= max_frames <= 12000");
    if (!(m->ctc_w > 0.f)) return sfail(fn, "the model has no CTC head (masr_create_ctc)");
    if (m->chunk.size <= 0) return sfail(fn, "the model's chunk policy has no size (masr_set_chunk)");
    Arena ar{nullptr, 0, 0};
    StreamBufs sb;
    plan_stream(m, ar, sb, B, max_frames, m->chunk.size);
    return m->persist_bytes + ar.off + 4096;
}

int masr_stream_begin(masr_model* m, int B, int max_frames, void* stream) {
    const char* fn = "masr_stream_begin";
    if (!m) return sfail(fn, "null model");
    if (!m->P) return sfail(fn, "not bound");
    if (!(m->ctc_w > 0.f)) return sfail(fn, "the model has no CTC head (masr_create_ctc)");
    if (m->chunk.size <= 0) return sfail(fn, "the model's chunk policy has no size (masr_set_chunk)");
    if (!stream_shape_ok(B, max_frames)) return sfail(fn, "need 1 <= B <= 65535 and 4 <= max_frames <= 12000");
    if (2 * (int64_t)B > m->stage_ints) return sfail(fn, "B exceeds the staging buffer");
    Arena ar{m->ws, m->ws_bytes, m->persist_bytes};
    StreamBufs sb;
    plan_stream(m, ar, sb, B, max_frames, m->chunk.size);
    if (ar.off > m->ws_bytes) { mk_set_error(fn, "workspace too small (masr_stream_workspace_bytes(B, max_frames))"); return -2; }
    hipStream_t s = (hipStream_t)stream;
    m->have_acts = false;                                   // (the activation plan of the last batch is overwritten)
    masr_model::Stream& st = m->stream;
    stream_close(m);
    HIP_CHECK_RET(hipMemsetAsync(sb.lens, 0, sizeof(int) * 2 * (size_t)B, s));
    HIP_CHECK_RET(hipMemsetAsync(sb.state, 0, sizeof(int) * 2 * (size_t)B, s));
    HIP_CHECK_RET(hipMemsetAsync(sb.tokens, 0xFF, sizeof(int) * (size_t)B * sb.cap, s));
    HIP_CHECK_RET(hipMemsetAsync(sb.frames, 0xFF, sizeof(int) * (size_t)B * sb.cap, s));
    HIP_CHECK_RET(hipMemsetAsync(sb.logits, 0, sizeof(float) * (size_t)B * sb.cap * m->Cp, s));
    st.B = B; st.max_frames = max_frames; st.c = m->chunk.size; st.left = m->chunk.left; st.recv = 0; st.emitted = 0; st.last = false;
    st.len.assign(B, 0); st.ended.assign(B, 0);
    m->chunk_last = st.c;
    st.open = true;
    return 0;
}

int masr_stream_feed(masr_model* m, const float* xs, int n, const int32_t* valid, int last, int* frames_out, void* stream) {
    const char* fn = "masr_stream_feed";
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    masr_model::Stream& st = m->stream;
    if (st.last) return sfail(fn, "the stream has had its last piece (masr_stream_begin opens another)");
    if (n < 0 || (n > 0 && !xs)) return sfail(fn, "need n >= 0 and, with n > 0, the piece");
    if ((int64_t)st.recv + n > st.max_frames) return sfail(fn, "more frames than max_frames");
    const int B = st.B;
    for (int b = 0; b < B; ++b) {
        const int v = valid ? valid[b] : n;
        if (v < 0 || v > n) return sfail(fn, "valid[b] must lie in [0, n]");
        if (st.ended[b] && v != 0) return sfail(fn, "an utterance that has ended must be given valid[b] = 0");
    }
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < B; ++b) {
        const int v = valid ? valid[b] : n;
        st.len[b] += v;
        if (v < n || last) st.ended[b] = 1;
    }
    if (n > 0) {
        const size_t rb = sizeof(float) * (size_t)n * m->D;
        HIP_CHECK_RET(hipMemcpy2DAsync(sb.xbuf + (int64_t)st.recv * m->D, sizeof(float) * (size_t)st.max_frames * m->D, xs, rb, rb, B,
                                       hipMemcpyDeviceToDevice, s));
    }
    st.recv += n; st.last = last != 0;
    {   // frames received and klen = frames / 4 of every utterance, through the next pinned staging slot
        const int slot = m->stage_slot; m->stage_slot = (slot + 1) & 3;
        HIP_CHECK_RET(hipEventSynchronize(m->stage_ev[slot]));
        int* h = m->h_stage + (int64_t)slot * m->stage_ints;
        for (int b = 0; b < B; ++b) { h[b] = st.len[b]; h[B + b] = st.len[b] / 4; }
        HIP_CHECK_RET(hipMemcpyAsync(sb.lens, h, sizeof(int) * 2 * (size_t)B, hipMemcpyHostToDevice, s));
        HIP_CHECK_RET(hipEventRecord(m->stage_ev[slot], s));
    }
    // every chunk whose window is complete; with `last` all that remain (a final partial chunk; the trailing T % 4 frames make no frame)
    for (;;) {
        const int s0 = st.emitted;
        int e = s0 + st.c;
        if (st.last) { if (s0 >= st.recv / 4) break; e = std::min(e, st.recv / 4); }
        else if (st.recv < 4 * e + 8) break;
        CK(stream_step(m, sb, s0, e, s));
        st.emitted = e;
    }
    if (st.beam) CK(mk_ctc_beam_run_advance(fn, st.beam, st.emitted, s));      // once per feed, whatever the cut
    if (frames_out) *frames_out = st.emitted;
    return 0;
}

int masr_stream_partial(masr_model* m, const int32_t** tokens, const int32_t** frames, const int32_t** lens, int* ld) {
    const char* fn = "masr_stream_partial";
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    if (!tokens || !frames || !lens || !ld) return sfail(fn, "null pointer");
    *tokens = sb.tokens; *frames = sb.frames; *lens = sb.state + m->stream.B; *ld = sb.cap;
    return 0;
}

int masr_stream_logits(masr_model* m, const float** logits, int64_t* ld, const int32_t** enc_lens, int* frames) {
    const char* fn = "masr_stream_logits";
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    if (!logits || !ld || !enc_lens || !frames) return sfail(fn, "null pointer");
    *logits = sb.logits; *ld = m->Cp; *enc_lens = sb.lens + m->stream.B; *frames = m->stream.emitted;
    return 0;
}

int masr_stream_ctc_beam(masr_model* m, int K, int nbest, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    const char* fn = "masr_stream_ctc_beam";
    if (!m) return sfail(fn, "null model");
    if (!(m->ctc_w > 0.f)) return sfail(fn, "the model has no CTC head (masr_create_ctc)");
    if (K < 1 || K > 64) return sfail(fn, "beam size K must be in [1, 64]");
    if (nbest < 1 || nbest > K) return sfail(fn, "nbest must be in [1, K]");
    if (!tokens || !lens || !scores) return sfail(fn, "null pointer");
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    if (!m->stream.last) return sfail(fn, "the stream has not had its last piece");
    return mk_ctc_beam_search(sb.logits, m->Cp, sb.lens + m->stream.B, m->stream.B, sb.cap, m->C, K, nbest, 0, m->C - 1, sb.work, sb.work_bytes, tokens,
                              lens, scores, (hipStream_t)stream);
}

int masr_stream_beam_open(masr_model* m, int K, const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* stream) {
    const char* fn = "masr_stream_beam_open";
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    masr_model::Stream& st = m->stream;
    masr_ctc_beam_run* run = mk_ctc_beam_run_open(fn, sb.logits, m->Cp, sb.lens + st.B, st.B, sb.cap, m->C, K, 0, m->C - 1, lm, lm_w, len_bonus, bias,
                                                  bias_w, sb.beam_work, sb.beam_work_bytes, (hipStream_t)stream);
    if (!run) return -1;
    // the frames emitted so far at once: after the last piece no feed would come to catch up with
    if (mk_ctc_beam_run_advance(fn, run, st.emitted, (hipStream_t)stream) != 0) { mk_ctc_beam_run_close(run); return -1; }
    mk_ctc_beam_run_close(st.beam);
    st.beam = run;
    return 0;
}

int masr_stream_beam_result(masr_model* m, int nbest, int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias, void* stream) {
    const char* fn = "masr_stream_beam_result";
    StreamBufs sb;
    CK(open_stream(fn, m, sb));
    if (!m->stream.beam) return sfail(fn, "no open beam (masr_stream_beam_open)");
    return mk_ctc_beam_run_result(fn, m->stream.beam, nbest, tokens, lens, scores, am, nbias, (hipStream_t)stream);
}

}  // extern "C"
