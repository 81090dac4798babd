// libmasr engine: the VGG-Transformer encoder-decoder of the reference (MyTransformer,
// src/model/transformer_pytorch/mono_transformer_torch.py) orchestrated as fixed sequences of hand-written gfx950
// kernels on one HIP stream, behind the C ABI of include/masr.h.  This file: the model behind the handle, its parameter
// table, the arena plans, bind / refresh, setters, stats, and the optimiser / utility wrappers.  The training step
// is train.hip, the decoders recog.hip, the streaming first pass stream_engine.hip, the standalone kernel entry points test_abi.hip;
// engine_internal.h is what they share.
//
// Memory model (sized for 288 GB HBM3E): ONE flat fp32 parameter buffer and ONE flat gradient buffer
// (caller-owned; every optimiser / clip / all-reduce is a single streaming pass), bf16 operand shadows
// of the weights (refreshed after each parameter update), and a bump-allocated activation arena that
// keeps every activation of the step resident (nothing is recomputed, nothing is re-read through host).
// Activations are batch-first row matrices [B*T][E]; conv activations are NHWC bf16.
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "engine_internal.h"
#include "nlm.h"

static thread_local std::string g_err;
void mk_set_error(const char* what, const char* detail) { g_err = std::string(what) + ": " + detail; }

namespace {

int64_t add_param(masr_model* m, const std::string& name, std::initializer_list<int64_t> shape) {
    PInfo p; p.name = name; p.ndim = (int)shape.size(); p.numel = 1;
    int i = 0; for (auto s : shape) { p.shape[i++] = s; p.numel *= s; }
    for (; i < 4; ++i) p.shape[i] = 1;
    p.off = m->nparams; m->nparams += p.numel;
    m->params.push_back(p);
    return p.off;
}
Lin add_linear(masr_model* m, const std::string& pre, int N, int K, const char* wname = ".weight", const char* bname = ".bias") {
    Lin l{}; l.N = N; l.K = K;
    l.w = add_param(m, pre + wname, {N, K});
    l.b = add_param(m, pre + bname, {N});
    return l;
}
Norm add_norm(masr_model* m, const std::string& pre) {
    Norm n; n.w = add_param(m, pre + ".weight", {m->E}); n.b = add_param(m, pre + ".bias", {m->E}); return n;
}
Attn add_attn(masr_model* m, const std::string& pre) {
    Attn a;
    a.in = add_linear(m, pre, 3 * m->E, m->E, ".in_proj_weight", ".in_proj_bias");
    a.out = add_linear(m, pre + ".out_proj", m->E, m->E);
    return a;
}

// ------------------------------------------------------------------ persistent region (shadows, stats)
void plan_persistent(masr_model* m, Arena& ar) {
    for (int i = 1; i < 4; ++i) {
        m->conv[i].k16 = ar.get<bf16>((int64_t)m->conv[i].CO * 9 * m->conv[i].CI);
        m->conv[i].d16 = ar.get<bf16>((int64_t)m->conv[i].CO * 9 * m->conv[i].CI);
    }
    auto lin = [&](Lin& l) {
        const int Np = (l.N + 7) / 8 * 8;
        l.k16 = ar.get<bf16>((int64_t)Np * l.K);
        l.t16 = ar.get<bf16>((int64_t)l.K * Np);
    };
    m->v2e_k = ar.get<bf16>((int64_t)m->E * m->F);
    m->v2e.t16 = ar.get<bf16>((int64_t)m->F * m->E);
    m->ct.k16 = ar.get<bf16>((int64_t)m->Cp * m->E);
    m->ct.t16 = ar.get<bf16>((int64_t)m->E * m->Cp);
    for (auto& e : m->enc) { lin(e.sa.in); lin(e.sa.out); lin(e.l1); lin(e.l2); }
    for (auto& d : m->dec) {
        lin(d.sa.in); lin(d.sa.out); lin(d.ca.out); lin(d.l1); lin(d.l2);
        d.ca.q_k16 = ar.get<bf16>((int64_t)m->E * m->E); d.ca.q_t16 = ar.get<bf16>((int64_t)m->E * m->E);
        d.ca.in.k16 = d.ca.in.t16 = nullptr;                        // (the packed in_proj of a cross-attention has no shadow of its own)
    }
    m->NK = m->ND * 2 * m->E;
    m->kv_k16 = ar.get<bf16>((int64_t)m->NK * m->E); m->kvT = ar.get<bf16>((int64_t)m->E * m->NK); m->kv_bias = ar.get<float>(m->NK);
    m->stats = ar.get<float>(64);
    m->conv_sched = ar.get<unsigned>(64);
    if (m->ctc_w > 0.f) { m->ctc.k16 = ar.get<bf16>((int64_t)m->Cp * m->E); m->ctc.t16 = ar.get<bf16>((int64_t)m->E * m->Cp); }   // (pads zeroed in masr_bind)
}

}  // namespace

// ------------------------------------------------------------------ activation plan
void plan_acts(const masr_model* m, Arena& ar, Acts& a, int B, int T, int L, bool train, bool ctc) {
    const int E = m->E, Fi = m->Fi, H = m->H;
    a.B = B; a.T = T; a.D = m->D; a.H2 = T / 2; a.W2 = m->D / 2; a.Tp = a.H2 / 2; a.Dp = a.W2 / 2; a.L = L;
    a.rows_e = B * a.Tp; a.rows_d = B * L;
    const int64_t re = a.rows_e, rd = a.rows_d;
    const bool hybrid = m->ctc_w > 0.f;
    a.tok_in = ar.get<int>(3 * rd + B + 8 + m->C + 1 + (hybrid ? 2 * B : 0) + (m->aug_on ? B : 0)); a.gold = a.tok_in + rd; a.enc_lens = a.gold + rd;   // one block: one H2D copy per step
    a.meta = reinterpret_cast<uint32_t*>(a.enc_lens + B);
    a.tok_order = a.enc_lens + B + 8; a.tok_start = a.tok_order + rd;
    a.ctc_tgt = hybrid ? a.tok_start + m->C + 1 : nullptr;
    a.raw_lens = m->aug_on ? a.tok_start + m->C + 1 + (hybrid ? 2 * B : 0) : nullptr;
    a.step_dev = ar.get<int>(4);
    a.step_qkv = ar.get<bf16>((int64_t)B * 3 * E);
    const int64_t P1 = (int64_t)B * T * m->D, P2 = (int64_t)B * a.H2 * a.W2;
    a.a1 = ar.get<bf16>(P1 * 64); a.p1 = ar.get<bf16>(P2 * 64);      // (the maps in front of the pools, a2 and a4, are never stored: pooled map + codes)
    a.a1_bits = ar.get<unsigned long long>(P1); a.a3_bits = ar.get<unsigned long long>(P2 * 2);      // (64 / 128 sign bits per pixel)
    a.a3 = ar.get<bf16>(P2 * 128); a.p2 = ar.get<bf16>(re * m->F);
    a.i1 = ar.get<uint8_t>(P2 * 64); a.i2 = ar.get<uint8_t>(re * m->F);
    a.x32.resize(m->NE + 1); a.x16.resize(m->NE + 1); a.enc.resize(m->NE);
    for (int l = 0; l <= m->NE; ++l) { a.x32[l] = ar.get<float>(re * E); a.x16[l] = ar.get<bf16>(re * E); }
    for (auto& e : a.enc) {
        e.qkv = ar.get<bf16>(re * 3 * E); e.ao = ar.get<bf16>(re * E); e.lse = ar.get<float>((int64_t)B * H * a.Tp);
        e.s1 = ar.get<float>(re * E); e.x1_32 = ar.get<float>(re * E); e.x1_16 = ar.get<bf16>(re * E);
        e.m1 = ar.get<float>(re); e.r1 = ar.get<float>(re); e.f = ar.get<bf16>(re * Fi);
        e.s2 = ar.get<float>(re * E); e.m2 = ar.get<float>(re); e.r2 = ar.get<float>(re);
    }
    a.mf = ar.get<float>(re); a.rf = ar.get<float>(re); a.mem16 = ar.get<bf16>(re * E);
    a.kv_all = ar.get<bf16>(re * m->NK);
    a.y32.resize(m->ND + 1); a.y16.resize(m->ND + 1); a.dec.resize(m->ND);
    for (int l = 0; l <= m->ND; ++l) { a.y32[l] = ar.get<float>(rd * E); a.y16[l] = ar.get<bf16>(rd * E); }
    for (auto& d : a.dec) {
        d.qkv = ar.get<bf16>(rd * 3 * E); d.ao = ar.get<bf16>(rd * E); d.lse_s = ar.get<float>((int64_t)B * H * L);
        d.s1 = ar.get<float>(rd * E); d.y1_32 = ar.get<float>(rd * E); d.y1_16 = ar.get<bf16>(rd * E);
        d.m1 = ar.get<float>(rd); d.r1 = ar.get<float>(rd);
        d.q = ar.get<bf16>(rd * E); d.kv = nullptr; d.co = ar.get<bf16>(rd * E); d.lse_c = ar.get<float>((int64_t)B * H * L);
        d.s2 = ar.get<float>(rd * E); d.y2_32 = ar.get<float>(rd * E); d.y2_16 = ar.get<bf16>(rd * E);
        d.m2 = ar.get<float>(rd); d.r2 = ar.get<float>(rd);
        d.f = ar.get<bf16>(rd * Fi); d.s3 = ar.get<float>(rd * E); d.m3 = ar.get<float>(rd); d.r3 = ar.get<float>(rd);
    }
    if (a.kv_all) for (int l = 0; l < m->ND; ++l) a.dec[l].kv = a.kv_all + (int64_t)l * 2 * E;
    a.mdf = ar.get<float>(rd); a.rdf = ar.get<float>(rd); a.yf16 = ar.get<bf16>(rd * E);
    a.logits = ar.get<float>(rd * m->Cp); a.dlogits = ar.get<bf16>(rd * m->Cp);
    a.row_loss = ar.get<float>(rd); a.row_correct = ar.get<int>(rd);
    // slab: max over all users
    int64_t sl = mk_sumsq_slab_floats(m->nparams);
    auto mx = [&](int64_t v) { if (v > sl) sl = v; };
    mx(mk_layernorm_bwd_slab_floats((int)(re > rd ? re : rd), E));
    mx(mk_colsum_slab_floats((int)P1, 64)); mx(mk_colsum_slab_floats((int)P2, 128));
    mx(mk_colsum_slab_floats((int)(re > rd ? re : rd), 3 * E > Fi ? 3 * E : Fi));
    a.slab_floats = sl; a.slab = ar.get<float>(sl);
    a.part = ar.get<float>((int64_t)KSPLIT_MAX * rd * E);
    if (train) {
        const int nln = 2 * m->NE + 1 + 3 * m->ND + 1;
        a.ln_slab_floats = 0;
        for (int i = 0; i < nln; ++i) a.ln_slab_floats += mk_layernorm_bwd_slab_floats((int)(i < 2 * m->NE + 1 ? re : rd), E);
        a.ln_slab = ar.get<float>(a.ln_slab_floats);
        a.cw_slab[0] = ar.get<float>(mk_conv3x3_wgrad_slab_floats(B, T, m->D, 64, 64));
        a.cw_slab[1] = ar.get<float>(mk_conv3x3_wgrad_slab_floats(B, a.H2, a.W2, 64, 128));
        a.cw_slab[2] = ar.get<float>(mk_conv3x3_wgrad_slab_floats(B, a.H2, a.W2, 128, 128));
        a.c1_slab = ar.get<float>(mk_conv1_wgrad_fused_slab_floats(B, T, m->D));
        a.ge_a = ar.get<float>(re * E); a.ge_b = ar.get<float>(re * E); a.gd_a = ar.get<float>(rd * E); a.gd_b = ar.get<float>(rd * E);
        a.dmem32 = ar.get<float>(re * E); a.v2e_g32 = ar.get<float>((int64_t)E * m->F);
        a.ge16 = ar.get<bf16>(re * E);
        a.gao_e = ar.get<bf16>(re * E); a.gao_d = ar.get<bf16>(rd * E);
        a.gkv_all = ar.get<bf16>(re * m->NK);
        a.delta_e = ar.get<float>((int64_t)B * H * a.Tp); a.delta_d = ar.get<float>((int64_t)B * H * L);
        a.egr.resize(m->NE);
        for (auto& g : a.egr) { g.g2 = ar.get<bf16>(re * E); g.g1 = ar.get<bf16>(re * E); g.gf = ar.get<bf16>(re * Fi); g.gqkv = ar.get<bf16>(re * 3 * E); }
        a.dgr.resize(m->ND);
        for (auto& g : a.dgr) {
            g.g3 = ar.get<bf16>(rd * E); g.g2 = ar.get<bf16>(rd * E); g.g1 = ar.get<bf16>(rd * E);
            g.gf = ar.get<bf16>(rd * Fi); g.gq = ar.get<bf16>(rd * E); g.gqkv = ar.get<bf16>(rd * 3 * E);
        }
        a.dp2 = ar.get<bf16>(re * m->F); a.da3 = ar.get<bf16>(P2 * 128); a.dp1 = ar.get<bf16>(P2 * 64);
    }
    a.ctc_logits = a.ctc_nll = a.ctc_work = nullptr; a.ctc_d16 = nullptr; a.ctc_maxS = 0;
    if (hybrid && ctc) {                                       // (behind everything else: the plain model's plan is unchanged)
        a.ctc_maxS = 2 * (L - 1) + 1;                           // 2 max(olen) + 1 lattice states
        a.ctc_logits = ar.get<float>(re * m->Cp);
        a.ctc_nll = ar.get<float>(B);
        a.ctc_work = ar.get<float>(mk_ctc_work_floats(a.Tp, B, a.ctc_maxS));
        a.ctc_d16 = train ? ar.get<bf16>(re * m->Cp) : nullptr;
    }
    a.xa = (m->aug_on && ctc && train) ? ar.get<float>(P1) : nullptr;      // (last: every other offset is the policy-free plan's)
}

const char* specaug_policy_error(const masr_specaug_policy& p, int D) {
    if (p.time_warp < 0) return "time_warp must be >= 0";
    if (p.freq_masks < 0 || p.freq_masks > 8) return "freq_masks must lie in [0, 8]";
    if (p.freq_width < 0) return "freq_width must be >= 0";
    const bool off = !p.time_warp && !p.freq_masks && !p.time_masks;
    if (!(off && p.freq_bins == 0) && (p.freq_bins < 1 || p.freq_bins > D)) return "freq_bins must lie in [1, D]";     // (an all-zero policy is "off")
    if (p.time_masks < 0 || p.time_masks > 8) return "time_masks must lie in [0, 8]";
    if (p.time_width < 0) return "time_width must be >= 0";
    if (!(p.time_ratio >= 0.f && p.time_ratio <= 1.f)) return "time_ratio must lie in [0, 1]";
    return nullptr;
}

// =========================================================================== C ABI
extern "C" {

int masr_version(void) { return 1; }
const char* masr_last_error(void) { return g_err.c_str(); }

masr_model* masr_create(const masr_config* cfg) {
    if (!cfg || cfg->d_model % cfg->nheads || cfg->d_model % 8 || cfg->d_inner % 8 || cfg->idim < 4) {
        mk_set_error("masr_create", "bad config"); return nullptr;
    }
    const int hd = cfg->d_model / cfg->nheads;
    if (hd != 16 && hd != 32 && hd != 64) { mk_set_error("masr_create", "head dim must be 16/32/64"); return nullptr; }
    if (cfg->d_model % 64) { mk_set_error("masr_create", "d_model must be a multiple of 64"); return nullptr; }
    if (cfg->d_model > 1024 || cfg->d_inner > 2048 || 3 * cfg->d_model > 2048) {
        mk_set_error("masr_create", "d_model <= 682, d_inner <= 2048 supported"); return nullptr;
    }
    masr_model* m = new masr_model();
    m->cfg = *cfg; m->E = cfg->d_model; m->H = cfg->nheads; m->hd = hd; m->Fi = cfg->d_inner; m->NE = cfg->enc_layers;
    m->ND = cfg->dec_layers; m->C = cfg->odim; m->Cp = (cfg->odim + 127) / 128 * 128; m->D = cfg->idim;
    m->Dp = (cfg->idim / 2) / 2; m->F = 128 * m->Dp;
    // state_dict order of the reference
    const int idx[4] = {0, 2, 5, 7}; const int co[4] = {64, 64, 128, 128}, ci[4] = {1, 64, 64, 128};
    for (int i = 0; i < 4; ++i) {
        Conv& c = m->conv[i]; c.CO = co[i]; c.CI = ci[i]; c.k16 = c.d16 = nullptr;
        const std::string pre = "feat_extractor." + std::to_string(idx[i]);
        c.w = add_param(m, pre + ".weight", {co[i], ci[i], 3, 3});
        c.b = add_param(m, pre + ".bias", {co[i]});
    }
    m->v2e = add_linear(m, "vgg2enc", m->E, 128 * (cfg->idim / 4));
    m->ct = add_linear(m, "char_trans", m->C, m->E);
    m->embed_w = cfg->tie_weights ? m->ct.w : add_param(m, "pre_embed.weight", {m->C, m->E});
    m->enc.resize(m->NE);
    for (int l = 0; l < m->NE; ++l) {
        const std::string pre = "encoder.layers." + std::to_string(l);
        EncL& e = m->enc[l];
        e.sa = add_attn(m, pre + ".self_attn");
        e.l1 = add_linear(m, pre + ".linear1", m->Fi, m->E); e.l2 = add_linear(m, pre + ".linear2", m->E, m->Fi);
        e.n1 = add_norm(m, pre + ".norm1"); e.n2 = add_norm(m, pre + ".norm2");
    }
    m->enc_norm = add_norm(m, "encoder.norm");
    m->dec.resize(m->ND);
    for (int l = 0; l < m->ND; ++l) {
        const std::string pre = "decoder.layers." + std::to_string(l);
        DecL& d = m->dec[l];
        d.sa = add_attn(m, pre + ".self_attn"); d.ca = add_attn(m, pre + ".multihead_attn");
        d.l1 = add_linear(m, pre + ".linear1", m->Fi, m->E); d.l2 = add_linear(m, pre + ".linear2", m->E, m->Fi);
        d.n1 = add_norm(m, pre + ".norm1"); d.n2 = add_norm(m, pre + ".norm2"); d.n3 = add_norm(m, pre + ".norm3");
    }
    m->dec_norm = add_norm(m, "decoder.norm");
    Arena ar{nullptr, 0, 0};
    plan_persistent(m, ar);
    m->persist_bytes = ar.off;
    m->stage_ints = 1 << 16;
    for (auto& e : m->stage_ev) e = nullptr;
    for (int i = 0; i < masr_model::RING; ++i) { m->ring_ev[i] = nullptr; m->ring_used[i] = false; }
    return m;
}

masr_model* masr_create_ctc(const masr_config* cfg, float ctc_weight) {
    if (!(ctc_weight >= 0.f && ctc_weight < 1.f)) { mk_set_error("masr_create_ctc", "ctc_weight must lie in [0, 1)"); return nullptr; }
    masr_model* m = masr_create(cfg);
    if (!m || ctc_weight == 0.f) return m;
    if (m->C > 4096) { mk_set_error("masr_create_ctc", "the CTC lattice supports odim <= 4096"); masr_destroy(m); return nullptr; }
    // the head goes behind every parameter of the plain model (its offsets, and those of the persistent region, stay put)
    m->ctc_w = ctc_weight;
    m->ctc = add_linear(m, "ctc.ctc_lo", m->C, m->E);
    Arena ar{nullptr, 0, 0};
    plan_persistent(m, ar);
    m->persist_bytes = ar.off;
    return m;
}

void masr_destroy(masr_model* m) {
    if (!m) return;
    stream_close(m);
    if (m->h_stage) hipHostFree(m->h_stage);
    if (m->h_stats) hipHostFree(m->h_stats);
    for (int i = 0; i < masr_model::RING; ++i) if (m->ring_ev[i]) { if (m->ring_used[i]) hipEventSynchronize(m->ring_ev[i]); hipEventDestroy(m->ring_ev[i]); }
    if (m->h_ring) hipHostFree(m->h_ring);
    for (DecodeGraph& g : m->decode_graphs) g.destroy();
    for (auto& sg : m->step_graphs) { hipGraphExecDestroy(sg.e); hipGraphDestroy(sg.g); }
    for (auto& e : m->stage_ev) if (e) hipEventDestroy(e);
    for (auto& v : m->prof_ev) for (auto& p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    delete m;
}

int64_t masr_param_numel(const masr_model* m) { return m->nparams; }
int masr_param_count(const masr_model* m) { return (int)m->params.size(); }
int masr_param_info(const masr_model* m, int idx, char* name, int cap, int64_t shape[4], int* ndim, int64_t* offset) {
    if (idx < 0 || idx >= (int)m->params.size()) { mk_set_error("masr_param_info", "index out of range"); return -1; }
    const PInfo& p = m->params[idx];
    if (name && cap > 0) { std::strncpy(name, p.name.c_str(), cap - 1); name[cap - 1] = 0; }
    for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
    *ndim = p.ndim; *offset = p.off;
    return 0;
}

int64_t masr_workspace_bytes(const masr_model* m, int B, int T, int L) {
    Arena ar{nullptr, 0, 0};
    Acts a;
    plan_acts(m, ar, a, B, T, L, true, true);
    return m->persist_bytes + ar.off + 4096;
}

int masr_bind(masr_model* m, float* params, float* grads, const float* pe, void* workspace, int64_t ws_bytes) {
    if (!params || !grads || !pe || !workspace || ws_bytes < m->persist_bytes) { mk_set_error("masr_bind", "null pointer or workspace too small"); return -1; }
    if (((uintptr_t)workspace & 255) || ((uintptr_t)params & 15) || ((uintptr_t)grads & 15)) { mk_set_error("masr_bind", "misaligned buffers"); return -1; }
    m->P = params; m->G = grads; m->pe = pe; m->ws = (char*)workspace; m->ws_bytes = ws_bytes;
    stream_close(m);
    Arena ar{m->ws, ws_bytes, 0};
    plan_persistent(m, ar);
    if (!m->h_stage) {
        HIP_CHECK_RET(hipHostMalloc((void**)&m->h_stage, sizeof(int) * m->stage_ints * 4, hipHostMallocDefault));
        HIP_CHECK_RET(hipHostMalloc((void**)&m->h_stats, sizeof(float) * 64, hipHostMallocDefault));
        for (auto& e : m->stage_ev) HIP_CHECK_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_CHECK_RET(hipHostMalloc((void**)&m->h_ring, sizeof(float) * 4 * masr_model::RING, hipHostMallocDefault));
        for (auto& e : m->ring_ev) HIP_CHECK_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    {   // device tables: the job list of the one-launch shadow refresh
        // the list travels BY VALUE in the kernel arguments (kernels.h), which caps one launch at SHADOW_JOBS_MAX jobs: deeper
        // models (8e4d = 69 jobs) simply take a second launch
        m->shadows.clear();
        auto job = [&](int type, long src, int N, int K, int ldt, int a0, int a1, void* p0, void* p1) {
            if (m->shadows.empty() || m->shadows.back().n == SHADOW_JOBS_MAX) { m->shadows.emplace_back(); m->shadows.back().n = 0; m->shadows.back().blocks = 0; }
            ShadowJobs& J = m->shadows.back();
            ShadowDesc d{}; d.src = src; d.type = type; d.N = N; d.K = K; d.ldt = ldt; d.a0 = a0; d.a1 = a1; d.tile_start = J.blocks;
            J.blocks += mk_shadow_blocks(d);
            J.d[J.n] = d; J.p[2 * J.n] = (bf16*)p0; J.p[2 * J.n + 1] = (bf16*)p1; ++J.n;
        };
        auto lin = [&](const Lin& l) { job(SH_LINEAR, l.w, l.N, l.K, (l.N + 7) / 8 * 8, 0, 0, l.k16, l.t16); };
        const int E = m->E;
        for (int i = 1; i < 4; ++i) job(SH_CONV, m->conv[i].w, m->conv[i].CO, m->conv[i].CI, 0, 0, 0, m->conv[i].k16, m->conv[i].d16);
        job(SH_VGG2ENC, m->v2e.w, E, 0, 0, 128, m->Dp, m->v2e_k, m->v2e.t16);
        job(SH_LINEAR, m->ct.w, m->C, E, m->Cp, 0, 0, m->ct.k16, m->ct.t16);     // pads (rows / columns >= odim) stay zero, see below
        for (auto& e : m->enc) { lin(e.sa.in); lin(e.sa.out); lin(e.l1); lin(e.l2); }
        for (int l = 0; l < m->ND; ++l) {
            const DecL& d = m->dec[l];
            lin(d.sa.in); lin(d.sa.out); lin(d.ca.out); lin(d.l1); lin(d.l2);
            job(SH_LINEAR, d.ca.in.w, E, E, E, 0, 0, d.ca.q_k16, d.ca.q_t16);                                              // query third
            job(SH_LINEAR, d.ca.in.w + (long)E * E, 2 * E, E, m->NK, 0, 0, m->kv_k16 + (long)l * 2 * E * E, m->kvT + (long)l * 2 * E);   // key|value thirds
            job(SH_COPY32, d.ca.in.b + E, 2 * E, 0, 0, 0, 0, m->kv_bias + (long)l * 2 * E, nullptr);
        }
        if (m->ctc_w > 0.f) job(SH_LINEAR, m->ctc.w, m->C, E, m->Cp, 0, 0, m->ctc.k16, m->ctc.t16);     // CTC head (pads zero, as char_trans)
    }
    // pads of the char_trans shadows must be zero (rows/cols >= odim); the refresh kernels only write the odim part
    HIP_CHECK_RET(hipMemset(m->conv_sched, 0, sizeof(unsigned) * 64));   // tile counters of the streaming conv (re-armed by the kernel itself)
    HIP_CHECK_RET(hipMemset(m->ct.k16, 0, sizeof(bf16) * (size_t)m->Cp * m->E));
    HIP_CHECK_RET(hipMemset(m->ct.t16, 0, sizeof(bf16) * (size_t)m->E * m->Cp));
    if (m->ctc_w > 0.f) {
        HIP_CHECK_RET(hipMemset(m->ctc.k16, 0, sizeof(bf16) * (size_t)m->Cp * m->E));
        HIP_CHECK_RET(hipMemset(m->ctc.t16, 0, sizeof(bf16) * (size_t)m->E * m->Cp));
    }
    m->have_acts = false; m->last_rescore = {};
    return 0;
}

void masr_set_seed(masr_model* m, uint64_t seed) { m->seed = seed; m->step = 0; }
// captured steps hold the launch geometry of the settings they were captured under: every setter that changes it drops them (after the
// device has drained: nothing of a graph may be in flight when it is destroyed)
static void drop_step_graphs(masr_model* m) {
    if (m->step_graphs.empty()) return;
    hipDeviceSynchronize();
    for (auto& sg : m->step_graphs) { hipGraphExecDestroy(sg.e); hipGraphDestroy(sg.g); }
    m->step_graphs.clear();
    m->last_key[3] = -1; m->last_xs = nullptr;
}
// (no RESULT depends on the number of task slots -- "K task slots == the sequential run, bit for bit" is a guarantee of --tasks_per_gpu, and
// every partition into partial sums is fixed per shape and per masr_set_ksplit; what follows the hint is the LDS footprint of a few launches:
// GemmArgs::lean -- and the size of the training step's persistent conv grids: ConvArgs::shared / ConvWgradArgs::shared cap them at 5/8 (tile-counter
// kernels) and 1/2 (static-walk weight-gradient kernels) of the CUs from THREE slots on; one and two slots are never capped; conv_grid_limit in
// conv.hip)
void masr_set_concurrency(masr_model* m, int slots) { slots = slots < 1 ? 1 : slots; if (slots != m->slots) drop_step_graphs(m); m->slots = slots; }
void masr_dropout_state(masr_model* m, uint64_t state[2], int set) {
    if (set) { m->seed = state[0]; m->step = state[1]; } else { state[0] = m->seed; state[1] = m->step; }
}

int masr_refresh(masr_model* m, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!m->P) { mk_set_error("masr_refresh", "not bound"); return -1; }
    Prof p(m, MASR_PROF_SHADOWS, s);
    // every bf16 operand shadow (conv forward/dgrad layouts, permuted vgg2enc, all Linear weights and their transposes, the
    // gathered cross-attention K/V operand) in ONE launch; the pads of the char_trans shadows are zeroed once in masr_bind
    for (const ShadowJobs& J : m->shadows) CK(mk_all_shadows(m->P, J, s));
    return 0;
}

int masr_set_specaug(masr_model* m, const masr_specaug_policy* p) {
    masr_specaug_policy q{};
    if (p) q = *p;
    if (const char* bad = specaug_policy_error(q, m->D)) { mk_set_error("masr_set_specaug", bad); return -1; }
    const bool on = q.time_warp > 0 || q.freq_masks > 0 || q.time_masks > 0;
    if (on != m->aug_on || (on && memcmp(&q, &m->aug, sizeof q))) drop_step_graphs(m);       // (the policy is a kernel argument of the captured launch)
    if (on != m->aug_on) m->aug_ran = false;                                                  // the next plan differs: the upload block and the batch buffer
    m->aug = q; m->aug_on = on;
    return 0;
}
int masr_chunk_draw(uint64_t seed, uint64_t step, int Tp) { return chunk_draw_of(step_seed_of(seed, step), Tp); }
int masr_set_chunk(masr_model* m, const masr_chunk_policy* p) {
    masr_chunk_policy q{0, -1, 0};
    if (p) q = *p;
    if (q.size < 0 || q.left < -1 || (q.dynamic != 0 && q.dynamic != 1)) { mk_set_error("masr_set_chunk", "need size >= 0, left >= -1, dynamic in {0, 1}"); return -1; }
    const bool on = q.size > 0 || q.dynamic != 0;
    if (!on) q = masr_chunk_policy{0, -1, 0};
    if (on != m->chunk_on || memcmp(&q, &m->chunk, sizeof q)) drop_step_graphs(m);            // (chunk and left are kernel arguments of the captured launches)
    m->chunk = q; m->chunk_on = on;
    stream_close(m);                                                                          // (an open stream was planned for the old chunk)
    return 0;
}
int masr_chunk_last(masr_model* m, int* size) {
    if (m->chunk_last < 0 || !size) { mk_set_error("masr_chunk_last", "no encoder forward yet (or a null pointer)"); return -1; }
    *size = m->chunk_last;
    return 0;
}
int masr_specaug_last(masr_model* m, const float** xa, int* B, int* T, int* D) {
    if (!m->have_acts || !m->aug_ran || !m->acts.xa) { mk_set_error("masr_specaug_last", "the last step did not augment (no policy, MASR_EVAL, or no step yet)"); return -1; }
    *xa = m->acts.xa; *B = m->acts.B; *T = m->acts.T; *D = m->acts.D;
    return 0;
}
int masr_specaug(const float* xs, const int32_t* lens_dev, float* out, int B, int T, int D, const masr_specaug_policy* p, uint64_t seed, uint64_t step,
                 void* stream) {
    if (!xs || !lens_dev || !out || !p) { mk_set_error("masr_specaug", "null pointer"); return -1; }
    if (out == xs) { mk_set_error("masr_specaug", "out must be another buffer than xs (the warp reads neighbouring rows)"); return -1; }
    if (B < 1 || B > 65535 || T < 1 || D < 1) { mk_set_error("masr_specaug", "need 1 <= B <= 65535, T >= 1, D >= 1"); return -1; }
    if ((int64_t)T * T > INT32_MAX || (int64_t)T * D > INT32_MAX) { mk_set_error("masr_specaug", "T * T and T * D must fit an int"); return -1; }
    if (const char* bad = specaug_policy_error(*p, D)) { mk_set_error("masr_specaug", bad); return -1; }
    return mk_specaug(xs, lens_dev, out, B, T, D, *p, step_seed_of(seed, step), nullptr, (hipStream_t)stream);
}

void masr_set_step_graphs(masr_model* m, int on) { m->step_graphs_on = on != 0; }
void masr_set_split_wgrad_launches(masr_model* m, int on) { if ((on != 0) != m->split_wgrad) drop_step_graphs(m); m->split_wgrad = on != 0; }
void masr_set_ksplit(masr_model* m, int on) { if ((on != 0) != m->ksplit) drop_step_graphs(m); m->ksplit = on != 0; }
void masr_set_drop_nan_grads(masr_model* m, int on) { m->drop_nan_grads = on != 0; }
void masr_step_counters(const masr_model* m, int64_t out[4]) { out[0] = m->n_direct; out[1] = m->n_captured; out[2] = m->n_replayed; out[3] = m->n_ksplit; }

int masr_read_stats(masr_model* m, float out[4], void* stream) {
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK_RET(hipMemcpyAsync(m->h_stats, m->stats, sizeof(float) * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK_RET(hipStreamSynchronize(s));
    for (int i = 0; i < 4; ++i) out[i] = m->h_stats[i];
    return 0;
}

const float* masr_stats_device(masr_model* m) { return m ? m->stats : nullptr; }
int64_t masr_stats_post(masr_model* m, void* stream) {
    if (!m->h_ring) { mk_set_error("masr_stats_post", "not bound"); return -1; }
    const int slot = (int)(m->ring_next % masr_model::RING);
    if (m->ring_used[slot]) HIP_CHECK_RET(hipEventSynchronize(m->ring_ev[slot]));     // the block's previous copy has landed (ticket long dropped or read)
    uint32_t* w = reinterpret_cast<uint32_t*>(m->h_ring + 4 * slot);
    for (int i = 0; i < 4; ++i) w[i] = MASR_STATS_PENDING;
    HIP_CHECK_RET(hipMemcpyAsync(m->h_ring + 4 * slot, m->stats, sizeof(float) * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_CHECK_RET(hipEventRecord(m->ring_ev[slot], (hipStream_t)stream));
    m->ring_used[slot] = true;
    return m->ring_next++;
}
const float* masr_stats_peek(masr_model* m, int64_t ticket) {
    if (!m->h_ring || ticket < 0 || ticket >= m->ring_next || m->ring_next - ticket > masr_model::RING) { mk_set_error("masr_stats_peek", "unknown or expired ticket"); return nullptr; }
    return m->h_ring + 4 * (ticket % masr_model::RING);
}
int masr_stats_wait(masr_model* m, int64_t ticket, float out[4]) {
    const float* p = masr_stats_peek(m, ticket);
    if (!p) return -1;
    HIP_CHECK_RET(hipEventSynchronize(m->ring_ev[ticket % masr_model::RING]));          // completion AND host visibility of the copy
    for (int i = 0; i < 4; ++i) out[i] = p[i];
    return 0;
}

int masr_last_logits(masr_model* m, const float** logits, const int32_t** gold, int* rows, int* L, int* ld) {
    if (!m->have_acts) { mk_set_error("masr_last_logits", "no forward has run"); return -1; }
    *logits = m->acts.logits; *gold = m->acts.gold; *rows = m->acts.rows_d; *L = m->acts.L; *ld = m->Cp;
    return 0;
}

static float* slab_of(masr_model* m) {
    // optimiser passes may run before any batch: fall back to the tail of the persistent stats block
    return m->have_acts ? m->acts.slab : nullptr;
}

int masr_grad_norm(masr_model* m, void* stream) {
    float* slab = slab_of(m);
    if (!slab) { mk_set_error("masr_grad_norm", "run a batch first"); return -1; }
    Prof p(m, MASR_PROF_OPTIM, (hipStream_t)stream);
    return mk_sumsq(m->G, m->nparams, slab, m->stats + 3, (hipStream_t)stream);
}
int masr_clip_sgd_step(masr_model* m, float* mom, float max_norm, float lr, float momentum, int nesterov, int first_step, void* stream) {
    CK(masr_grad_norm(m, stream));
    { Prof p(m, MASR_PROF_OPTIM, (hipStream_t)stream);
      CK(mk_clip_sgd(m->P, m->G, mom, m->nparams, m->stats + 3, max_norm, lr, momentum, nesterov, first_step, (hipStream_t)stream)); }
    return masr_refresh(m, stream);
}
int masr_clip_grads(masr_model* m, float max_norm, void* stream) {
    CK(masr_grad_norm(m, stream));
    return mk_clip_scale(m->G, m->nparams, m->stats + 3, max_norm, (hipStream_t)stream, m->drop_nan_grads);
}
int masr_clip_scale_flat(float* buf, int64_t n, const float* norm, float max_norm, void* stream) {
    return mk_clip_scale(buf, n, norm, max_norm, (hipStream_t)stream);
}
int masr_clip_accumulate(masr_model* m, float* updates, float max_norm, void* stream) {
    CK(masr_grad_norm(m, stream));
    return mk_clip_axpy(updates, m->G, m->nparams, m->stats + 3, max_norm, (hipStream_t)stream, m->drop_nan_grads);
}
int masr_adam_step(float* p, const float* g, float* ea, float* eas, int64_t n, float lr, float b1, float b2, float eps, int step, void* stream) {
    return mk_adam(p, g, ea, eas, n, lr, b1, b2, eps, step, 0.f, 0, (hipStream_t)stream);
}
int masr_adam_step_guarded(masr_model* m, float* p, const float* g, float* ea, float* eas, int64_t n, float lr_a, int t_a, float lr_b, int t_b,
                           float b1, float b2, float eps, float weight_decay, int decoupled, int slot, void* stream) {
    Prof pr(m, MASR_PROF_OPTIM, (hipStream_t)stream);
    return mk_adam_guarded(p, g, ea, eas, n, lr_a, t_a, lr_b, t_b, b1, b2, eps, weight_decay, decoupled, m->stats + 3,
                           reinterpret_cast<int*>(m->stats + 16), slot, (hipStream_t)stream);
}
int masr_adam_sum_step(float* p, const float* const* grads, int n_grads, float gscale, float* ea, float* eas, int64_t n, float lr, float b1,
                       float b2, float eps, int step, void* stream) {
    return mk_adam_sum(p, grads, n_grads, gscale, ea, eas, n, lr, b1, b2, eps, step, (hipStream_t)stream);
}
int masr_sum_n(float* out, const float* const* grads, int n_grads, float scale, int64_t n, void* stream) {
    return mk_sum_n(out, grads, n_grads, scale, n, (hipStream_t)stream);
}
int masr_adamw_step(float* p, const float* g, float* ea, float* eas, int64_t n, float lr, float b1, float b2, float eps, float weight_decay,
                    int decoupled, int step, void* stream) {
    return mk_adam(p, g, ea, eas, n, lr, b1, b2, eps, step, weight_decay, decoupled, (hipStream_t)stream);
}
int masr_radam_step(float* p, const float* g, float* ea, float* eas, int64_t n, float lr, float b1, float b2, float eps, float weight_decay,
                    int step, int variant, void* stream) {
    return mk_radam(p, g, ea, eas, n, lr, b1, b2, eps, step, weight_decay, variant, (hipStream_t)stream);
}
int masr_sgd_step(float* p, const float* g, float* mom, int64_t n, float lr, float momentum, int nesterov, int first_step, void* stream) {
    return mk_clip_sgd(p, g, mom, n, nullptr, 0.f, lr, momentum, nesterov, first_step, (hipStream_t)stream);
}
int masr_scale(float* x, int64_t n, float a, void* stream) { return mk_scale(x, n, a, (hipStream_t)stream); }
int masr_axpy(float* y, const float* x, int64_t n, float a, void* stream) { return mk_axpy(y, x, n, a, (hipStream_t)stream); }
int masr_copy(float* dst, const float* src, int64_t n, void* stream) {
    HIP_CHECK_RET(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// Levenshtein distance of two id sequences (host code; the reference's metric imports the `editdistance` C extension,
// src/monitor/metric.py:4,66,87).  Two-row DP, unit costs.
int64_t masr_edit_distance(const int32_t* a, int na, const int32_t* b, int nb) {
    if (na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) { mk_set_error("masr_edit_distance", "bad arguments"); return -1; }
    std::vector<int64_t> row((size_t)nb + 1);
    for (int j = 0; j <= nb; ++j) row[j] = j;
    for (int i = 1; i <= na; ++i) {
        int64_t diag = row[0];
        row[0] = i;
        for (int j = 1; j <= nb; ++j) {
            const int64_t sub = diag + (a[i - 1] != b[j - 1]);
            diag = row[j];
            int64_t v = row[j] + 1;
            if (row[j - 1] + 1 < v) v = row[j - 1] + 1;
            if (sub < v) v = sub;
            row[j] = v;
        }
    }
    return row[nb];
}

int masr_gather_pad(const float* feat, const int64_t* row_start, const int32_t* lens, float* xs, int B, int Tmax, int D, void* stream) {
    return mk_gather_pad(feat, (const long*)row_start, lens, xs, B, Tmax, D, (hipStream_t)stream);
}
int masr_fbank(const float* wav, const int64_t* wav_off, const int64_t* row_off, int B, int max_frames, int n_mel, float* feat, void* stream) {
    return mk_fbank(wav, (const long*)wav_off, (const long*)row_off, B, max_frames, n_mel, feat, (hipStream_t)stream);
}
int64_t masr_fbank_pitch_work_bytes(int64_t total_samples, int B, int max_frames) { return mk_pitch_work_bytes(total_samples, B, max_frames); }
int masr_fbank_pitch(const float* wav, const int64_t* wav_off, const int64_t* row_off, int64_t total_samples, int64_t max_samples, int B, int max_frames,
                     int n_mel, float* feat, void* work, int64_t work_bytes, void* stream) {
    if (mk_fbank(wav, (const long*)wav_off, (const long*)row_off, B, max_frames, n_mel, feat, (hipStream_t)stream, 1) != 0) return -1;
    return mk_pitch(wav, (const long*)wav_off, (const long*)row_off, total_samples, max_samples, B, max_frames, n_mel, feat, work, work_bytes, (hipStream_t)stream);
}
int64_t masr_ctc_work_floats(int T, int B, int maxS) { return mk_ctc_work_floats(T, B, maxS); }
int masr_ctc_status(const float* work, int T, int B, int maxS, void* stream) { return mk_ctc_status(work, T, B, maxS, (hipStream_t)stream); }
int masr_ctc_loss(const float* logits, const int32_t* targets, const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int T,
                  int B, int C, int blank, float* nll, float* loss, float* grad, float* work, int maxS, void* stream) {
    return mk_ctc_loss(logits, targets, tgt_off, in_len, tgt_len, T, B, C, blank, nll, loss, grad, work, maxS, (hipStream_t)stream);
}
int64_t masr_ctc_beam_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_work_bytes(B, Tp, C, K); }
int masr_ctc_beam_search(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                         void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens, float* scores, void* stream) {
    return mk_ctc_beam_search(logits, (long)ld, enc_lens, B, Tp, C, K, nbest, blank, eos, work, work_bytes, tokens, lens, scores, (hipStream_t)stream);
}
int64_t masr_ctc_beam_lm_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_lm_work_bytes(B, Tp, C, K); }
int masr_ctc_beam_search_lm(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                            const masr_lm* lm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens,
                            float* scores, float* am, void* stream) {
    return mk_ctc_beam_search_lm(logits, (long)ld, enc_lens, B, Tp, C, K, nbest, blank, eos, lm, lm_w, len_bonus, work, work_bytes, tokens, lens, scores,
                                 am, (hipStream_t)stream);
}
int64_t masr_ctc_beam_bias_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_bias_work_bytes(B, Tp, C, K); }
int masr_ctc_beam_search_bias(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                              const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work, int64_t work_bytes,
                              int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias, void* stream) {
    return mk_ctc_beam_search_bias(logits, (long)ld, enc_lens, B, Tp, C, K, nbest, blank, eos, lm, lm_w, len_bonus, bias, bias_w, work, work_bytes, tokens,
                                   lens, scores, am, nbias, (hipStream_t)stream);
}
int64_t masr_ctc_beam_run_work_bytes(int B, int Tp, int C, int K) { return mk_ctc_beam_run_work_bytes(B, Tp, C, K); }
masr_ctc_beam_run* masr_ctc_beam_run_open(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int blank, int eos,
                                          const masr_lm* lm, float lm_w, float len_bonus, const masr_bias* bias, float bias_w, void* work,
                                          int64_t work_bytes, void* stream) {
    return mk_ctc_beam_run_open("masr_ctc_beam_run_open", logits, (long)ld, enc_lens, B, Tp, C, K, blank, eos, lm, lm_w, len_bonus, bias, bias_w, work,
                                work_bytes, (hipStream_t)stream);
}
int masr_ctc_beam_run_advance(masr_ctc_beam_run* run, int t_end, void* stream) {
    return mk_ctc_beam_run_advance("masr_ctc_beam_run_advance", run, t_end, (hipStream_t)stream);
}
int masr_ctc_beam_run_result(const masr_ctc_beam_run* run, int nbest, int32_t* tokens, int32_t* lens, float* scores, float* am, int32_t* nbias,
                             void* stream) {
    return mk_ctc_beam_run_result("masr_ctc_beam_run_result", run, nbest, tokens, lens, scores, am, nbias, (hipStream_t)stream);
}
void masr_ctc_beam_run_close(masr_ctc_beam_run* run) { mk_ctc_beam_run_close(run); }
int64_t masr_ctc_beam_nlm_work_bytes(const masr_nlm* nlm, int B, int Tp, int C, int K) { return mk_ctc_beam_nlm_work_bytes(nlm, B, Tp, C, K); }
int masr_ctc_beam_search_nlm(const float* logits, int64_t ld, const int32_t* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                             const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int32_t* tokens, int32_t* lens,
                             float* scores, float* am, void* stream) {
    return mk_ctc_beam_search_nlm(logits, (long)ld, enc_lens, B, Tp, C, K, nbest, blank, eos, nlm, lm_w, len_bonus, work, work_bytes, tokens, lens, scores,
                                  am, (hipStream_t)stream);
}
int64_t masr_ctc_align_work_bytes(int B, int Tp, int maxL) { return mk_ctc_align_work_bytes(B, Tp, maxL); }
int masr_ctc_align(const float* logits, int64_t ld, const int32_t* enc_lens, const int32_t* targets, const int32_t* tgt_off, const int32_t* tgt_len,
                   int B, int Tp, int C, int blank, int maxL, void* work, int64_t work_bytes, int32_t* frames, int32_t* start, int32_t* end,
                   float* score, void* stream) {
    return mk_ctc_align(logits, (long)ld, enc_lens, targets, tgt_off, tgt_len, B, Tp, C, blank, maxL, work, work_bytes, frames, start, end, score,
                        (hipStream_t)stream);
}

int masr_profile_enable(masr_model* m, int on) {
    m->prof = on != 0;
    for (int i = 0; i < MASR_PROF_N; ++i) m->prof_used[i] = 0;
    return 0;
}
int masr_profile_read(masr_model* m, float* ms, int* launches) {
    HIP_CHECK_RET(hipDeviceSynchronize());
    for (int i = 0; i < MASR_PROF_N; ++i) {
        float tot = 0.f;
        for (int k = 0; k < m->prof_used[i]; ++k) {
            float t = 0.f;
            hipEventElapsedTime(&t, m->prof_ev[i][k].first, m->prof_ev[i][k].second);
            tot += t;
        }
        ms[i] = tot; launches[i] = m->prof_used[i]; m->prof_used[i] = 0;
    }
    return 0;
}

}  // extern "C"
