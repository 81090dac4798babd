// libmasr engine, the training step: MyTransformer.forward (src/model/transformer_pytorch/mono_transformer_torch.py:178-208) plus
// run_batch's loss / backward (src/transformer_torch_trainer.py:59-99) as a fixed sequence of kernel launches over the activation
// plan of engine.hip -- the forward and backward blocks, the backward pass, masr_run_batch and its captured step graphs.
// forward_encoder / project_memory_kv / forward_decoder also serve the decoders (recog.hip).
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace {

// weight/bias gradients of a Linear: dW[N][K] = dy^T x, db = colsum(dy).  They feed nothing but the optimiser, so they are not launched one by
// one: every layer keeps its own dY operand and ONE grid of 256 x 256 tiles (gemm.hip gemm_wgrad_grouped16_kernel) computes them all at the end
// of the backward pass -- the encoder-row members (reduction over B*T' rows: `enc`) first, the decoder-row ones (B*L rows) filling the CUs
// those leave idle.  A member that does not fit the descriptor list (very deep models) runs as a plain reduction-major GEMM at once.
int lin_wgrad(Ctx& c, const bf16* dy, long lddy, const bf16* x, long ldx, int rows, int N, int K, float* dW, float* db, bool enc = false) {
    masr_model* m = c.m;
    WgradGroup& grp = enc ? m->wge : m->wg;
    if (m->wge.n + m->wg.n < WGRAD_GROUP_MAX) {
        WgradDesc& d = grp.p[grp.n++];
        d.dy = dy; d.x = x; d.dW = dW; d.db = db; d.lddy = (int)lddy; d.ldx = (int)ldx; d.rows = rows; d.N = N; d.K = K; d.tile_start = 0;
        return 0;
    }
    GemmArgs g = gemm_args();
    g.reduction_major = 1; g.A = dy; g.lda = lddy; g.B = x; g.ldb = ldx; g.M = N; g.N = K; g.K = rows;
    g.C32 = dW; g.ldc = K; g.colsum = db;
    return gemm(c, g);
}
// hkust: 148 tiles over 4000 rows + 228 over 592 rows.  As two launches the first leaves 108 CUs idle for ~110 us and the second takes ~40 us
// of its own; as one the short tiles run on those CUs (125 us).  masr_set_split_wgrad_launches: two launches (A/B; same bits -- every element
// of dW is reduced by one workgroup over its rows in order either way: tests/test_hip_engine.py).
int flush_wgrads(Ctx& c) {
    masr_model* m = c.m;
    int rc = 0;
    if (!m->split_wgrad) {
        const int first = m->wge.n;                                        // the encoder-row members go first (long reductions)
        for (int i = 0; i < m->wg.n; ++i) m->wge.p[m->wge.n++] = m->wg.p[i];
        m->wg.n = 0;
        if (m->wge.n) { Prof p(m, MASR_PROF_WGRAD_ENC, c.s); rc = mk_gemm_wgrad_grouped(m->wge, c.s, first); }
    } else {
        if (m->wge.n) { Prof p(m, MASR_PROF_WGRAD_ENC, c.s); rc = mk_gemm_wgrad_grouped(m->wge, c.s); }
        if (rc == 0 && m->wg.n) { Prof p(m, MASR_PROF_WGRAD_DEC, c.s); rc = mk_gemm_wgrad_grouped(m->wg, c.s); }
    }
    m->wge.n = 0; m->wg.n = 0;
    return rc;
}
// dX = dy W via the transposed shadow t16 [K][ldt]
GemmArgs lin_dgrad_args(const bf16* dy, long lddy, const bf16* t16, long ldt, int rows, int N, int K) {
    GemmArgs g = gemm_args();
    g.A = dy; g.lda = lddy; g.B = t16; g.ldb = ldt; g.M = rows; g.N = K; g.K = N;
    return g;
}

// The few-row GEMMs with a long reduction (decoder rows: FFN second layer and the first layer's dgrad, K = d_inner; packed q/k/v dgrad, K = 3E) are
// 80 workgroups with a chain of 24-32 k steps each -- 16 us where their K = 512 siblings take 8.  They run k-split over K / 512 x as many
// workgroups; each writes its fp32 partial product and the LayerNorm that always follows sums them (and applies what the GEMM's epilogue would
// have: bias, dropout, residual) on its way in: no combine pass, no extra launch (rowops.hip LnSumArgs).  0: not this shape.
// It buys latency with occupancy -- 320 workgroups x 7.4 us instead of 80 x 16 -- so it pays with the GPU to the task alone (train.py: +3 %) and costs
// beside other task slots, where occupancy counts (four-slot throughput 9 920 -> 10 000 utt/s with whole reductions).  It changes the fp32 summation
// order, so it follows ONLY masr_set_ksplit (default off), never the slot count: the caller that runs one task per GPU turns it on (mono / multi
// interface), the FOMAML interface leaves it off for every --tasks_per_gpu (K slots == the sequential run == N ranks, bit for bit).
static int ksplit_of(const masr_model* m, int rows, int K) { return (m->ksplit && rows <= 1024 && K >= 1024 && K % 512 == 0 && K / 512 <= KSPLIT_MAX) ? K / 512 : 0; }
// The GEMM in front of a LayerNorm: whole (sum.n == 0), or k-split sum.n ways into Acts::part with `sum` -- what the epilogue would have
// applied -- handed through `defer` to that LayerNorm (ln_fwd / ln_bwd), which adds the partial products up on its way in
static int gemm_or_ksplit(Ctx& c, GemmArgs g, LnSumArgs* defer, const LnSumArgs& sum) {
    if (!sum.n) {
        if (defer) defer->n = 0;
        return gemm(c, g);
    }
    *defer = sum;
    ++c.m->n_ksplit;
    g.bias = nullptr; g.drop_p = 0.f; g.residual = nullptr; g.C16 = nullptr;
    g.C32 = c.m->acts.part; g.ldc = g.N; g.split_k = sum.n; g.split_stride = sum.stride;
    return gemm(c, g);
}

// nb: the attention's batches, rows_q = nb * Tq query rows
int attn_block_fwd(Ctx& c, const Attn& at, const bf16* xq, int rows_q, int nb, int Tq, int Tk, bool self, bool causal, const int* klens,
                   bf16* qkv_or_q, bf16* kv, bf16* ao, float* lse, const float* resid, float* s_out, uint32_t site_p, uint32_t site_o,
                   LnSumArgs* defer = nullptr, bool chunk = false) {
    masr_model* m = c.m; const int E = m->E; const float* P = m->P;
    AttnArgs a{};
    if (chunk) { a.chunk = c.chunk; a.left = c.left; a.chunk_ptr = c.chunk_ptr; }      // the encoder's self-attention under masr_set_chunk
    if (self) {
        GemmArgs g = lin_fwd_args(xq, E, at.in.k16, rows_q, 3 * E, E, P + at.in.b); g.C16 = qkv_or_q; g.ldc16 = 3 * E;
        CK(gemm(c, g));
        a.q = qkv_or_q; a.k = qkv_or_q + E; a.v = qkv_or_q + 2 * E; a.ldq = a.ldk = a.ldv = 3 * E;
    } else {
        GemmArgs g = lin_fwd_args(xq, E, at.q_k16, rows_q, E, E, P + at.in.b); g.C16 = qkv_or_q; g.ldc16 = E;
        CK(gemm(c, g));
        // K|V of the encoder memory were projected for all layers at once (project_memory_kv); kv = this layer's columns
        a.q = qkv_or_q; a.ldq = E; a.k = kv; a.v = kv + E; a.ldk = a.ldv = m->NK;
    }
    a.o = ao; a.ldo = E; a.lse = lse; a.klens = klens; a.B = nb; a.H = m->H; a.Tq = Tq; a.Tk = Tk; a.hd = m->hd;
    a.causal = causal; a.drop_p = c.p_drop; a.seed = c.seed; a.seed_ptr = c.seed_ptr; a.site = site_p;
    { Prof p(m, Tk == m->acts.Tp && Tq == Tk ? MASR_PROF_ATTN_ENC : MASR_PROF_ATTN_DEC, c.s); CK(mk_attn_fwd(a, c.s)); }
    GemmArgs o = lin_fwd_args(ao, E, at.out.k16, rows_q, E, E, P + at.out.b);
    o.drop_p = c.p_drop; o.seed = c.seed; o.site = site_o; o.residual = resid; o.ldres = E; o.C32 = s_out; o.ldc = E;
    // few rows: the reduction over E runs as two halves on twice the workgroups, the LayerNorm behind the block sums them (see ksplit_of):
    // out-projection 8.6 -> 5.9 us, the LayerNorm 4.8 -> 5.6 with the second partial to read
    const int S = (defer && m->ksplit && rows_q <= 1024 && E >= 512 && E % 128 == 0) ? 2 : 0;
    return gemm_or_ksplit(c, o, defer, LnSumArgs{m->acts.part, (long)rows_q * E, S, P + at.out.b, resid, c.p_drop, c.seed, site_o, c.seed_ptr, s_out});
}

int ffn_fwd(Ctx& c, const Lin& l1, const Lin& l2, const bf16* x16, const float* x32, int rows, bf16* f, float* s_out, uint32_t site_i, uint32_t site_o,
            LnSumArgs* defer = nullptr) {
    masr_model* m = c.m; const int E = m->E, Fi = m->Fi; const float* P = m->P;
    GemmArgs g = lin_fwd_args(x16, E, l1.k16, rows, Fi, E, P + l1.b); g.relu = 1; g.drop_p = c.p_drop; g.seed = c.seed; g.site = site_i;
    g.C16 = f; g.ldc16 = Fi;
    CK(gemm(c, g));
    GemmArgs h = lin_fwd_args(f, Fi, l2.k16, rows, E, Fi, P + l2.b); h.drop_p = c.p_drop; h.seed = c.seed; h.site = site_o;
    h.residual = x32; h.ldres = E; h.C32 = s_out; h.ldc = E;
    const int S = defer ? ksplit_of(m, rows, Fi) : 0;
    return gemm_or_ksplit(c, h, defer, LnSumArgs{m->acts.part, (long)rows * E, S, P + l2.b, x32, c.p_drop, c.seed, site_o, c.seed_ptr, s_out});
}

int ln_bwd(Ctx& c, const Norm& n, const float* dy, const float* x, const float* mean, const float* rstd, float* dx32, bf16* dx16,
           uint32_t site, int rows, const LnSumArgs* sum = nullptr) {
    masr_model* m = c.m;
    // the dgamma/dbeta partials of every LayerNorm go to their own slab region; the fold launch at the end of the pass folds them all at once
    // (the summing kernel writes ceil(rows / 4) blocks, the plain one mk_layernorm_bwd_blocks(rows) = ceil(rows / 4 ln_rows_per_wave(rows)), and
    // rowops.hip's ln_rows_per_wave is 1 below 2048 rows: one count for both, since a k-split GEMM has at most 1024 rows -- ksplit_of)
    const int nblocks = mk_layernorm_bwd_blocks(rows);
    const int64_t need = (int64_t)nblocks * 2 * m->E;
    const bool summing = sum && sum->n > 0;                    // dy = the partial products of a k-split dgrad GEMM + its residual gradient
    float* slab = nullptr;
    if (m->lng.n < LN_GROUP_MAX && m->ln_slab_used + need <= m->acts.ln_slab_floats) {
        slab = m->acts.ln_slab + m->ln_slab_used;
        m->ln_slab_used += need;
        m->lng.p[m->lng.n++] = LnReduceDesc{slab, m->G + n.w, m->G + n.b, nblocks};
    } else if (summing) { mk_set_error("ln_bwd", "no room for the LayerNorm partials"); return -1; }
    const float p_drop = dx16 ? c.p_drop : 0.f;
    Prof p(c.m, MASR_PROF_LAYERNORM, c.s);
    if (summing) return mk_layernorm_bwd_sum(*sum, x, m->P + n.w, mean, rstd, dx32, dx16, p_drop, c.seed, site, slab, rows, m->E, c.s, c.seed_ptr);
    if (slab) return mk_layernorm_bwd(dy, x, m->P + n.w, mean, rstd, dx32, dx16, p_drop, c.seed, site, nullptr, nullptr, slab, rows, m->E, c.s, c.seed_ptr);
    // no room in the grouped reduce (very deep models): this LayerNorm folds its own partials at once
    return mk_layernorm_bwd(dy, x, m->P + n.w, mean, rstd, dx32, dx16, p_drop, c.seed, site, m->G + n.w, m->G + n.b, m->acts.slab, rows, m->E, c.s,
                            c.seed_ptr);
}

// backward of  s_out = x + drop(ffn(x16))  given d s_out (gs32 fp32, gs16 bf16 already dropout-masked for the ffn output site)
// writes d x (fp32) = gs32 + ffn-branch gradient into gout
int ffn_bwd(Ctx& c, const Lin& l1, const Lin& l2, const bf16* x16, const bf16* f, const float* gs32, const bf16* gs16, int rows,
            bf16* gf, float* gout, bool split, LnSumArgs* defer = nullptr) {
    masr_model* m = c.m; const int E = m->E, Fi = m->Fi;
    CK(lin_wgrad(c, gs16, E, f, Fi, rows, E, Fi, m->G + l2.w, m->G + l2.b, split));
    GemmArgs g = lin_dgrad_args(gs16, E, l2.t16, E, rows, E, Fi);
    g.mask = f; g.ldmask = Fi; g.mask_scale = c.p_drop > 0.f ? 1.f / (1.f - c.p_drop) : 1.f; g.C16 = gf; g.ldc16 = Fi;
    CK(gemm(c, g));
    CK(lin_wgrad(c, gf, Fi, x16, E, rows, Fi, E, m->G + l1.w, m->G + l1.b, split));
    GemmArgs h = lin_dgrad_args(gf, Fi, l1.t16, Fi, rows, Fi, E);
    h.residual = gs32; h.ldres = E; h.C32 = gout; h.ldc = E;
    const int S = defer ? ksplit_of(m, rows, Fi) : 0;              // (k-split: gout is not written, the LayerNorm backward that follows takes `defer`)
    return gemm_or_ksplit(c, h, defer, LnSumArgs{m->acts.part, (long)rows * E, S, nullptr, gs32, 0.f, 0u, 0u, nullptr, nullptr});
}

}  // namespace

int forward_encoder(Ctx& c, const float* xs) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s; const float* P = m->P;
    const int B = a.B, T = a.T, D = a.D, E = m->E;
    // every pass that does not train (MASR_EVAL, the decoders) runs under the policy's own chunk; a training pass brings the step's along
    if (!c.train) { c.chunk = m->chunk.size; c.left = m->chunk.left; c.chunk_ptr = nullptr; m->chunk_last = c.chunk; }
    uint32_t site = 1;
    {
        Prof p(m, MASR_PROF_CONV1_FWD, s);
        CK(mk_conv1_fwd(xs, P + m->conv[0].w, P + m->conv[0].b, a.a1, B, T, D, s, c.train ? a.a1_bits : nullptr));
    }
    // the maps in front of the two pools are needed by nothing but the pool + ReLU backward, and that needs one byte per POOLED
    // element (which window position won, or that none passed the ReLU): the pooling convs store those and drop the map
    auto conv = [&](const bf16* in, const Conv& cv, bf16* out, int H, int W, bf16* pooled, uint8_t* idx) -> int {
        Prof p(m, MASR_PROF_CONV2_FWD + (int)(&cv - &m->conv[1]), s);
        ConvArgs ca{}; ca.sched = m->conv_sched; ca.in = in; ca.wk = cv.k16; ca.bias = P + cv.b; ca.relu = 1; ca.mask = nullptr; ca.out = out; ca.shared = c.train ? m->slots : 0;
        ca.B = B; ca.H = H; ca.W = W; ca.CIN = cv.CI; ca.COUT = cv.CO; ca.pool_out = pooled;      // MaxPool2d written by the producing conv's epilogue
        if (ca.pool_out) { ca.pool_idx = c.train ? idx : nullptr; ca.out_optional = 1; }
        if (&cv == &m->conv[2] && c.train) ca.out_sign_bits = a.a3_bits;      // conv3's ReLU mask as sign bits for conv4's masked dgrad
        return mk_conv3x3(ca, s);
    };
    CK(conv(a.a1, m->conv[1], nullptr, T, D, a.p1, a.i1));
    CK(conv(a.p1, m->conv[2], a.a3, a.H2, a.W2, nullptr, nullptr));
    CK(conv(a.a3, m->conv[3], nullptr, a.H2, a.W2, a.p2, a.i2));
    // vgg2enc + positional encoding + pos dropout
    {
        GemmArgs g = lin_fwd_args(a.p2, m->F, m->v2e_k, a.rows_e, E, m->F, P + m->v2e.b);
        g.pe = m->pe; g.pe_period = a.Tp; g.drop_p = c.p_pos; g.seed = c.seed; g.site = a.site_v2e = site++;
        g.C32 = a.x32[0]; g.ldc = E; g.C16 = a.x16[0]; g.ldc16 = E;
        CK(gemm(c, g));
    }
    for (int l = 0; l < m->NE; ++l) {
        EncAct& e = a.enc[l]; const EncL& w = m->enc[l];
        for (int i = 0; i < 4; ++i) e.site[i] = site++;
        CK(attn_block_fwd(c, w.sa, a.x16[l], a.rows_e, a.B, a.Tp, a.Tp, true, false, a.enc_lens, e.qkv, nullptr, e.ao, e.lse, a.x32[l], e.s1,
                          e.site[0], e.site[1], nullptr, true));
        CK(ln_fwd(c, w.n1, e.s1, e.x1_32, e.x1_16, e.m1, e.r1, a.rows_e));
        CK(ffn_fwd(c, w.l1, w.l2, e.x1_16, e.x1_32, a.rows_e, e.f, e.s2, e.site[2], e.site[3]));
        CK(ln_fwd(c, w.n2, e.s2, a.x32[l + 1], a.x16[l + 1], e.m2, e.r2, a.rows_e));
    }
    CK(ln_fwd(c, m->enc_norm, a.x32[m->NE], nullptr, a.mem16, a.mf, a.rf, a.rows_e));
    return 0;
}

// K|V projections of the encoder memory for the cross-attention of EVERY decoder layer: one GEMM, N = ND*2E
int project_memory_kv(Ctx& c) {
    masr_model* m = c.m; Acts& a = m->acts;
    GemmArgs h = lin_fwd_args(a.mem16, m->E, m->kv_k16, a.rows_e, m->NK, m->E, m->kv_bias);
    h.C16 = a.kv_all; h.ldc16 = m->NK;
    return gemm(c, h);
}

// gm (null: the plan's a.B sequences of a.L positions, today's launches exactly): gm->seqs sequences of gm->L positions in the plan's buffers,
// gm->seqs a multiple of a.B with the sequences of one utterance next to each other.  The embedding and the causal self-attention run per
// sequence; the cross-attention runs per utterance, its seqs / a.B * L query rows (contiguous) against that utterance's memory.
int forward_decoder(Ctx& c, bool project_kv, bool logits_f32, const DecoderGeom* gm) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s; const float* P = m->P;
    const int E = m->E, L = gm ? gm->L : a.L, seqs = gm ? gm->seqs : a.B, rows_d = gm ? gm->seqs * gm->L : a.rows_d;
    const int Tq_cross = rows_d / a.B;
    uint32_t site = 100;
    a.site_emb = site++;
    if (project_kv) CK(project_memory_kv(c));
    { Prof p(m, MASR_PROF_MISC, s); CK(mk_embed_fwd(a.tok_in, P + m->embed_w, m->pe, a.y32[0], a.y16[0], seqs, L, E, c.p_pos, c.seed, a.site_emb, s, c.seed_ptr)); }
    for (int l = 0; l < m->ND; ++l) {
        DecAct& d = a.dec[l]; const DecL& w = m->dec[l];
        for (int i = 0; i < 6; ++i) d.site[i] = site++;
        LnSumArgs ks{};                                        // (k-split GEMMs: their partial products are summed by the LayerNorm behind them)
        CK(attn_block_fwd(c, w.sa, a.y16[l], rows_d, seqs, L, L, true, true, nullptr, d.qkv, nullptr, d.ao, d.lse_s, a.y32[l], d.s1, d.site[0],
                          d.site[1], &ks));
        CK(ln_fwd(c, w.n1, d.s1, d.y1_32, d.y1_16, d.m1, d.r1, rows_d, &ks));
        CK(attn_block_fwd(c, w.ca, d.y1_16, rows_d, a.B, Tq_cross, a.Tp, false, false, a.enc_lens, d.q, d.kv, d.co, d.lse_c, d.y1_32, d.s2, d.site[2],
                          d.site[3], &ks));
        CK(ln_fwd(c, w.n2, d.s2, d.y2_32, d.y2_16, d.m2, d.r2, rows_d, &ks));
        CK(ffn_fwd(c, w.l1, w.l2, d.y2_16, d.y2_32, rows_d, d.f, d.s3, d.site[4], d.site[5], &ks));
        CK(ln_fwd(c, w.n3, d.s3, a.y32[l + 1], a.y16[l + 1], d.m3, d.r3, rows_d, &ks));
    }
    if (logits_f32) {
        // greedy decode: the last projection in fp32 on the master weights (see mk_logits_f32); layer 0's pre-LayerNorm sum is free by now
        float* yf32 = a.dec[0].s1;
        CK(ln_fwd(c, m->dec_norm, a.y32[m->ND], yf32, nullptr, a.mdf, a.rdf, rows_d));
        return mk_logits_f32(yf32, P + m->ct.w, P + m->ct.b, a.logits, m->Cp, rows_d, m->C, E, c.s);
    }
    CK(ln_fwd(c, m->dec_norm, a.y32[m->ND], nullptr, a.yf16, a.mdf, a.rdf, rows_d));
    GemmArgs g = lin_fwd_args(a.yf16, E, m->ct.k16, rows_d, m->C, E, P + m->ct.b);
    g.C32 = a.logits; g.ldc = m->Cp;
    CK(gemm(c, g));
    return 0;
}

// backward of an attention block  s = resid + drop(out_proj(attn(...)))
//   gs32/gs16: d s (bf16 copy already masked with the out-proj dropout site)
//   self : writes d x (fp32) = gs32 + qkv-proj dgrad into gout
//   cross: writes d xq (fp32) = gs32 + q-proj dgrad into gout and d K|V into gkv, this layer's columns of gkv_all (memory_kv_bwd takes them on)
static int attn_block_bwd(Ctx& c, const Attn& at, const bf16* xq16, int rows_q, int Tq, int Tk, bool self, bool causal, const int* klens,
                          const bf16* qkv_or_q, const bf16* kv, const bf16* ao, const float* lse, const float* gs32, const bf16* gs16, bf16* gao,
                          bf16* gqkv_or_q, bf16* gkv, float* delta, float* gout, uint32_t site_p, bool split, LnSumArgs* defer = nullptr,
                          bool chunk = false) {
    masr_model* m = c.m; const int E = m->E; float* G = m->G;
    CK(lin_wgrad(c, gs16, E, ao, E, rows_q, E, E, G + at.out.w, G + at.out.b, split));
    { GemmArgs g = lin_dgrad_args(gs16, E, at.out.t16, E, rows_q, E, E); g.C16 = gao; g.ldc16 = E; CK(gemm(c, g)); }
    AttnArgs a{};
    if (self) {
        a.q = qkv_or_q; a.k = qkv_or_q + E; a.v = qkv_or_q + 2 * E; a.ldq = a.ldk = a.ldv = 3 * E;
        a.dq = gqkv_or_q; a.dk = gqkv_or_q + E; a.dv = gqkv_or_q + 2 * E; a.lddq = a.lddk = a.lddv = 3 * E;
    } else {
        a.q = qkv_or_q; a.ldq = E; a.k = kv; a.v = kv + E; a.ldk = a.ldv = m->NK;
        a.dq = gqkv_or_q; a.lddq = E; a.dk = gkv; a.dv = gkv + E; a.lddk = a.lddv = m->NK;     // this layer's columns of gkv_all
    }
    a.o = const_cast<bf16*>(ao); a.ldo = E; a.lse = const_cast<float*>(lse); a.dout = gao; a.lddo = E; a.delta = delta; a.klens = klens;
    a.B = m->acts.B; a.H = m->H; a.Tq = Tq; a.Tk = Tk; a.hd = m->hd; a.causal = causal; a.drop_p = c.p_drop; a.seed = c.seed; a.seed_ptr = c.seed_ptr; a.site = site_p;
    if (chunk) { a.chunk = c.chunk; a.left = c.left; a.chunk_ptr = c.chunk_ptr; }      // the mask of the forward (attn_block_fwd)
    { Prof p(m, Tk == m->acts.Tp && Tq == Tk ? MASR_PROF_ATTN_ENC : MASR_PROF_ATTN_DEC, c.s); CK(mk_attn_bwd(a, c.s)); }
    if (self) {
        CK(lin_wgrad(c, gqkv_or_q, 3 * E, xq16, E, rows_q, 3 * E, E, G + at.in.w, G + at.in.b, split));
        GemmArgs g = lin_dgrad_args(gqkv_or_q, 3 * E, at.in.t16, 3 * E, rows_q, 3 * E, E);
        g.residual = gs32; g.ldres = E; g.C32 = gout; g.ldc = E;
        const int S = defer ? ksplit_of(m, rows_q, 3 * E) : 0;     // (k-split: gout is not written, the next LayerNorm backward takes `defer`)
        return gemm_or_ksplit(c, g, defer, LnSumArgs{m->acts.part, (long)rows_q * E, S, nullptr, gs32, 0.f, 0u, 0u, nullptr, nullptr});
    }
    CK(lin_wgrad(c, gqkv_or_q, E, xq16, E, rows_q, E, E, G + at.in.w, G + at.in.b));
    GemmArgs g = lin_dgrad_args(gqkv_or_q, E, at.q_t16, E, rows_q, E, E);
    g.residual = gs32; g.ldres = E; g.C32 = gout; g.ldc = E;
    // the K|V halves (weight gradients, gradient of the encoder memory) are handled for all layers at once by
    // memory_kv_bwd after the decoder layer loop
    return gemm(c, g);
}

// backward of project_memory_kv for all decoder layers at once: the ND weight gradients dW_l = gkv_l^T mem are ONE
// reduction-major GEMM with M = ND*2E whose output rows are segmented over the layers' in_proj_weight blocks (constant
// distance in the flat gradient buffer), and d(memory) = sum_l gkv_l Wkv_l is ONE GEMM with K = ND*2E
static int memory_kv_bwd(Ctx& c) {
    masr_model* m = c.m; Acts& a = m->acts; float* G = m->G;
    const int E = m->E;
    const DecL& d0 = m->dec[0];
    if (m->wge.n + m->wg.n + m->ND <= WGRAD_GROUP_MAX) {
        // one descriptor per decoder layer in the grouped encoder-row launch (gkv_all stays untouched until the end of the pass)
        for (int l = 0; l < m->ND; ++l)
            CK(lin_wgrad(c, a.gkv_all + (int64_t)l * 2 * E, m->NK, a.mem16, E, a.rows_e, 2 * E, E, G + m->dec[l].ca.in.w + (long)E * E, G + m->dec[l].ca.in.b + E, true));
    } else {
        GemmArgs g = gemm_args();
        g.reduction_major = 1; g.A = a.gkv_all; g.lda = m->NK; g.B = a.mem16; g.ldb = E; g.M = m->NK; g.N = E; g.K = a.rows_e;
        g.C32 = G + d0.ca.in.w + (long)E * E; g.ldc = E; g.colsum = G + d0.ca.in.b + E;
        g.cseg_rows = 2 * E; g.cseg_stride = m->ND > 1 ? m->dec[1].ca.in.w - d0.ca.in.w : 0;
        CK(gemm(c, g));
    }
    GemmArgs h = lin_dgrad_args(a.gkv_all, m->NK, m->kvT, m->NK, a.rows_e, m->NK, E);
    h.C32 = a.dmem32; h.ldc = E;
    CK(gemm(c, h));
    return 0;
}

// the CTC head of the joint objective (masr_create_ctc): fp32 logits of the encoder memory's bf16 operand, the lattice over them with the
// targets read from `gold`, and stats[0] = (1 - w) CE + w CTC.  Training: w * d CTC / d logits as the bf16 operand of ctc_backward
static int ctc_forward(Ctx& c) {
    masr_model* m = c.m; Acts& a = m->acts;
    GemmArgs g = lin_fwd_args(a.mem16, m->E, m->ctc.k16, a.rows_e, m->C, m->E, m->P + m->ctc.b);
    g.C32 = a.ctc_logits; g.ldc = m->Cp;
    CK(gemm(c, g));
    Prof p(m, MASR_PROF_MISC, c.s);
    return mk_ctc_loss_joint(a.ctc_logits, m->Cp, a.gold, a.ctc_tgt, a.enc_lens, a.ctc_tgt + a.B, a.Tp, a.B, m->C, a.ctc_nll,
                             c.train ? a.ctc_d16 : nullptr, m->ctc_w, m->stats, a.ctc_work, a.ctc_maxS, c.s);
}
// its backward: weight / bias gradients join the grouped encoder-row launch, d(memory) is added into dmem32 (behind memory_kv_bwd)
static int ctc_backward(Ctx& c) {
    masr_model* m = c.m; Acts& a = m->acts;
    CK(lin_wgrad(c, a.ctc_d16, m->Cp, a.mem16, m->E, a.rows_e, m->C, m->E, m->G + m->ctc.w, m->G + m->ctc.b, true));
    GemmArgs g = lin_dgrad_args(a.ctc_d16, m->Cp, m->ctc.t16, m->Cp, a.rows_e, m->Cp, m->E);
    g.C32 = a.dmem32; g.ldc = m->E; g.accumulate = 1;
    return gemm(c, g);
}

static int backward(Ctx& c, const float* xs) {
    masr_model* m = c.m; Acts& a = m->acts; hipStream_t s = c.s; float* G = m->G;
    const int E = m->E, L = a.L, B = a.B;
    // ---- output projection.  The weight gradients of the decoder-row Linears (reduction over only B*L rows) are not
    // launched one by one: their operands are kept per layer and ONE grouped launch computes them after the layer loop
    m->wg.n = 0; m->wge.n = 0;
    m->lng.n = 0; m->ln_slab_used = 0;
    CK(lin_wgrad(c, a.dlogits, m->Cp, a.yf16, E, a.rows_d, m->C, E, G + m->ct.w, G + m->ct.b));
    { GemmArgs g = lin_dgrad_args(a.dlogits, m->Cp, m->ct.t16, m->Cp, a.rows_d, m->Cp, E); g.C32 = a.gd_a; g.ldc = E; CK(gemm(c, g)); }
    float *gcur = a.gd_b, *gs = a.gd_a;
    CK(ln_bwd(c, m->dec_norm, a.gd_a, a.y32[m->ND], a.mdf, a.rdf, gcur, nullptr, 0, a.rows_d));
    // ---- decoder layers
    LnSumArgs ks{};                                            // pending partial products of a k-split dgrad (the LayerNorm backward behind it sums them)
    for (int l = m->ND - 1; l >= 0; --l) {
        DecAct& d = a.dec[l]; const DecL& w = m->dec[l]; const DecGrad& dg = a.dgr[l];
        CK(ln_bwd(c, w.n3, gcur, d.s3, d.m3, d.r3, gs, dg.g3, d.site[5], a.rows_d, &ks));
        CK(ffn_bwd(c, w.l1, w.l2, d.y2_16, d.f, gs, dg.g3, a.rows_d, dg.gf, gcur, false, &ks));
        CK(ln_bwd(c, w.n2, gcur, d.s2, d.m2, d.r2, gs, dg.g2, d.site[3], a.rows_d, &ks));
        ks.n = 0;
        CK(attn_block_bwd(c, w.ca, d.y1_16, a.rows_d, L, a.Tp, false, false, a.enc_lens, d.q, d.kv, d.co, d.lse_c, gs, dg.g2, a.gao_d, dg.gq,
                          a.gkv_all + (int64_t)l * 2 * E, a.delta_d, gcur, d.site[2], false));
        CK(ln_bwd(c, w.n1, gcur, d.s1, d.m1, d.r1, gs, dg.g1, d.site[1], a.rows_d));
        // (layer 0's input gradient goes to the embedding backward, not to a LayerNorm: its q/k/v dgrad runs whole)
        CK(attn_block_bwd(c, w.sa, a.y16[l], a.rows_d, L, L, true, true, nullptr, d.qkv, nullptr, d.ao, d.lse_s, gs, dg.g1, a.gao_d, dg.gqkv,
                          nullptr, a.delta_d, gcur, d.site[0], false, l > 0 ? &ks : nullptr));
    }
    CK(memory_kv_bwd(c));
    if (m->ctc_w > 0.f) CK(ctc_backward(c));
    float* g_dec_in = gcur;                                  // d(decoder input): consumed by embed_bwd after the split-K combine
    // ---- encoder
    gcur = a.ge_b; gs = a.ge_a;
    CK(ln_bwd(c, m->enc_norm, a.dmem32, a.x32[m->NE], a.mf, a.rf, gcur, nullptr, 0, a.rows_e));
    for (int l = m->NE - 1; l >= 0; --l) {
        EncAct& e = a.enc[l]; const EncL& w = m->enc[l];
        // (grouped weight gradients read their dY operands at the END of the pass: every layer keeps its own)
        const EncGrad eg = a.egr[l];
        CK(ln_bwd(c, w.n2, gcur, e.s2, e.m2, e.r2, gs, eg.g2, e.site[3], a.rows_e));
        CK(ffn_bwd(c, w.l1, w.l2, e.x1_16, e.f, gs, eg.g2, a.rows_e, eg.gf, gcur, true));
        CK(ln_bwd(c, w.n1, gcur, e.s1, e.m1, e.r1, gs, eg.g1, e.site[1], a.rows_e));
        CK(attn_block_bwd(c, w.sa, a.x16[l], a.rows_e, a.Tp, a.Tp, true, false, a.enc_lens, e.qkv, nullptr, e.ao, e.lse, gs, eg.g1, a.gao_e,
                          eg.gqkv, nullptr, a.delta_e, gcur, e.site[0], true, nullptr, true));
    }
    // ---- vgg2enc (through the positional dropout)
    { Prof p(m, MASR_PROF_MISC, s); CK(mk_cast_dropout(gcur, a.ge16, (long)a.rows_e * E, c.p_pos, c.seed, a.site_v2e, s, c.seed_ptr)); }
    CK(lin_wgrad(c, a.ge16, E, a.p2, m->F, a.rows_e, E, m->F, a.v2e_g32, G + m->v2e.b, true));
    CK(flush_wgrads(c));                                     // every Linear weight gradient of the step, one grid
    { GemmArgs g = lin_dgrad_args(a.ge16, E, m->v2e.t16, E, a.rows_e, E, m->F); g.C16 = a.dp2; g.ldc16 = m->F; CK(gemm(c, g)); }
    // ---- VGG
    FoldJobs folds{};
    // The two maps behind a max-pool, d(a4) and d(a2), are never materialised: their consumers -- the weight-gradient kernels and the
    // dgrad kernels -- take the POOLED gradient + the one-byte pool codes of the forward launch and expand the 2 x 2 windows while staging
    // (a quarter of the gradient bytes; the maxpool backward launches and their 338 MB per step are gone)
    auto wgrad = [&](const bf16* in, const bf16* dy, const Conv& cv, int H, int W, const bf16* dy_pooled = nullptr, const uint8_t* idx = nullptr) -> int {
        const int k = (int)(&cv - &m->conv[1]);
        ConvWgradArgs wa{}; wa.in = in; wa.dy = dy; wa.dw = G + cv.w; wa.db = G + cv.b; wa.slab = a.cw_slab[k]; wa.B = B; wa.H = H; wa.W = W; wa.CIN = cv.CI; wa.COUT = cv.CO;
        wa.dy_pooled = dy_pooled; wa.pool_idx = idx; wa.shared = m->slots;
        { Prof p(m, MASR_PROF_CONV2_WGRAD + k, s); CK(mk_conv3x3_wgrad(wa, s, 1)); }     // the partial slabs; their reduce rides in the fold launch below
        folds.conv[folds.nconv++] = {a.cw_slab[k], mk_conv3x3_wgrad_nsplit(wa), G + cv.w, G + cv.b, cv.CI, cv.CO};
        return 0;
    };
    auto dgrad = [&](const bf16* dy, const Conv& cv, bf16* out, int H, int W, const bf16* dy_pooled = nullptr, const uint8_t* idx = nullptr) -> int {
        Prof p(m, MASR_PROF_CONV2_DGRAD + (int)(&cv - &m->conv[1]), s);
        ConvArgs ca{}; ca.sched = m->conv_sched; ca.in = dy; ca.in_pooled = dy_pooled; ca.in_idx = idx; ca.wk = cv.d16; ca.out = out; ca.B = B; ca.H = H; ca.W = W;
        ca.CIN = cv.CO; ca.COUT = cv.CI; ca.shared = m->slots;       // (also the fused conv1 weight gradient's w1_slab launch)
        if (&cv == &m->conv[3]) { ca.mask = a.a3; ca.mask_bits = a.a3_bits; }      // conv3's ReLU mask: the sign words its forward launch wrote
        if (&cv == &m->conv[1]) {
            // d(conv1 output) is consumed only by conv1's weight gradient: contracted inside the dgrad epilogue, never stored
            ca.mask = a.a1; ca.mask_bits = a.a1_bits; ca.out = nullptr; ca.x1 = xs; ca.w1_slab = a.c1_slab;
        }
        return mk_conv3x3(ca, s);
    };
    CK(wgrad(a.a3, nullptr, m->conv[3], a.H2, a.W2, a.dp2, a.i2));
    CK(dgrad(nullptr, m->conv[3], a.da3, a.H2, a.W2, a.dp2, a.i2));
    CK(wgrad(a.p1, a.da3, m->conv[2], a.H2, a.W2));
    CK(dgrad(a.da3, m->conv[2], a.dp1, a.H2, a.W2));
    CK(wgrad(a.a1, nullptr, m->conv[1], a.T, a.D, a.dp1, a.i1));
    CK(dgrad(nullptr, m->conv[1], nullptr, a.T, a.D, a.dp1, a.i1));
    // ---- every fold of the pass as ONE launch (fold.hip): the conv / conv1 slab reduces, the LayerNorm dgamma / dbeta partials, vgg2enc's weight
    // gradient back in the reference's feature order, and the embedding rows added into the (tied) table -- after the grouped launch wrote it
    folds.E = E;
    folds.conv1 = {a.c1_slab, mk_conv1_wgrad_fused_rows(B, a.T, a.D), G + m->conv[0].w, G + m->conv[0].b};
    folds.unperm = {a.v2e_g32, G + m->v2e.w, E, 128, m->Dp};
    folds.embed = {a.tok_order, a.tok_start, g_dec_in, G + m->embed_w, m->C, E, m->cfg.tie_weights ? 1 : 0, c.p_pos, c.seed, a.site_emb, c.seed_ptr};
    folds.ln = m->lng;
    { Prof p(m, MASR_PROF_CONV1_WGRAD, s); CK(mk_backward_folds(folds, s)); }
    m->lng.n = 0; m->ln_slab_used = 0;
    return 0;
}

// (described in host_util.h: test_abi.hip stages masr_test_embed_bwd's tokens with it)
void group_positions_by_token(const int* tok, int B, int L, const int64_t* olens, int V, int* order, int* start) {
    auto cnt = [&](int b) { return olens ? (int)olens[b] + 1 : L; };
    for (int v = 0; v <= V; ++v) start[v] = 0;
    for (int b = 0; b < B; ++b) for (int l = 0; l < cnt(b); ++l) start[tok[b * L + l] + 1]++;
    for (int v = 0; v < V; ++v) start[v + 1] += start[v];
    // (fill with a running cursor kept in the start array itself, then shift it back)
    for (int b = 0; b < B; ++b) for (int l = 0; l < cnt(b); ++l) order[start[tok[b * L + l]]++] = b * L + l;
    for (int v = V; v > 0; --v) start[v] = start[v - 1];
    start[0] = 0;
}

extern "C" int masr_run_batch(masr_model* m, const float* xs, const int64_t* ilens, const int64_t* ys_flat, const int64_t* olens, int B, int T,
                   int flags, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!m->P) { mk_set_error("masr_run_batch", "not bound"); return -1; }
    if (B <= 0 || T < 4) { mk_set_error("masr_run_batch", "need B >= 1 and T >= 4"); return -1; }
    const bool train = (flags & MASR_TRAIN) != 0;
    int maxo = 0; int64_t ntot = 0;
    for (int b = 0; b < B; ++b) { if (olens[b] > maxo) maxo = (int)olens[b]; ntot += olens[b] + 1; }
    const int L = maxo + 1;
    Arena ar{m->ws, m->ws_bytes, m->persist_bytes};
    stream_close(m);
    plan_acts(m, ar, m->acts, B, T, L, train, true);
    if (ar.off > m->ws_bytes) { mk_set_error("masr_run_batch", "workspace too small (see masr_workspace_bytes)"); return -2; }
    Acts& a = m->acts; m->have_acts = true;
    const bool hybrid = m->ctc_w > 0.f;
    if (hybrid && 2 * maxo + 1 > 2048) { mk_set_error("masr_run_batch", "CTC objective: labels longer than 1023 tokens"); return -1; }
    const bool aug = train && m->aug_on;                           // SpecAugment: training steps under a policy (masr_set_specaug)
    if (aug && ((int64_t)T * T > INT32_MAX || (int64_t)T * m->D > INT32_MAX || B > 65535)) { mk_set_error("masr_run_batch", "SpecAugment: T * T and T * idim must fit an int, B <= 65535"); return -1; }
    // tok_in | gold | enc_lens | meta | tok_order | tok_start (| CTC target offsets | lengths) (| raw ilens)
    const int64_t stage_n = (int64_t)3 * B * L + B + 8 + m->C + 1 + (hybrid ? 2 * B : 0) + (m->aug_on ? B : 0);
    if (stage_n > m->stage_ints) {
        // the pinned staging ring grows with the batch (B * L) and the vocabulary (C): drain the copies in flight, then re-allocate
        for (auto& ev : m->stage_ev) HIP_CHECK_RET(hipEventSynchronize(ev));
        int* grown = nullptr;
        const int64_t want = stage_n + stage_n / 2;
        HIP_CHECK_RET(hipHostMalloc((void**)&grown, sizeof(int) * want * 4, hipHostMallocDefault));
        hipHostFree(m->h_stage);
        m->h_stage = grown; m->stage_ints = want;
    }
    // ---- MyTransformer.preprocess (:124-141): ys_in = [sos]+y padded with eos, ys_out = y+[eos] padded with -1
    const int slot = m->stage_slot; m->stage_slot = (slot + 1) & 3;
    HIP_CHECK_RET(hipEventSynchronize(m->stage_ev[slot]));
    int* h = m->h_stage + (int64_t)slot * m->stage_ints;
    int* h_in = h; int* h_out = h + (int64_t)B * L; int* h_len = h + (int64_t)2 * B * L;
    const int sos = 0, eos = m->C - 1;
    int64_t off = 0;
    for (int b = 0; b < B; ++b) {
        const int n = (int)olens[b];
        for (int l = 0; l < L; ++l) { h_in[b * L + l] = eos; h_out[b * L + l] = -1; }
        h_in[b * L] = sos;
        for (int l = 0; l < n; ++l) {
            const int tok = (int)ys_flat[off + l];
            if (tok < 0 || tok >= m->C) { mk_set_error("masr_run_batch", "label out of range"); return -1; }
            h_in[b * L + l + 1] = tok; h_out[b * L + l] = tok;
        }
        h_out[b * L + n] = eos;
        off += n;
        h_len[b] = (int)(ilens[b] / 4);                             // enc_lens = floor(ilens/4) (:117)
        if (h_len[b] < 1 || ilens[b] > T) { mk_set_error("masr_run_batch", "ilens must be in [4, T]"); return -1; }
    }
    Ctx c{m, s, step_seed_of(m->seed, m->step), train,
          train ? m->cfg.dropout : 0.f, train ? m->cfg.pos_dropout : 0.f};
    m->step++;
    const float inv_ntot = 1.0f / (float)ntot;
    // the chunk mask of this step's encoder self-attention (masr_set_chunk): the policy's size, or a dynamic policy's draw for a training step
    const bool chunk_dyn = train && m->chunk_on && m->chunk.dynamic;
    c.chunk = chunk_dyn ? chunk_draw_of(c.seed, a.Tp) : m->chunk.size; c.left = m->chunk.left;
    m->chunk_last = c.chunk;
    std::memcpy(h_len + B, &c.seed, 4); std::memcpy(h_len + B + 1, &inv_ntot, 4); h_len[B + 2] = c.chunk;     // Acts::meta
    {   // the decoder-input positions grouped by token (counting sort, stable: ascending position inside a token) for the embedding backward.
        // Only the positions 0 .. olens[b] of an utterance: behind them the inputs are eos padding whose gradient is exactly zero (their
        // outputs carry no loss, and the causal mask keeps every valid output from reading them) -- hundreds of hits on ONE table row
        // that a single workgroup column would sum for nothing.
        int* h_order = h_len + B + 8; int* h_start = h_order + (int64_t)B * L;
        const int V = m->C;
        group_positions_by_token(h_in, B, L, olens, V, h_order, h_start);
        if (hybrid) {
            // CTC targets: the labels of utterance b are the first olens[b] entries of its gold row (behind them: eos, then -1).  Every
            // 2 olen + 1 fits the lattice the work buffer holds (2 max olen + 1); olen > enc_len is left to zero_infinity
            int* h_ctc = h_start + V + 1;
            for (int b = 0; b < B; ++b) { h_ctc[b] = b * L; h_ctc[B + b] = (int)olens[b]; }
        }
        if (m->aug_on) {
            // the raw frame lengths, behind everything else: SpecAugment draws its centres and masks inside [0, ilens) (enc_lens is ilens / 4)
            int* h_raw = h_start + V + 1 + (hybrid ? 2 * B : 0);
            for (int b = 0; b < B; ++b) h_raw[b] = (int)ilens[b];
        }
    }
    HIP_CHECK_RET(hipMemcpyAsync(a.tok_in, h, sizeof(int) * (size_t)stage_n, hipMemcpyHostToDevice, s));   // tok_in | gold | enc_lens | meta | tok_order | tok_start
    HIP_CHECK_RET(hipEventRecord(m->stage_ev[slot], s));

    auto run = [&](Ctx& cc) -> int {
        m->n_ksplit = 0;
        // under a policy the step's first launch augments the batch; conv1's forward AND conv1's weight gradient (backward) read the result
        const float* x_in = xs;
        if (aug) {
            Prof p(m, MASR_PROF_MISC, s);
            CK(mk_specaug(xs, a.raw_lens, a.xa, B, T, a.D, m->aug, cc.seed, cc.seed_ptr, s));
            x_in = a.xa;
        }
        CK(forward_encoder(cc, x_in));
        CK(forward_decoder(cc));
        { Prof p(m, MASR_PROF_MISC, s);
          CK(mk_ls_ce(a.logits, m->Cp, a.gold, a.rows_d, m->C, m->cfg.label_smoothing, inv_ntot, a.dlogits, a.row_loss, a.row_correct,
                      m->stats, s, cc.inv_ptr, 1.f - m->ctc_w)); }
        if (hybrid) CK(ctc_forward(cc));
        if (train) CK(backward(cc, x_in));
        return 0;
    };
    m->aug_ran = aug;
    // ---- a batch shape seen twice in a row is captured once and replayed from then on (everything that changes from step to
    // step -- tokens, lengths, dropout seed, 1/n_total -- reaches the kernels through the upload above)
    const bool graphs_on = m->step_graphs_on;
    const int key[4] = {B, T, L, train ? 1 : 0};
    const bool repeat = !memcmp(key, m->last_key, sizeof key) && m->last_xs == (const void*)xs;
    memcpy(m->last_key, key, sizeof key); m->last_xs = xs;
    if (!graphs_on || s == nullptr || m->prof || !repeat) { ++m->n_direct; return run(c); }
    masr_model::StepGraph* sg = nullptr;
    for (auto& g : m->step_graphs)
        if (g.B == B && g.T == T && g.L == L && g.train == key[3] && g.ws == m->ws && g.P == m->P && g.xs == (const void*)xs) { sg = &g; break; }
    if (!sg) {
        if (m->step_graphs.size() >= 8) {                            // evict the least recently used (nothing of it may be in flight)
            HIP_CHECK_RET(hipStreamSynchronize(s));
            size_t lru = 0;
            for (size_t i = 1; i < m->step_graphs.size(); ++i) if (m->step_graphs[i].used < m->step_graphs[lru].used) lru = i;
            hipGraphExecDestroy(m->step_graphs[lru].e); hipGraphDestroy(m->step_graphs[lru].g);
            m->step_graphs.erase(m->step_graphs.begin() + lru);
        }
        masr_model::StepGraph ng{B, T, L, key[3], m->ws, m->P, xs, nullptr, nullptr, 0};
        Ctx cc = c; cc.seed_ptr = a.meta; cc.inv_ptr = reinterpret_cast<const float*>(a.meta + 1);
        if (chunk_dyn) cc.chunk_ptr = reinterpret_cast<const int*>(a.meta + 2);      // a drawn chunk changes from step to step: read at replay
        HIP_CHECK_RET(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = run(cc);
        const hipError_t e = hipStreamEndCapture(s, &ng.g);
        if (rc || e != hipSuccess) { mk_set_error("masr_run_batch", "stream capture of the step failed"); return -1; }
        HIP_CHECK_RET(hipGraphInstantiate(&ng.e, ng.g, nullptr, nullptr, 0));
        m->step_graphs.push_back(ng);
        sg = &m->step_graphs.back();
        ++m->n_captured;
    }
    sg->used = ++m->graph_clock;
    HIP_CHECK_RET(hipGraphLaunch(sg->e, s));
    ++m->n_replayed;
    return 0;
}
