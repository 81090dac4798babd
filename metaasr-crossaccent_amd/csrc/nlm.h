// LSTM language model on the device (nlm.hip): what the host builder, the step kernels, the decoders' entry points and the test
// entry share.  Embedding [C][E] -> L LSTM layers of H units -> Linear [C][H].  E and H are padded up to multiples of 32 (Ep, Hp) with
// zeros, so every reduction is whole 32-wide MFMA chunks and a padded unit's c and h stay exactly 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

constexpr int NLM_MAX_LAYERS = 4;
constexpr int NLM_MAX_DIM = 2048;

struct NlmDev {
    int C, E, H, L, Ep, Hp, start_id;
    const bf16* embed;                       // [C][Ep]
    const bf16* w[NLM_MAX_LAYERS];           // [4 Hp][INp + Hp]: W_ih | W_hh of gate g, unit u in row g * Hp + u (g in torch's order i, f, g, o); INp = Ep for layer 0, else Hp
    const float* b[NLM_MAX_LAYERS];          // [4 Hp]: fl(b_ih + b_hh), same rows
    const bf16* lo;                          // [C][Hp]
    const float* lo_b;                       // [C]
};

// the handle of include/masr.h
struct masr_nlm {
    NlmDev dev;
    void* mem;                               // one device allocation
    int64_t bytes;
    uint32_t serial;                         // unique per created model: keys the cached step graph
};

// One step of the layer stack on R rows.  The step st (1-based) is read from *step.  At st = 1 every row feeds start_id from the zero state;
// later row r feeds tok_hist[(st - 2) * hist_stride + r] (an id outside [0, C) reads as 0) and continues the state of its parent row
// par_hist[(st - 2) * hist_stride + r] (null: the row itself; a parent outside the K rows of r's utterance reads as r).  The states live in
// hstate bf16 / cstate fp32 [2][L][R][Hp] by step parity: a row reads its parent's at parity (st - 1) & 1 and writes its own at st & 1, and
// the top layer's new h also goes to htop [R][Hp], the output projection's operand at an address that does not depend on the step.
// A row with score == -inf or of an utterance with fin != 0 (either array may be null: none such) writes nothing.
struct NlmStepArgs {
    const int* step;
    int R, K;
    const int *tok_hist, *par_hist; long hist_stride;
    const float* score; const int* fin;
    bf16* hstate; float* cstate; bf16* htop;
    const int* live;                         // the carry form only (mk_nlm_step_carry): live counts [2][R / K] by step parity
};
inline int64_t nlm_state_elems(const NlmDev& d, int R) { return 2 * (int64_t)d.L * R * d.Hp; }

// the L layer launches, then the output projection (decode.hip's skinny GEMM) into logits fp32 [R][ld]
int mk_nlm_step(const NlmDev& lm, const NlmStepArgs& a, float* logits, long ld, hipStream_t s);
// out [R][ldo] = the log_softmax of logits [R][ld] over the C classes, (y - mx) - log_s of search.h row_lse
int mk_nlm_logp(const float* logits, long ld, int R, int C, float* out, long ldo, hipStream_t s);

// The carry form of the step, for a search whose rows mostly do NOT take a token (the CTC prefix beam).  The histories are one
// slot per row (hist_stride 0): tok_hist[r] in [1, C - 2] is the row's token, anything else marks a STAY; par_hist[r] its parent row (outside
// the K rows of r's utterance: r).  Row r of utterance u is live when r - u * K < live[(st & 1) * (R / K) + u].  At step st
//   a token row computes from its parent's state at parity (st - 1) & 1 exactly as mk_nlm_step does, and its logits go through the
//   log-softmax into logp[st & 1][r]  (logp fp32 [2][R][ldp]);
//   a stay row copies its parent's (h, c) of every layer and its parent's logp row from parity (st - 1) & 1 to its own slot at st & 1;
//   a dead row writes nothing.
// A 16-row tile without a token row skips its reduction.  At st = 1 every live row feeds start_id from the zero state.  The last launch
// advances *step (search.h step_ticket).
int mk_nlm_step_carry(const NlmDev& lm, const NlmStepArgs& a, float* logits, long ld, float* logp, long ldp, int* step, hipStream_t s);

// ---- the CTC prefix beam with the LSTM LM (ctc_beam.hip)
struct CtcNlmArgs {
    int* step;                               // [2] the step word st and its ticket: frame t runs at st = t + 2
    float* wts;                              // lm_w, len_bonus
    float *pb, *pnb, *lmacc; int *last, *len; unsigned long long *hash, *phash;      // the beam by parity [2][B][K]
    int* nlive;                              // [2][B] live entries
    int *tok, *par;                          // [R] the frame's token (-1: stay) and parent row of every kept entry
    float* logp; long ldp;                   // [2][R][ldp] the rows' LM log-softmax
    float* am;                               // [B][nbest]
};
struct CtcNlmRun { CtcBeamArgs a; CtcNlmArgs q; NlmStepArgs st; NlmDev lm; float* logits; long ldl; };
int64_t mk_ctc_beam_nlm_work_bytes(const masr_nlm* nlm, int B, int Tp, int C, int K);
// begin: the checks (-1 with the message under fn), the frames' log-sum-exp and token sets, the initial beam and LM step 1; frame: ONE frame
// for every utterance, parameter-identical launches (the frame number is the device step word); end: the tail.  The operator below is begin,
// Tp frames, end.
int mk_ctc_beam_nlm_begin(const char* fn, const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                          const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, const int* tokens, const int* lens,
                          const float* scores, float* am, CtcNlmRun* run, hipStream_t s);
int mk_ctc_beam_nlm_frame(const CtcNlmRun& r, hipStream_t s);
int mk_ctc_beam_nlm_end(const CtcNlmRun& r, int nbest, int* tokens, int* lens, float* scores, hipStream_t s);
int mk_ctc_beam_search_nlm(const float* logits, long ld, const int* enc_lens, int B, int Tp, int C, int K, int nbest, int blank, int eos,
                           const masr_nlm* nlm, float lm_w, float len_bonus, void* work, int64_t work_bytes, int* tokens, int* lens, float* scores,
                           float* am, hipStream_t s);
