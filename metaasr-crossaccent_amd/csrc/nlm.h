// LSTM language model on the device (nlm.hip): what the host builder, the step kernels, the decoders' entry points and the test
// entry share.  Embedding [C][E] -> L LSTM layers of H units -> Linear [C][H].  E and H are padded up to multiples of 32 (Ep, Hp) with
// zeros, so every reduction is whole 32-wide MFMA chunks and a padded unit's c and h stay exactly 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

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
};
inline int64_t nlm_state_elems(const NlmDev& d, int R) { return 2 * (int64_t)d.L * R * d.Hp; }

// the L layer launches, then the output projection (decode.hip's skinny GEMM) into logits fp32 [R][ld]
int mk_nlm_step(const NlmDev& lm, const NlmStepArgs& a, float* logits, long ld, hipStream_t s);
// out [R][ldo] = the log_softmax of logits [R][ld] over the C classes, (y - mx) - log_s of search.h row_lse
int mk_nlm_logp(const float* logits, long ld, int R, int C, float* out, long ldo, hipStream_t s);
