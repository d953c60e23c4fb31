// Internal (not part of the C ABI): the H = 128 GRU layers of gru128.hip, launched by the
// lg_gru_seq_* dispatchers of gru.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int64_t kGru128H = 128;

struct LgGru128Drop {
    int on;
    float p, scale;
    uint64_t seed;
    uint32_t salt;
};

// Dense forward: x [L][Nseq][I] -> h_seq [L][Nseq][128] (or NULL), gates [L][Nseq][4][128] (or
// NULL), h_last [Nseq][128] (or NULL).  I in 1..1024.
int lg_gru128_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                  float* h_seq, float* gates, float* h_last, int64_t Nseq, int64_t L, int64_t I,
                  const LgGru128Drop& dr, hipStream_t s);

// Window forward: gi [B][T][384] holds W_ih x + b_ih; sequence q = k * B + b reads row (b, k + t).
int lg_gru128_win_fwd(const float* gi, const float* w_hh, const float* b_hh, float* h_seq, float* h_last, int64_t B,
                      int64_t T, int64_t l_pred, int64_t n_win, hipStream_t s);

// Dense backward.  Workspace: lg_gru128_bwd_ws_bytes(Nseq, I) at least (more lets the call take
// more steps per pass).  The weight / bias gradients end in the library's slab reduction.
int64_t lg_gru128_bwd_ws_bytes(int64_t Nseq, int64_t I);
int lg_gru128_bwd(const float* x, const float* w_ih, const float* w_hh, const float* h_seq, const float* gates,
                  const float* dh_seq, const float* dh_last, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                  float* db_hh, int64_t Nseq, int64_t L, int64_t I, const LgGru128Drop& dr, void* workspace,
                  int64_t ws_bytes, hipStream_t s);
