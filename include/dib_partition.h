/* dib_partition.h - C ABI of the random-MLP partition kernel (chaos notebook, Chaos_experiments.ipynb cell 7; the paper's Fig. 1).
 *
 * A partition of a d-dimensional state space given by a plain MLP, described by dib_mlp_desc of dib_hip.h (layer l: kernel
 * [in_l][out_l] row-major (Keras) at params + w_off[l], bias at params + b_off[l]; a DenseStack's flat buffer passes unchanged):
 *   x [d] (fp32, or fp64 cast to fp32 first) -> n_hidden x Dense(width[l], act) -> Dense(A = width[n_hidden])  (linear)
 *   symbol = argmax_k |logit_k|   (uint8; the first index wins exact ties, so all-zero logits give symbol 0)
 * A NaN logit never wins: its magnitude ranks below every number; a point whose logits are all NaN gets symbol 0.
 * Exact fp32 MFMA operands; tanh is the accurate tanhf.  fp64 input gives the same bits as its float32 cast.
 *
 * Envelope (dib_partition_supported): 1 <= in_dim <= 4, n_freq <= 1 (no positional encoding), 1 <= n_hidden <= 3, hidden widths
 * multiples of 16 up to 128, 2 <= A <= 16, act in {DIB_ACT_LINEAR, DIB_ACT_RELU, DIB_ACT_LEAKY_RELU (0.2), DIB_ACT_TANH}.
 * Outside it every entry returns DIB_E_UNSUPPORTED and launches nothing.  Part of libdib_hip.so; additions only within
 * DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_PARTITION_H
#define DIB_PARTITION_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the network is inside the envelope */
int dib_partition_supported(const dib_mlp_desc* d);
/* Symbolises n points x [n][ldx] (x_is_f64: 0 = float, 1 = double; ldx >= in_dim elements) in one launch:
 *   sym [n] uint8, logits [n][A] fp32 (may be NULL), counts [A] int64 (may be NULL): the symbol histogram of these n points is
 *   ADDED into counts (integer sums: deterministic), so a caller-zeroed buffer accumulates over chunked calls.
 * DIB_E_ARG for a NULL params / x / sym, n < 0 or ldx < in_dim (nothing launched); n == 0 launches nothing. */
int dib_partition_symbolize(const dib_mlp_desc* d, const float* params, const void* x, int x_is_f64, int64_t ldx, int64_t n,
                            uint8_t* sym, float* logits, int64_t* counts, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_PARTITION_H */
