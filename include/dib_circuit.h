/* dib_circuit.h - C ABI of the Boolean-circuit kernels (complex_systems/InfoDecomp_Boolean_circuits.ipynb cells 4 and 6).
 *
 * The notebook's model: one SimpleEncoder per input gate g with two trainable scalars, x in {-1, +1} -> N(x s_g, exp(lv_g)),
 * and a predictor Dense(256, leaky_relu) x3 -> Dense(1) over the G sampled embeddings, trained with BCE from logits plus
 * beta * sum_g KL_g.  The scalars sit in one float array sc: s[0..G) then lv[0..G).
 *
 * Truth table: 2^G uint32 rows, bit g = input g (0 / 1), bit G = y; the notebook's 'xy'-meshgrid row order.
 * Row draw (training batch, row b of B at step `step`): r_b = x0 >> (32 - G), x0 the first Philox4x32-10 output for counter
 *   (b, 0xFFFFFFFF, 0, step) and key seed - exactly uniform over the 2^G rows, with replacement.
 * Noise: eps[b][g] = the library's normal keyed (seed, step, row b, feature g, dim 0) (dib_philox_normal_ref).
 * Envelope: 1 <= G <= 16, 1 <= B <= 2048; everything else is DIB_E_UNSUPPORTED (nothing launched).
 * Part of libdib_hip.so; its revision is DIB_ABI_VERSION of dib_hip.h. */
#ifndef DIB_CIRCUIT_H
#define DIB_CIRCUIT_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_CIRCUIT_U_LD 16   /* row pitch of u and g_u: 16 * ceil(G / 16), the row-tile head's in_dim (pad columns are 0) */

/* 1 if (G, B) is inside the envelope */
int dib_circuit_supported(int G, int B);
/* Everything in front of the predictor, one launch: rows_out[b] = the drawn row (row_idx[b] mod 2^G instead when row_idx is
 * non-NULL), u [B][16] = x sc_s + exp(sc_lv / 2) eps with x = 2 bit - 1 (pad columns 0), y [B] = the row's output bit,
 * kl [G + 1] = {KL_0 .. KL_{G-1}, beta * sum_g KL_g} (summed in gate order). */
int dib_circuit_fwd(const uint32_t* table, int G, int B, const float* sc, uint64_t seed, uint32_t step, float beta,
                    const int32_t* row_idx, int32_t* rows_out, float* u, float* y, float* kl, dib_stream_t stream);
/* Gradient of the 2G scalars given g_u [B][16] = dL/du of the predictor (dib_mlp_small_head_step's g_x), the rows the forward
 * drew, the same seed / step / beta:  g_sc[g] = sum_b g_u[b][g] x[b][g] + beta s_g,
 * g_sc[G + g] = sum_b g_u[b][g] eps[b][g] exp(lv_g / 2) / 2 + beta (exp(lv_g) - 1) / 2.  One workgroup per gate, float64 sums
 * in a fixed order (the same bits on any device). */
int dib_circuit_bwd(const uint32_t* table, int G, int B, const float* sc, uint64_t seed, uint32_t step, float beta,
                    const int32_t* rows, const float* g_u, float* g_sc, dib_stream_t stream);
/* Sandwich bounds (utils.estimate_mi_sandwich_bounds / the notebook's compute_batch, nats, float64 with log-sum-exp) of every
 * gate's channel for nb evaluation batches of n points each: x [nb][n] (+-1), eps of point i of batch b keyed (seed, b, i, g);
 * out [G][nb][2] = per-batch {lower, upper}.  The values of dib_mi_sandwich_rows(enc = [x s_g, lv_g], n, 1, seed, b, g) averaged
 * over its rows, up to the summation order (64 points per workgroup, four lanes per point, fixed-order partial sums).
 * ws: dib_circuit_mi_workspace_bytes, zero-filled once by the caller (arrival counters, self-cleaning). */
int64_t dib_circuit_mi_workspace_bytes(int G, int n, int nb);
int dib_circuit_mi_bounds(const float* sc, int G, const float* x, int n, int nb, uint64_t seed, double* out, void* ws,
                          dib_stream_t stream);

/* ---- R replicas per launch (CircuitEnsemble) ----
 * The model's shapes do not depend on the circuit (u is 16 columns wide for every G), so R models that differ in circuit, G,
 * seed and beta share every launch: the replica is a grid index, each workgroup runs the single kernel's code on its
 * replica's slices, and every output of replica r has the bits of the single entry point called on those slices.
 * Replica r's scalars are params + r * param_stride + sc_off (s[0..G_r) then lv[0..G_r)); G, table_off, seeds and beta are HOST
 * arrays of R entries (they travel in the kernel arguments, 64 replicas per launch: a larger ensemble takes ceil(R / 64)
 * launches).  tables: the R packed truth tables in one device buffer of table_words words, replica r's 2^G_r words at
 * table_off[r].  A refusal (R < 1, any G_r or B outside the envelope: DIB_E_UNSUPPORTED; a NULL pointer, a negative stride, a
 * table outside the buffer: DIB_E_ARG) launches nothing. */
int dib_circuit_batched_supported(const int* G, int replicas, int B);
/* row_idx [R][B] or NULL; rows_out [R][B], u [R][B][16], y [R][B], kl [R][17] (replica r: {KL_0 .. KL_{G_r-1}, beta_r sum KL},
 * the rest of its row untouched). */
int dib_circuit_fwd_batched(const uint32_t* tables, int64_t table_words, const int64_t* table_off, const int* G, int replicas, int B,
                            const float* params, int64_t param_stride, int64_t sc_off, const uint64_t* seeds, uint32_t step,
                            const float* beta, const int32_t* row_idx, int32_t* rows_out, float* u, float* y, float* kl,
                            dib_stream_t stream);
/* rows [R][B], g_u [R][B][16]; the 2 G_r gradients of replica r go to grads + r * grad_stride + sc_off.  Grid (gate, replica):
 * the same float64 fixed-order sums as dib_circuit_bwd. */
int dib_circuit_bwd_batched(const uint32_t* tables, int64_t table_words, const int64_t* table_off, const int* G, int replicas, int B,
                            const float* params, int64_t param_stride, int64_t sc_off, const uint64_t* seeds, uint32_t step,
                            const float* beta, const int32_t* rows, const float* g_u, float* grads, int64_t grad_stride,
                            dib_stream_t stream);
/* x [R][nb][n]; out [R][16][nb][2], rows g >= G_r untouched; ws: dib_circuit_mi_batched_workspace_bytes (one slice per replica),
 * zero-filled once by the caller. */
int64_t dib_circuit_mi_batched_workspace_bytes(int replicas, int n, int nb);
int dib_circuit_mi_bounds_batched(const float* params, int64_t param_stride, int64_t sc_off, const int* G, int replicas,
                                  const float* x, int n, int nb, const uint64_t* seeds, double* out, void* ws,
                                  dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_CIRCUIT_H */
