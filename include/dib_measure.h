/* dib_measure.h - C ABI of the measurement-partition kernels (chaos notebook, Chaos_experiments.ipynb cells 3 and 10).
 *
 * The model between the IB encoder's output enc [rows, 2E] = (mu | logvar) and the measurement aggregator's input:
 *   z = mu + eps * exp(logvar / 2)      eps keyed (seed, step, row, feature 0, dim) like dib_token_reparam_kl_fwd
 *   VQ network: E -> Dense(H1, act) -> Dense(H2, act) -> Dense(A), softmax (temperature 1)
 * Layer l of the VQ network: kernel [in_l][out_l] row-major (Keras) at params + w_off[l], bias at params + b_off[l].
 * Envelope (dib_measure_supported): in_dim <= 4, E <= 32, 2 <= A <= 16, L <= 32, H1 / H2 multiples of 16 up to 128 (the
 * chain of a 16-row tile lives in registers); everything else is DIB_E_UNSUPPORTED (nothing launched).  Part of libdib_hip.so;
 * its revision is DIB_ABI_VERSION of dib_hip.h. */
#ifndef DIB_MEASURE_H
#define DIB_MEASURE_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dib_measure_desc {
  int64_t w_off[3], b_off[3];
  int32_t in_dim, E, H1, H2, A, L, act;   /* act: DIB_ACT_* of the VQ hidden layers (linear / relu / leaky_relu) */
  int32_t pad_;
} dib_measure_desc;   /* 80 bytes */

/* 1 if the shape is inside the envelope and the packed VQ weights of the largest kernel fit in one workgroup's LDS */
int dib_measure_supported(const dib_measure_desc* d);
/* bytes of the forward's workspace for `rows` rows (KL partials + arrival counter); zero-fill it once */
int64_t dib_measure_workspace_bytes(const dib_measure_desc* d, int rows);
/* Forward over rows = B * L sequence states (row = b * L + l): z, h1, h2 stashes [rows][E | H1 | H2]; soft [rows][A] = the
 * aggregator's input [B][L * A]; out3 = {kl (mean over rows), beta * L * kl^p, p * beta * L * kl^(p-1) / rows}; the last
 * workgroup to arrive sums the per-workgroup KL partials in workgroup order. */
int dib_measure_fwd(const dib_measure_desc* d, const float* params, const float* enc, int rows, uint64_t seed, uint32_t step,
                    float beta, float kl_exponent, float* z, float* h1, float* h2, float* soft, float* out3, void* ws,
                    dib_stream_t stream);
/* Backward: dsoft = g_agg [B][agg_width] (dL/d pre-activation of the aggregator's first layer) @ w_agg0[L*A][agg_width]^T,
 * softmax backward, VQ dgrad chain; writes g3 [rows][A], g2 [rows][H2], g1 [rows][H1] (dL/d pre-activations: with z / h1 / h2
 * the operands of the VQ weight gradients) and g_enc [rows][2E] = dL/d(mu | logvar) including the nonlinear-KL term
 * out3[2] * d(kl row)/d(mu | logvar) read from the forward's out3. */
int dib_measure_bwd(const dib_measure_desc* d, const float* params, const float* enc, int rows, uint64_t seed, uint32_t step,
                    const float* h1, const float* h2, const float* soft, const float* g_agg, const float* w_agg0,
                    int agg_width, const float* out3, float* g3, float* g2, float* g1, float* g_enc, dib_stream_t stream);
/* ---- `replicas` independent models of one shape in one launch each (MeasurementEnsemble) ----
 * Replica r has its packed VQ parameters at params + r * param_stride (a multiple of 4 floats), its noise seed seeds[r] (a HOST
 * array, read before the call returns) and slice r of every row buffer: enc, z, h1, h2, soft, g3, g2, g1, g_enc are
 * [replicas][rows][...] contiguous, g_agg [replicas][rows / L][agg_width], w_agg0 at w_agg0 + r * w_agg0_stride, out3
 * [replicas][3].  The row index of the noise key is local to the replica (row = b * L + l), so replica r computes, bit for bit,
 * what dib_measure_fwd / dib_measure_bwd compute on its slices with seed seeds[r]: the replica is an outer grid index, each
 * replica sums its own KL partials behind its own arrival counter, and no workgroup waits on another.  One launch each for up
 * to 64 replicas (one more per further 64).  Workspace of the forward: dib_measure_batched_workspace_bytes, zero-filled once. */
int64_t dib_measure_batched_workspace_bytes(const dib_measure_desc* d, int rows, int replicas);
int dib_measure_fwd_batched(const dib_measure_desc* d, const float* params, int64_t param_stride, const float* enc, int rows,
                            int replicas, const uint64_t* seeds, uint32_t step, float beta, float kl_exponent, float* z, float* h1,
                            float* h2, float* soft, float* out3, void* ws, dib_stream_t stream);
int dib_measure_bwd_batched(const dib_measure_desc* d, const float* params, int64_t param_stride, const float* enc, int rows,
                            int replicas, const uint64_t* seeds, uint32_t step, const float* h1, const float* h2,
                            const float* soft, const float* g_agg, const float* w_agg0, int64_t w_agg0_stride, int agg_width,
                            const float* out3, float* g3, float* g2, float* g1, float* g_enc, dib_stream_t stream);
/* Symbolisation of n points from their encodings enc [n][2E]: for each of the K noise vectors noise [K][E],
 * argmax(VQ(mu + noise_k * exp(logvar / 2))) (first maximum wins); sym[i] = (mean_k argmax > 0.5) as uint8 - the reference's
 * rule for every alphabet size; counts [n][A] (may be NULL): how often each symbol was the argmax. */
int dib_measure_symbolize(const dib_measure_desc* d, const float* params, const float* enc, int64_t n, const float* noise,
                          int K, uint8_t* sym, int32_t* counts, dib_stream_t stream);
/* PositionalEncoding(2**arange(first_exponent, first_exponent + n_freq - 1)) of rows row_idx[0..n) of x:
 * out [n][d * n_freq] = [x, sin(2^f0 x), sin(2^(f0+1) x), ...] (the notebook's reference-state encoder: f0 = 0) */
int dib_measure_posenc_rows(const float* x, int64_t ldx, const int32_t* row_idx, int n, int d, int n_freq, int first_exponent,
                            float* out, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_MEASURE_H */
