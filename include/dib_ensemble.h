/* dib_ensemble.h - C ABI of the kernels a LOCKSTEP step of R DistributedIBNet replicas needs besides dib_gemm_grouped
 * (dib_st.h), dib_reduce_splits and dib_adam_step: R models of one architecture (F features of d columns each, embedding
 * width E) that differ in weights, noise seed, batch rows and beta share every launch.  The replica is a grid index; every
 * output of replica r has the bits the same entry point gives at R = 1 on that replica's slices, and the arithmetic is the
 * single model's (dib_encoder_bank_fwd's reparameterisation and KL, dib_loss_fwd_bwd, dib_metrics_accumulate).
 *
 * Layouts (row-major, contiguous): rows [R][n] int32 dataset rows - they gather x and the labels and key the noise
 * (seed_r, step, dataset row, feature, dim: dib_philox_normal_ref); enc, d_enc [R][F][n][2E] (mu | logvar); u, g_u [R][n][F E];
 * pred, g_pred [R][n][out_dim]; kl [R][F]; beta [R] and seeds [R] (uint64) are DEVICE arrays.
 *
 * Envelope (dib_ens_supported): 1 <= R, 1 <= F, R F <= 65535, 1 <= E <= 1024 (a row of one feature is one pass of a 256-thread
 * workgroup, four dimensions per thread - the single kernel's own limit), 1 <= n <= 2048, 1 <= out_dim <= 16, kind 0
 * (BinaryCrossentropy from logits), 2 (SparseCategoricalCrossentropy from logits) or 3 (mse).  Outside it every entry returns
 * DIB_E_UNSUPPORTED, launches nothing and writes nothing; a NULL pointer or a bad size is DIB_E_ARG.
 * ws: dib_ens_workspace_bytes(R, F, E, n) bytes, zero-filled once by the caller (workgroup partials and self-cleaning arrival
 * counters); one workspace serves the forward and the loss of one stream.  Sums are taken in a fixed order: no float atomics,
 * the same bits every call.  Part of libdib_hip.so; its revision is DIB_ABI_VERSION of dib_hip.h. */
#ifndef DIB_ENSEMBLE_H
#define DIB_ENSEMBLE_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the shape is inside the envelope (host only: answers without a device) */
int dib_ens_supported(int R, int F, int E, int n, int out_dim, int kind);
int64_t dib_ens_workspace_bytes(int R, int F, int E, int n);
/* Batch gather + positional encoding for every (replica, feature): x [N][ldx] with F features of d columns,
 * out [R F][n][n_blocks d], out[r F + f][b][j d + c] = (j == 0 ? v : sin(2^j v)), v = x[rows[r][b]][f d + c].  Each x row is read
 * once per replica.  1 <= d, 1 <= n_blocks <= 32, (R, F, n) as in the envelope. */
int dib_ens_posenc_rows(const float* x, int64_t ldx, const int32_t* rows, int R, int F, int d, int n_blocks, int n, float* out,
                        dib_stream_t stream);
/* u = mu + exp(logvar / 2) eps (deterministic != 0: u = mu) and kl[r][f] = sum_b sum_e (mu^2 + exp(lv) - lv - 1) / 2 */
int dib_ens_reparam_kl_fwd(const float* enc, const int32_t* rows, const uint64_t* seeds, uint32_t step, int deterministic, int R,
                           int F, int E, int n, float* u, float* kl, void* ws, dib_stream_t stream);
/* Task loss of every replica, g_pred = d(mean loss)/d pred * inv_b (times act'(pred) of out_act), and the History sums of the
 * step ADDED to metrics_acc [R][F + 3]: [f] kl[r][f] inv_b, [F] task sum + beta_r sum_f kl[r][f], [F + 1] rows predicted
 * right, [F + 2] n.  y [N][ldy] labels, read at rows[r][b]. */
int dib_ens_loss(int kind, const float* pred, int out_dim, const float* y, int64_t ldy, const int32_t* rows, int R, int F, int n,
                 float inv_b, int out_act, const float* beta, const float* kl, float* g_pred, float* metrics_acc, void* ws,
                 dib_stream_t stream);
/* d_enc: dmu = g_u + beta_r inv_b mu, dlogvar = g_u (u - mu) / 2 + beta_r inv_b (exp(lv) - 1) / 2; nothing is regenerated */
int dib_ens_reparam_kl_bwd(const float* enc, const float* g_u, const float* u, const float* beta, float inv_b, int R, int F, int E,
                           int n, float* d_enc, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_ENSEMBLE_H */
