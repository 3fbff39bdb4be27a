/* dib_mi_features.h - C ABI of the per-feature information bounds of a DistributedIBNet in one evaluation: the InfoNCE lower
 * and leave-one-out upper bound on I(U_f; X_f) (reference utils.py:10-73, models.py:188-223; Poole et al. 2019) of EVERY feature
 * and EVERY evaluation batch, from the feature-major encoding that one dib_encoder_bank_fwd(DIB_FWD_DETERMINISTIC |
 * DIB_FWD_INFERENCE) leaves in DIB_WS_ENC_OUT - instead of one dib_encode_deterministic + dib_mi_sandwich_rows + read-back per
 * (feature, batch).
 *
 * enc [F][plane_rows][2E] (fp32, mu | logvar) is feature-major.  Group (f, b), f < F, b < nb, is the n rows
 * row0 + b n + i, i < n, of plane f:
 *   u_i     = mu_i + exp(logvar_i / 2) eps,  eps = the library's counter-based normal noise keyed (seed, step0 + b, row i,
 *             feature0 + f) - the keys of dib_mi_sandwich_rows(enc_fb, n, E, seed, step0 + b, feature0 + f) on that slice
 *             (oracle/dib_oracle.py philox_normal regenerates it)
 *   l_ij    = log N(u_i; mu_j, diag sigma_j^2)
 *   lower_i = l_ii - (LSE_j l_ij - log n),   upper_i = l_ii - (LSE_{j != i} l_ij - log n),  j != i by POSITION
 *   out[f][b] = (mean_i lower_i, mean_i upper_i) in nats.
 * float64 with a log-sum-exp (far-apart Gaussians give lower = log n instead of an underflow; their upper bound is +inf).
 * Deterministic: per-workgroup (max, sum) partials merged in a fixed order, no floating-point atomics.  The order depends on
 * (E, n) alone - not on the device, F or nb - so a replay, a split of the features over several calls (feature0 advanced, enc
 * offset by the planes already done) and a split of the batches over several calls (step0 and row0 advanced) give the same bits.
 * Three launches per call whatever F and nb are.
 *
 * Envelope: 1 <= E <= 64, or E a multiple of 4 up to 256; 2 <= n <= 16384; 1 <= F nb <= 65535.  Outside it
 * dib_mi_features_supported returns 0 and dib_mi_features_bounds returns DIB_E_UNSUPPORTED; DIB_E_ARG for a non-positive size,
 * a NULL enc / out / ws, a ws that is not 16-byte aligned, row0 < 0 or row0 + nb n > plane_rows, or only one of lower_rows /
 * upper_rows given.  A refused call launches nothing.  dib_mi_features_workspace_bytes returns the same negative codes and, like
 * dib_mi_features_supported, is host-only (callable without a GPU).  lower_rows / upper_rows [F][nb][n] (both or neither) and
 * u_out [F][nb][n][E] are optional (NULL).  ws needs no initialisation.  The call enqueues on `stream`, never allocates and
 * never synchronises: it can be captured into a hipGraph.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_MI_FEATURES_H
#define DIB_MI_FEATURES_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int dib_mi_features_supported(int F, int E, int n, int nb);
int64_t dib_mi_features_workspace_bytes(int F, int E, int n, int nb);
int dib_mi_features_bounds(const float* enc, int64_t plane_rows, int64_t row0, int F, int E, int n, int nb, uint64_t seed,
                           uint32_t step0, uint32_t feature0, double* out, double* lower_rows, double* upper_rows, double* u_out,
                           void* ws, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_MI_FEATURES_H */
