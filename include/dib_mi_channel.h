/* dib_mi_channel.h - C ABI of the Monte-Carlo estimate of I(U;X) for a channel whose conditionals p(u|x) are known diagonal
 * Gaussians (the reference's "Characterization of mutual information bounds with synthetic data" notebook, paper Fig. S4): the
 * number that the InfoNCE lower and leave-one-out upper bounds of dib_mi_sandwich_rows / dib_mi_sandwich_batched bracket.
 *
 * enc_tables [n_tables][n_rows][2E] (fp32, mu | logvar) holds one dataset of n_rows conditionals per table.  Group g evaluates
 * table group_table[g] with n_samples samples; sample s of group g is drawn from row r = src_idx[g][s]:
 *   u    = mu_r + exp(logvar_r / 2) eps,  eps = the library's counter-based normal noise keyed (seed, step0 + g, row s, feature 0)
 *          - the keys of dib_mi_sandwich_rows / dib_mi_sandwich_batched (oracle/dib_oracle.py philox_normal regenerates it)
 *   term = l_r - (LSE_j l_j - log n_rows),  l_j = log N(u; mu_j, diag sigma_j^2) over ALL n_rows rows of the table, by position
 *          (a row that is in the table twice counts twice: p(u) is the plain mean over the dataset's rows)
 *   group_means[g] = mean of the group's terms (nats).
 * float64 with a log-sum-exp (far-apart Gaussians give log(n_rows / multiplicity) instead of an underflow); any per-row logvar.
 * Deterministic: per-workgroup (max, sum) partials merged in a fixed order, no floating-point atomics; the order depends on
 * (n_rows, n_samples) alone, so a replay and a split of the groups over several calls (step0 advanced by the groups already
 * done) give the same bits.
 *
 * Envelope: 1 <= E <= 64, 2 <= n_rows <= 65536, 1 <= n_samples <= 2^20, 1 <= n_groups <= 65535, 1 <= n_tables <= 65536.
 * Outside it dib_mi_monte_carlo returns DIB_E_UNSUPPORTED (DIB_E_ARG for a non-positive size, a NULL enc_tables / group_table /
 * src_idx / group_means / ws or a ws that is not 16-byte aligned) and launches nothing; the *_workspace_bytes call returns the
 * same negative code.  group_table and src_idx are DEVICE arrays (the call enqueues on `stream` and never synchronises, so it
 * cannot read them): an index outside [0, n_tables) / [0, n_rows) is never dereferenced and makes the affected terms and the
 * group's mean NaN, as dib_mi_sandwich_batched does.  sample_terms [n_groups][n_samples] and u_out [n_groups][n_samples][E]
 * are optional (NULL).  ws: dib_mi_monte_carlo_workspace_bytes, 16-byte aligned, needs no initialisation.  No allocation.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_MI_CHANNEL_H
#define DIB_MI_CHANNEL_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t dib_mi_monte_carlo_workspace_bytes(int n_tables, int n_rows, int E, int n_groups, int n_samples);
int dib_mi_monte_carlo(const float* enc_tables, int n_tables, int n_rows, int E, const int32_t* group_table,
                       const int32_t* src_idx, int n_groups, int n_samples, uint64_t seed, uint32_t step0, double* group_means,
                       double* sample_terms, double* u_out, void* ws, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_MI_CHANNEL_H */
