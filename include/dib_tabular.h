/* dib_tabular.h - C ABI of the tabular front end: the quantile transform of the reference's preprocessor (reference
 * data.py:178-297, sklearn's QuantileTransformer(output_distribution='normal' | 'uniform').transform) on a table that is
 * already on the device, in one launch.
 *
 * dib_quantile_transform: x [n_rows][ldx] (fp32, row-major), out [n_rows][ldo] (fp32).  quantiles is [n_cols][n_quantiles]
 * (fp64, each COLUMN's table contiguous - the transpose of sklearn's quantiles_), references [n_quantiles] (fp64), both on the
 * device; references is read from the passed table and never recomputed.  Per element (row r, column c), in float64 from the
 * exactly widened float32 input, with q = the table of column c, last = n_quantiles - 1:
 *   a = interp(x, q, ref),  b = interp(-x, -reverse(q), -reverse(ref)),  u = 0.5 (a - b)
 *   interp = np.interp: below the first knot the first value, at or above the last knot the last value; j the largest index with
 *     xp[j] <= x; x == xp[j] gives fp[j]; else slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]), slope (x - xp[j]) + fp[j] with
 *     each operation rounded on its own (no FMA) and NumPy's two NaN fall-backs
 *   normal (distribution 0):  x + 1e-7 > q[last] gives u = 1; then x - 1e-7 < q[0] gives u = 0 (the lower bound is applied last);
 *     then u is clipped to [1e-7 - 2^-52, 1 - (1e-7 - 2^-52)];  out = (float) ndtri(u), ndtri = Wichura's AS 241 PPND16
 *   uniform (distribution 1): x == q[last] gives u = 1; then x == q[0] gives u = 0;  out = (float) u
 * NaN stays NaN; +-inf take the bounds.  Clipping u before the inverse CDF equals sklearn's clip after it (the inverse CDF is
 * monotone) and keeps infinities out.  u64 (optional, NULL to skip) [n_rows][n_cols] dense receives u as it enters the inverse
 * CDF (after the bounds and the clip): the float64 quantity NumPy computes, bit for bit.
 * An element's result depends on its value and its column's table alone - not on n_rows, its row, the column's position, the
 * columns that share the launch, the grid, or whether the call stages the tables in LDS (it does from 4 n_quantiles rows on
 * while one column's table fits 64 KB, n_quantiles <= 8192; smaller and larger tables are searched in global memory).  No
 * atomics, no scratch.  One launch per call.
 *
 * Envelope (DIB_TABULAR_*): 2 <= n_quantiles <= 10 000 (sklearn's own cap is the subsample size), 1 <= n_cols <= 65 535,
 * n_rows >= 1, distribution 0 or 1.  Outside it dib_quantile_supported returns 0 and the call returns DIB_E_UNSUPPORTED;
 * DIB_E_ARG for a NULL x / quantiles / references / out, ldx < n_cols, ldo < n_cols or a non-positive size.  A refused call
 * launches nothing and writes nothing.  dib_quantile_supported is host-only (callable without a GPU).  The call enqueues on
 * `stream`, never allocates and never synchronises: it can be captured into a hipGraph.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_TABULAR_H
#define DIB_TABULAR_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_TABULAR_MIN_QUANTILES 2
#define DIB_TABULAR_MAX_QUANTILES 10000
#define DIB_TABULAR_MAX_COLS 65535
#define DIB_TABULAR_NORMAL 0
#define DIB_TABULAR_UNIFORM 1

int dib_quantile_supported(int n_quantiles, int n_cols, int distribution);
int dib_quantile_transform(const float* x, int64_t ldx, int64_t n_rows, int n_cols, const double* quantiles,
                           const double* references, int n_quantiles, int distribution, float* out, int64_t ldo, double* u64,
                           dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_TABULAR_H */
