/* dib_compression.h - C ABI of the compression-scheme matrices of a DistributedIBNet in one evaluation: for EVERY feature the
 * matrix exp(-Bhattacharyya distance) between the Gaussians its encoder assigns to a display sample of its values (reference
 * visualization.py:14-81, utils.py:177-212; README "confusion matrices"), from the feature-major encoding that one
 * dib_encoder_bank_fwd(DIB_FWD_DETERMINISTIC | DIB_FWD_INFERENCE) leaves in DIB_WS_ENC_OUT - instead of one
 * dib_encode_deterministic + dib_bhattacharyya + two read-backs per feature.
 *
 * dib_compression_gather builds the input of that one forward.  Feature f is displayed on ITS OWN rows rows[f][0..n_max) of the
 * dataset matrix x [n_rows][ldx] (rows is a device table [F][n_max], int32):
 *   xg[i][cols_f] = x[rows[f][i]][cols_f]      for every feature f of the layout's column table (ragged d_f), i < n_max
 * so xg [n_max][sum_d] (dense, leading dimension sum_d) carries in row i the i-th display value of every feature and a forward
 * of n_max rows encodes each feature on exactly its rows (not F n_max rows through all F encoders).  One launch.  The kernel
 * clamps every index into [0, n_rows): a bad table reads a wrong row, never out of bounds.  The layout's tables must have been
 * uploaded (dib_layout_upload_tables).
 *
 * dib_compression_matrices: enc [F][plane_rows][2E] (fp32, mu | logvar) is feature-major; feature f's sample is the rows
 * row0 + i, i < counts[f], of plane f (counts is a device array [F], int32, clamped to [0, n_max]).  For i, j < counts[f]
 *   dist[f][i][j] = 1/8 sum_e (mu_ie - mu_je)^2 / s_e + 1/2 sum_e (ln s_e - (lv_ie + lv_je) / 2),   s_e = (e^lv_ie + e^lv_je) / 2
 *   comp[f][i][j] = exp(-dist[f][i][j])
 * (the closed form of dib_bhattacharyya) and every other entry of the [F][n_max][n_max] outputs is written as exactly 0.0f.
 * dist and comp are optional (NULL), at least one must be given.  fp32 throughout; exp(logvar) is taken once per staged row
 * element, not per pair, and the logvar that enters the second sum is the logarithm of that rounded variance: a row against
 * itself or a duplicate of it is at distance exactly 0.0f (comp exactly 1.0f).  Every (f, i, j) sums over e = 0 .. E-1 in that
 * order in one accumulator per sum, with operations that commute in (i, j): the matrices equal their transposes bit for bit, and
 * the bits of a feature's matrix depend on (E, its rows) alone - not on F, its plane index, n_max, row0 or the features that
 * share the launch.  One launch whatever F is.
 *
 * Envelope (DIB_COMPRESSION_*): 1 <= E <= 256, 1 <= n_max <= 2048 (528 tile pairs of 64 x 64), 1 <= F <= 65535 (the grid's second
 * dimension).  Outside it dib_compression_supported returns 0 and the two calls return DIB_E_UNSUPPORTED; DIB_E_ARG for a NULL
 * layout / x / rows / xg / enc / counts, a non-positive size, ldx < sum_d, a layout without uploaded tables, dist and comp both
 * NULL, row0 < 0 or row0 + n_max > plane_rows.  A refused call launches nothing and writes nothing.  dib_compression_supported
 * is host-only (callable without a GPU).  The calls enqueue on `stream`, never allocate and never synchronise: they can be
 * captured into a hipGraph.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_COMPRESSION_H
#define DIB_COMPRESSION_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_COMPRESSION_MAX_E 256
#define DIB_COMPRESSION_MAX_ROWS 2048
#define DIB_COMPRESSION_MAX_F 65535

int dib_compression_supported(int F, int E, int n_max);
int dib_compression_gather(dib_layout* l, const float* x, int64_t ldx, int64_t n_rows, const int32_t* rows, int n_max,
                           float* xg, dib_stream_t stream);
int dib_compression_matrices(const float* enc, int64_t plane_rows, int64_t row0, int F, int E, const int32_t* counts, int n_max,
                             float* dist, float* comp, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_COMPRESSION_H */
