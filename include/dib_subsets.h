/* dib_subsets.h - C ABI of the exhaustive subset informations: I(X_S;Y) in bits for EVERY subset S of the features of a small
 * discrete table, from its joint counts, in one launch (the ground truth the Boolean-circuit notebook compares the Distributed
 * IB against: reference complex_systems/InfoDecomp_Boolean_circuits.ipynb cells 7 and 10, `all_mis`).
 *
 * counts [2^B][K] (int32, device): counts[key][k] = the number of rows of the table with that key and class k.  The key of a row
 * is its features' bit fields concatenated, feature 0 lowest: feature f is feature_bits[f] >= 1 bits wide (feature_bits is a HOST
 * array of F ints, read during the call), B = sum_f feature_bits[f].  N = the sum of all counts, N < 2^31.
 * For a subset S (mask: bit f set when feature f is in S), with c[a][k] = the sum of counts over the keys that agree with
 * pattern a on the bits of S, c[a] = sum_k c[a][k], n_k = sum_key counts[key][k] and xlog2(c) = c log2(c), xlog2(0) = 0:
 *     E[S]  = sum_a xlog2(c[a]) - sum_{a,k} xlog2(c[a][k])
 *     H(Y)  = ( xlog2(N) - sum_k xlog2(n_k) ) / N
 *     I(X_S;Y) = H(Y) - E[S] / N,      I of the empty subset = 0.0 exactly
 * out_bits [n_masks] (float64, device) receives I of the subsets mask0 .. mask0 + n_masks - 1.  Float64 accumulation in a fixed
 * order; a power of two's logarithm is its exponent, so tables whose counts are all powers of two (a parity, y = x_j on a full
 * cube) give their exact answers.  The bits of out_bits[S - mask0] depend on (counts, feature_bits, S) and the tuning key below
 * alone - not on mask0 / n_masks (a table may be computed in chunks), the grid or an address.  No atomics.  One launch per call.
 *
 * dib_subset_information_workspace_bytes: bytes of `ws` the call needs for these sizes, -1 outside the envelope.  The present
 * kernel needs none (0; ws may then be NULL) - callers that honour the query stay correct if a later one does.
 * dib_set_tuning("subset_low_bits", L) (dib_hip.h): the number of low key bits a workgroup folds in LDS; 0 (default) = the most
 * that fits (8 for K <= 2, 7 for K <= 6, 6 beyond), otherwise clipped to [1, that].  Another L is another order of the float64
 * sums over the high bits' patterns (csrc/dib_subsets.h).
 *
 * Envelope: 1 <= F <= B <= 20, 1 <= K <= 16.  Outside it dib_subset_information_supported returns 0 and the call returns
 * DIB_E_UNSUPPORTED; DIB_E_ARG for a NULL counts / feature_bits / out_bits, a feature_bits entry < 1, sum feature_bits != B,
 * mask0 < 0, n_masks < 1 or mask0 + n_masks > 2^F.  A refused call launches nothing and writes nothing.
 * dib_subset_information_supported and the workspace query are host-only (callable without a GPU).  The call enqueues on
 * `stream`, never allocates, never synchronises and reads nothing from the environment: it can be captured into a hipGraph.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_SUBSETS_H
#define DIB_SUBSETS_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_SUBSET_MAX_BITS 20
#define DIB_SUBSET_MAX_CLASSES 16

int dib_subset_information_supported(int B, int F, int K);
int64_t dib_subset_information_workspace_bytes(int B, int K);
int dib_subset_information(const int32_t* counts, int B, int K, const int* feature_bits, int F, int mask0, int n_masks,
                           double* out_bits, void* ws, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_SUBSETS_H */
