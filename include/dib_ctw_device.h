/* dib_ctw_device.h - C ABI of the context-tree-weighting (CTW) entropy-rate estimator on the device: the tree of
 * include/dib_ctw.h (reference chaos/cppctw.cpp) built level by level, all positions of all windows in parallel
 * (csrc/dib_ctw_levels.h; DESIGN.md "CTW on the device").
 *
 * Windows: window w is symbols[starts[w] .. starts[w] + lengths[w]) of ONE device-resident uint8 array of n_symbols symbols over
 * {0 .. alphabet_size - 1}; windows may overlap or coincide and are never copied.  starts / lengths are HOST arrays of n_windows
 * int64, read during the call.  Outputs, device arrays of n_windows entries each:
 *   code_bits  float64  L_w(root) in bits, unrounded
 *   rates      float64  (float)(L_w(root) / length): rounded through float32 as the host estimator's; NaN for an empty window
 *   nodes      int64    nodes of the tree, root included, as dib_ctw_node_count counts them
 *   status     int32    0 = ok, else a sum of DIB_CTW_DEVICE_DEEP (at level 512 a group of >= 2 positions still has a member with
 *                       more context: beyond that depth the host's tree depends on the order of insertion and the level build does
 *                       not reproduce it - the flag is conservative), DIB_CTW_DEVICE_OVERFLOW (the tree needed more than
 *                       node_capacity nodes while this window was still growing) and DIB_CTW_DEVICE_BAD_SYMBOL (a symbol >=
 *                       alphabet_size).  The other outputs of a window whose status is not 0 are not results.
 * node_capacity counts the nodes with at least two positions (and one root per window) over all windows of the call: the others
 * are leaves and cost no memory.  A chaotic sequence needs about 1.5 per symbol, a periodic one more.
 * The doubles are functions of integer counts alone: the same call gives the same bits twice, and a window gives the same bits
 * in whichever call, with whichever other windows, it is computed.  lgamma comes from a table the host fills with its libm below
 * 65 536 and from the device's lgamma beyond; log2 / exp2 in the mixture are the device's, so code_bits agrees with the host's
 * unrounded value to a few units in the last place and rates with the host's float32 value or one of its neighbours.
 *
 * dib_ctw_device_estimate enqueues on `stream`, allocates nothing and reads nothing from the environment.  It waits for the
 * stream once per level of the tree (at most 513 times) to learn how many positions still move; it is therefore not capturable
 * into a hipGraph.  info (HOST, may be NULL) receives the size of the work; with info the call also waits for its last kernel,
 * to time the bottom-up pass.
 *
 * Envelope: 1 <= alphabet_size <= 16, lengths >= 0, the sum of the lengths of one call < 2^31.  Outside it
 * dib_ctw_device_supported returns 0, dib_ctw_device_workspace_bytes -1 and the call DIB_E_UNSUPPORTED; DIB_E_ARG for a NULL
 * pointer, a negative start or length, a window that leaves the array or node_capacity outside [max(n_windows, 1), 2^31);
 * DIB_E_WORKSPACE for ws_bytes below dib_ctw_device_workspace_bytes.  A refused call launches nothing and writes nothing.
 * dib_ctw_device_supported and the workspace query are host-only (callable without a GPU).
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_CTW_DEVICE_H
#define DIB_CTW_DEVICE_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_CTW_DEVICE_MAX_ALPHABET 16
#define DIB_CTW_DEVICE_MAX_SYMBOLS 2147483647LL
#define DIB_CTW_DEVICE_DEEP 1
#define DIB_CTW_DEVICE_OVERFLOW 2
#define DIB_CTW_DEVICE_BAD_SYMBOL 4

typedef struct dib_ctw_device_info {
  int32_t levels;          /* levels of the tree built, the root's included */
  int32_t reserved;
  int64_t element_steps;   /* the sum over the levels of the positions on the level's list */
  int64_t big_nodes;       /* nodes that took an entry of node_capacity */
  double level_seconds;    /* host clock: the loop over levels (it ends on a wait) */
  double mix_seconds;      /* host clock: the bottom-up pass and the outputs */
} dib_ctw_device_info;

int dib_ctw_device_supported(int alphabet_size, int64_t total_window_symbols, int n_windows);
int64_t dib_ctw_device_workspace_bytes(int64_t total_window_symbols, int n_windows, int alphabet_size, int64_t node_capacity);
int dib_ctw_device_estimate(const uint8_t* symbols, int64_t n_symbols, const int64_t* starts, const int64_t* lengths, int n_windows,
                            int alphabet_size, int64_t node_capacity, double* code_bits, double* rates, int64_t* nodes,
                            int32_t* status, void* ws, int64_t ws_bytes, dib_ctw_device_info* info, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_CTW_DEVICE_H */
