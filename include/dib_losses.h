/* dib_losses.h - C ABI of the Keras loss and metric family of DistributedIBNet.compile beyond the four kinds of dib_hip.h
 * (DIB_LOSS_BCE_LOGITS, _BCE, _SPARSE_CCE_LOGITS, _MSE through dib_loss_fwd_bwd, which does not change).
 *
 * Every loss is the mean over the batch of a per-row value.  eps = 1e-7, e = p - y, C = out_dim, p = the model output (after
 * its output activation), y = the label row.  `param` is delta (Huber) or label_smoothing s (the cross-entropies), else 0.
 *   DIB_LOSS_BCE_LOGITS   y <- y(1 - s) + s/2;  mean_k [max(z,0) - z y + log1p(exp(-|z|))]
 *   DIB_LOSS_BCE          y <- y(1 - s) + s/2;  c = clip(p, eps, 1 - eps);  mean_k -[y log c + (1 - y) log(1 - c)]
 *   DIB_LOSS_MSE          mean_k e_k^2
 *   DIB_LOSS_MAE          mean_k |e_k|                                      gradient 0 at e = 0
 *   DIB_LOSS_MAPE         100 mean_k |e_k| / max(|y_k|, eps)
 *   DIB_LOSS_MSLE         mean_k (log(max(p_k, eps) + 1) - log(max(y_k, eps) + 1))^2          no gradient where p_k < eps
 *   DIB_LOSS_HUBER        mean_k (|e_k| <= delta ? e_k^2 / 2 : delta |e_k| - delta^2 / 2)
 *   DIB_LOSS_LOGCOSH      mean_k (e_k + softplus(-2 e_k) - log 2)           gradient tanh(e_k)
 *   DIB_LOSS_POISSON      mean_k (p_k - y_k log(p_k + eps))
 *   DIB_LOSS_KLD          sum_k y'_k log(y'_k / p'_k), y' and p' clipped to [eps, 1]          no gradient outside the clip range
 *   DIB_LOSS_COSINE       -sum_k yhat_k phat_k, xhat = x rsqrt(max(sum x^2, 1e-12))
 *   DIB_LOSS_CCE_LOGITS   y <- y(1 - s) + s/C;  lse(z) sum_k y_k - sum_k y_k z_k     gradient softmax(z) sum_k y_k - y
 *                                                                                      (= softmax(z) - y: the labels sum to 1)
 *   DIB_LOSS_CCE          y <- y(1 - s) + s/C;  q = p / sum p;  c = clip(q, eps, 1 - eps);  -sum_k y_k log c_k
 *                         the gradient goes through the normalisation and is zero where q_k is clipped
 *   DIB_LOSS_SPARSE_CCE   label = (int)y[0];  c = clip(p, eps, 1 - eps);  log sum_k c_k - log c_label
 *                         (a label outside [0, C) is clamped into it: the kernel reads nothing out of bounds)
 * Metrics, each a per-row value whose batch sum lands in the metric slot (ws[STEP_OUT][F + 1]); they read the labels as given,
 * before any smoothing:
 *   DIB_METRIC_NONE 0;  DIB_METRIC_BINARY_ACCURACY mean_k [(p_k > 0.5) == y_k];  DIB_METRIC_CATEGORICAL_ACCURACY
 *   [argmax p == argmax y];  DIB_METRIC_SPARSE_CATEGORICAL_ACCURACY [argmax p == (int)y[0]];  DIB_METRIC_MAE mean_k |e_k|;
 *   DIB_METRIC_MSE mean_k e_k^2 (arg-max takes the first of equal maxima).
 * DIB_LOSS_SPARSE_CCE reads ONE label column: it takes DIB_METRIC_NONE or _SPARSE_CATEGORICAL_ACCURACY; every other kind reads
 * out_dim label columns and takes every metric but that one.
 *
 * dib_loss_ex_supported is host-only (callable without a GPU): 1 or 0.
 * dib_loss_rows_ex is the raw form on caller buffers: pred [batch, out_dim] dense, label row of batch position b at
 * y + (row_idx ? row_idx[b] : row0 + b) * ldy, g_pred [batch, out_dim] = dL/dpred * inv_bg * act'(out_act; pred),
 * partial [2 * ceil(batch / 256)]: partial[2 blk] = the loss sum and partial[2 blk + 1] = the metric sum of rows
 * [256 blk, 256 blk + 256).  One launch.
 * dib_loss_fwd_bwd_ex is dib_loss_fwd_bwd for a descriptor: ws[PRED] -> ws[G_PRED], the same partial and ws[STEP_OUT] slots, so
 * dib_backward and dib_step_tail(DIB_TAIL_LOSS) follow it unchanged; flags: DIB_HEAD_DEFER_SUMS.
 *
 * Every reduction runs in a fixed order: the bits of a row do not depend on the batch, the grid or the buffer's address.
 * Every entry returns int, never allocates, never synchronises, reads nothing from the environment and can be captured into a
 * hipGraph.  DIB_E_ARG: a NULL descriptor / buffer, batch <= 0, out_dim <= 0, ldy smaller than the label columns the kind
 * reads; DIB_E_UNSUPPORTED: !dib_loss_ex_supported.  A refused call launches nothing and writes nothing.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_LOSSES_H
#define DIB_LOSSES_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kinds 0, 1 and 3 are dib_hip.h's DIB_LOSS_BCE_LOGITS, DIB_LOSS_BCE and DIB_LOSS_MSE; 2 stays with dib_loss_fwd_bwd */
#define DIB_LOSS_MAE 4
#define DIB_LOSS_MAPE 5
#define DIB_LOSS_MSLE 6
#define DIB_LOSS_HUBER 7
#define DIB_LOSS_LOGCOSH 8
#define DIB_LOSS_POISSON 9
#define DIB_LOSS_KLD 10
#define DIB_LOSS_COSINE 11
#define DIB_LOSS_CCE_LOGITS 12
#define DIB_LOSS_CCE 13
#define DIB_LOSS_SPARSE_CCE 14

#define DIB_METRIC_NONE 0
#define DIB_METRIC_BINARY_ACCURACY 1
#define DIB_METRIC_CATEGORICAL_ACCURACY 2
#define DIB_METRIC_SPARSE_CATEGORICAL_ACCURACY 3
#define DIB_METRIC_MAE 4
#define DIB_METRIC_MSE 5

typedef struct dib_loss_desc {
  int32_t kind;    /* DIB_LOSS_* */
  int32_t metric;  /* DIB_METRIC_* */
  float param;     /* Huber: delta > 0; the cross-entropies: label_smoothing in [0, 1]; else 0 */
} dib_loss_desc;

int dib_loss_ex_supported(const dib_loss_desc* desc, int out_dim);
/* lanes that share a row for this out_dim (1, 4, 16 or 64); host-only */
int dib_loss_ex_lanes(int out_dim);
int dib_loss_rows_ex(const dib_loss_desc* desc, const float* pred, int out_dim, const float* y, int64_t ldy,
                     const int32_t* row_idx, int64_t row0, int batch, float inv_bg, int out_act, float* g_pred, float* partial,
                     dib_stream_t stream);
int dib_loss_fwd_bwd_ex(dib_layout* layout, const dib_loss_desc* desc, const float* y, int64_t ldy, const int32_t* row_idx,
                        int64_t row0, int batch, float inv_bg, int flags, void* ws, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_LOSSES_H */
