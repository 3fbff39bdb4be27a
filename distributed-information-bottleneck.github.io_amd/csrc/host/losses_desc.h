// host/losses_desc.h - the host half of include/dib_losses.h that needs no device: which (kind, metric, param, out_dim) the
// family takes, how many label columns a kind reads and how many lanes share a row.  Plain C++ on include/dib_losses.h alone, so
// that a stand-alone CPU program can run it under the sanitizers.
#pragma once
#include "../../../include/dib_losses.h"

inline bool dib_loss_desc_kind_known(int kind) {
  return kind == DIB_LOSS_BCE_LOGITS || kind == DIB_LOSS_BCE || kind == DIB_LOSS_MSE || (kind >= DIB_LOSS_MAE && kind <= DIB_LOSS_SPARSE_CCE);
}

inline bool dib_loss_desc_takes_smoothing(int kind) {
  return kind == DIB_LOSS_BCE_LOGITS || kind == DIB_LOSS_BCE || kind == DIB_LOSS_CCE_LOGITS || kind == DIB_LOSS_CCE;
}

// label columns the kernel reads of a row of y
inline int dib_loss_desc_label_columns(int kind, int out_dim) { return kind == DIB_LOSS_SPARSE_CCE ? 1 : out_dim; }

inline int dib_loss_desc_lanes(int out_dim) { return out_dim <= 1 ? 1 : out_dim <= 4 ? 4 : out_dim <= 16 ? 16 : 64; }

inline int dib_loss_desc_supported(const dib_loss_desc* d, int out_dim) {
  if (!d || out_dim <= 0) return 0;
  if (!dib_loss_desc_kind_known(d->kind)) return 0;
  if (d->metric < DIB_METRIC_NONE || d->metric > DIB_METRIC_MSE) return 0;
  const bool sparse_metric = d->metric == DIB_METRIC_SPARSE_CATEGORICAL_ACCURACY;
  if (d->kind == DIB_LOSS_SPARSE_CCE ? !(sparse_metric || d->metric == DIB_METRIC_NONE) : sparse_metric) return 0;
  const float p = d->param;
  if (!(p == p)) return 0;                                            // NaN
  if (d->kind == DIB_LOSS_HUBER) return (p > 0.f && p <= 3.0e38f) ? 1 : 0;
  if (dib_loss_desc_takes_smoothing(d->kind)) return (p >= 0.f && p <= 1.f) ? 1 : 0;
  return p == 0.f ? 1 : 0;
}
