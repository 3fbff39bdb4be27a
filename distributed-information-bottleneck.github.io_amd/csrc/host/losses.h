// host/losses.h - the Keras loss and metric family (include/dib_losses.h, csrc/dib_losses.h): the argument checks (losses_desc.h)
// and the one launch of dib_loss_ex_kernel<KIND, LANES>, on caller buffers (dib_loss_rows_ex) or on the workspace slots of
// dib_loss_fwd_bwd (dib_loss_fwd_bwd_ex).
#include "losses_desc.h"

namespace {

template <int KIND>
void loss_ex_launch_lanes(int lanes, dim3 grid, hipStream_t st, int metric, float prm, const float* pred, int C, const float* y,
                          long long ldy, const int* row_idx, long long row0, int batch, float inv_bg, int out_act, float* g_pred,
                          float* partial) {
#define DIB_LOSS_EX(L) DIB_LAUNCH((dib_loss_ex_kernel<KIND, L>), grid, dim3(256), 0, st, metric, prm, pred, C, y, ldy, row_idx, row0, \
                                  batch, inv_bg, out_act, g_pred, partial)
  switch (lanes) {
    case 1: DIB_LOSS_EX(1); break;
    case 4: DIB_LOSS_EX(4); break;
    case 16: DIB_LOSS_EX(16); break;
    default: DIB_LOSS_EX(64); break;
  }
#undef DIB_LOSS_EX
}

// every check of a call, then the launch: a refused call has launched and written nothing
int loss_ex_launch(const dib_loss_desc* d, const float* pred, int C, const float* y, int64_t ldy, const int32_t* row_idx,
                   int64_t row0, int batch, float inv_bg, int out_act, float* g_pred, float* partial, hipStream_t st) {
  if (!d || !pred || !y || !g_pred || !partial || batch <= 0 || C <= 0) return DIB_E_ARG;
  if (!dib_loss_desc_supported(d, C)) return DIB_E_UNSUPPORTED;
  if (ldy < dib_loss_desc_label_columns(d->kind, C) || (!row_idx && row0 < 0)) return DIB_E_ARG;
  if (out_act < DIB_ACT_LINEAR || out_act > DIB_ACT_LEAKY_RELU_01) return DIB_E_ARG;
  const int lanes = dib_loss_desc_lanes(C);
  const dim3 grid((batch + 255) / 256);
  ProfScope ps(kProfOther, st);
#define DIB_LOSS_KIND(K) case K: loss_ex_launch_lanes<K>(lanes, grid, st, d->metric, d->param, pred, C, y, (long long)ldy,      \
                                                         (const int*)row_idx, (long long)row0, batch, inv_bg, out_act, g_pred, \
                                                         partial); break
  switch (d->kind) {
    DIB_LOSS_KIND(DIB_LOSS_BCE_LOGITS); DIB_LOSS_KIND(DIB_LOSS_BCE); DIB_LOSS_KIND(DIB_LOSS_MSE); DIB_LOSS_KIND(DIB_LOSS_MAE);
    DIB_LOSS_KIND(DIB_LOSS_MAPE); DIB_LOSS_KIND(DIB_LOSS_MSLE); DIB_LOSS_KIND(DIB_LOSS_HUBER); DIB_LOSS_KIND(DIB_LOSS_LOGCOSH);
    DIB_LOSS_KIND(DIB_LOSS_POISSON); DIB_LOSS_KIND(DIB_LOSS_KLD); DIB_LOSS_KIND(DIB_LOSS_COSINE);
    DIB_LOSS_KIND(DIB_LOSS_CCE_LOGITS); DIB_LOSS_KIND(DIB_LOSS_CCE); DIB_LOSS_KIND(DIB_LOSS_SPARSE_CCE);
    default: return DIB_E_UNSUPPORTED;
  }
#undef DIB_LOSS_KIND
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int dib_loss_ex_supported(const dib_loss_desc* desc, int out_dim) { return dib_loss_desc_supported(desc, out_dim); }

int dib_loss_ex_lanes(int out_dim) { return out_dim <= 0 ? DIB_E_ARG : dib_loss_desc_lanes(out_dim); }

int dib_loss_rows_ex(const dib_loss_desc* desc, const float* pred, int out_dim, const float* y, int64_t ldy,
                     const int32_t* row_idx, int64_t row0, int batch, float inv_bg, int out_act, float* g_pred, float* partial,
                     dib_stream_t stream) {
  return loss_ex_launch(desc, pred, out_dim, y, ldy, row_idx, row0, batch, inv_bg, out_act, g_pred, partial, (hipStream_t)stream);
}

int dib_loss_fwd_bwd_ex(dib_layout* l, const dib_loss_desc* desc, const float* y, int64_t ldy, const int32_t* row_idx,
                        int64_t row0, int batch, float inv_bg, int flags, void* ws, dib_stream_t stream) {
  if (!l || !ws || batch <= 0) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  if (int rc = loss_ex_launch(desc, w + m.pred, l->out_dim, y, ldy, row_idx, row0, batch, inv_bg, l->out_act, w + m.g_pred,
                              w + m.loss_partial, st))
    return rc;
  if (flags & DIB_HEAD_DEFER_SUMS) return DIB_OK;   // dib_step_tail(DIB_TAIL_LOSS) sums the partials
  ProfScope ps(kProfOther, st);
  DIB_LAUNCH(dib_loss_finalize_kernel, dim3(2), dim3(256), 0, st, (const float*)(w + m.loss_partial), m.loss_blocks, (float)batch,
             w + m.step_out + l->F);
  return (int)hipGetLastError();
}

}  // extern "C"
