// host/step.h - the launch sequences of a training step (include/dib_hip.h): integration network forward / loss / backward, the
// fused output head, gradient finalize, metrics, the one-launch step tail, optimizers and the evaluation helpers.

static int integration_fwd_impl(dib_layout* l, int batch, const float* params, void* ws, dib_stream_t stream,
                                bool with_output_layer) {
  if (!l || !params || !ws || batch <= 0) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  const int LI = l->n_int + 1;
  int first = 0;
  if (use_small_int(l, batch)) {   // the hidden layers (and a general output layer of width % 16 == 0) in one launch
    const bool out_too = with_output_layer && l->out_dim % 16 == 0;
    int rc = small_integration(l, m, w, batch, params, DIB_SMALL_INT_FWD | (out_too ? DIB_SMALL_INT_OUT : 0), 0, nullptr, 0,
                               nullptr, 0, 0.f, st);
    if (rc || out_too || !with_output_layer) return rc;
    first = LI - 1;   // the narrow output layer below
  }
  for (int ly = first; ly < LI; ++ly) {
    if (ly == LI - 1 && !with_output_layer) break;
    const float* A = ly == 0 ? w + m.U : w + m.int_h[ly - 1];
    float* C = ly == LI - 1 ? w + m.pred : w + m.int_h[ly];
    const int act = ly == LI - 1 ? l->out_act : l->act;  // reference models.py:82-83
    int rc;
    if (ly == LI - 1 && l->out_dim <= DIB_SKINNY_MAX) {  // 1-unit logit & co: HBM-bound stream, not an MFMA tile
      const int win = ly == 0 ? l->F * l->E : l->int_width[ly - 1];
      ProfScope ps(kProfOther, st);
      DIB_LAUNCH(dib_skinny_fwd_kernel, dim3(grid_for((int64_t)batch * 64, 256, 2048)), dim3(256), 0, st, A, batch,
                         win, params + l->int_w_off[ly], params + l->int_b_off[ly], l->out_dim, act, C);
      rc = (int)hipGetLastError();
    } else {
      rc = launch_gemm<0>(l, l->int_fwd[ly], A, params, C, params, nullptr, nullptr, batch, act, 1, 0, 0, st);
    }
    if (rc) return rc;
  }
  return DIB_OK;
}

static int integration_bwd_impl(dib_layout* l, int batch, const float* params, float* grads, void* ws, dib_stream_t stream,
                                bool with_output_layer, bool skip_dgrad = false) {
  if (!l || !params || !grads || !ws || batch <= 0) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  float* gt = wgrad_target(m, w, grads);
  const long long sstride = align_up(l->n_params, 4);
  const int LI = l->n_int + 1;
  // small batches: the whole dgrad chain dL/dpred (or the head's dL/dh) -> dL/du in one launch; the weight gradients below
  if (!skip_dgrad && use_small_int(l, batch) && (!with_output_layer || l->out_dim % 16 == 0)) {
    int rc = small_integration(l, m, w, batch, params, DIB_SMALL_INT_LOAD_H | DIB_SMALL_INT_BWD |
                               (with_output_layer ? DIB_SMALL_INT_BWD_OUT : DIB_SMALL_INT_LOAD_G), 0, nullptr, 0, nullptr, 0, 0.f, st);
    if (rc) return rc;
    skip_dgrad = true;
  }
  for (int ly = LI - 1; ly >= 0; --ly) {
    if (ly == LI - 1 && !with_output_layer) continue;  // done by dib_output_head_fused
    const float* gout = ly == LI - 1 ? w + m.g_pred : w + m.g_int_h[ly];
    const float* hin = ly == 0 ? w + m.U : w + m.int_h[ly - 1];
    float* gin = ly == 0 ? w + m.g_u : w + m.g_int_h[ly - 1];
    int rc;
    if (ly == LI - 1 && l->out_dim <= DIB_SKINNY_MAX) {
      const int win = ly == 0 ? l->F * l->E : l->int_width[ly - 1];
      ProfScope ps(kProfOther, st);
      // stage 1 per row chunk, stage 2 into slab 0 (the other slabs of this block stay zero), both fixed-order
      DIB_LAUNCH(dib_skinny_wgrad_kernel, dim3(m.skinny_chunks), dim3(256), 0, st, hin, gout, batch, win, l->out_dim,
                         m.skinny_rows, w + m.skinny_partial);
      DIB_LAUNCH(dib_skinny_wgrad_reduce_kernel, dim3(win * l->out_dim + l->out_dim), dim3(256),
                         0, st, (const float*)(w + m.skinny_partial), m.skinny_chunks, win, l->out_dim,
                         gt + l->int_w_off[ly], gt + l->int_b_off[ly]);
      DIB_LAUNCH(dib_skinny_dgrad_kernel, dim3(grid_for((int64_t)batch * win)), dim3(256), 0, st, gout, batch, win,
                         params + l->int_w_off[ly], l->out_dim, ly == 0 ? (const float*)nullptr : hin, ly == 0 ? 0 : l->act,
                         gin);
      rc = (int)hipGetLastError();
      if (rc) return rc;
      continue;
    }
    rc = launch_gemm<2>(l, l->int_wgrad[ly], hin, gout, gt, nullptr, nullptr, gt, batch, 0, m.nsplit,
                        m.rows_per_split, sstride, st, m.nsplit);
    if (rc) return rc;
    if (skip_dgrad) continue;   // the small-batch kernel already ran the dgrad chain
    // u is not an activation output (no mask for ly == 0)
    rc = launch_gemm<1>(l, l->int_dgrad[ly], gout, params, gin, nullptr, ly == 0 ? nullptr : hin, nullptr, batch,
                        ly == 0 ? 0 : l->act, 1, 0, 0, st);
    if (rc) return rc;
  }
  return DIB_OK;
}

extern "C" {

int dib_integration_fwd(dib_layout* l, int batch, const float* params, void* ws, dib_stream_t stream) {
  return integration_fwd_impl(l, batch, params, ws, stream, true);
}

int dib_integration_fwd_hidden(dib_layout* l, int batch, const float* params, void* ws, dib_stream_t stream) {
  return integration_fwd_impl(l, batch, params, ws, stream, false);
}

// ---- loss + backward ----------------------------------------------------------------------------
int dib_loss_fwd_bwd(dib_layout* l, int loss_kind, const float* y, int64_t ldy, const int32_t* row_idx, int64_t row0,
                     int batch, float inv_global_batch, int flags, void* ws, dib_stream_t stream) {
  if (!l || !y || !ws || batch <= 0) return DIB_E_ARG;
  if (loss_kind < 0 || loss_kind > 3) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_loss_kernel, dim3(m.loss_blocks), dim3(256), 0, st, loss_kind, w + m.pred, l->out_dim, y,
                     (long long)ldy, (const int*)row_idx, (long long)row0, batch, inv_global_batch, l->out_act,
                     w + m.g_pred, w + m.loss_partial); }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  if (flags & DIB_HEAD_DEFER_SUMS) return DIB_OK;   // dib_step_tail(DIB_TAIL_LOSS) sums the partials
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_loss_finalize_kernel, dim3(2), dim3(256), 0, st, (const float*)(w + m.loss_partial), m.loss_blocks,
                     (float)batch, w + m.step_out + l->F); }
  return (int)hipGetLastError();
}

int dib_integration_bwd(dib_layout* l, int batch, const float* params, float* grads, void* ws, dib_stream_t stream) {
  return integration_bwd_impl(l, batch, params, grads, ws, stream, true);
}

int dib_integration_bwd_hidden(dib_layout* l, int batch, const float* params, float* grads, void* ws, dib_stream_t stream) {
  return integration_bwd_impl(l, batch, params, grads, ws, stream, false);
}

// fused 1-unit output head of a training step: supported for out_dim == 1, linear output activation, BCE-from-logits or
// MSE, at least one integration hidden layer whose width is a multiple of 4 and <= 1024
int dib_output_head_fused_supported(const dib_layout* l, int loss_kind) {
  if (!l) return 0;
  if (!knobs().fused_head) return 0;   // dib_set_tuning("fused_head", 0): A/B switch
  if (l->out_dim != 1 || l->out_act != DIB_ACT_LINEAR || l->n_int < 1) return 0;
  if (loss_kind != DIB_LOSS_BCE_LOGITS && loss_kind != DIB_LOSS_MSE) return 0;
  const int K = l->int_width[l->n_int - 1];
  return (K % 4 == 0 && K <= 1024) ? 1 : 0;
}

int dib_output_head_fused(dib_layout* l, int loss_kind, const float* y, int64_t ldy, const int32_t* row_idx, int64_t row0,
                          int batch, float inv_global_batch, int flags, const float* params, float* grads, void* ws,
                          dib_stream_t stream) {
  const bool no_grad = (flags & DIB_HEAD_NO_GRAD) != 0;
  if (!l || !y || !params || (!grads && !no_grad) || !ws || batch <= 0) return DIB_E_ARG;
  if (!dib_output_head_fused_supported(l, loss_kind)) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  float* gt = no_grad ? nullptr : wgrad_target(m, w, grads);
  const int ly = l->n_int, K = l->int_width[ly - 1];
  const int nblk = m.skinny_chunks, rpb = m.skinny_rows;
  const float* A = w + m.int_h[ly - 1];
  {
    ProfScope ps(kProfOther, st);
#define DIB_HEAD(NC) DIB_LAUNCH(dib_head_fused_kernel<NC>, dim3(nblk), dim3(256), 0, st, loss_kind, A, batch, K,      \
                                        params + l->int_w_off[ly], params + l->int_b_off[ly], y, (long long)ldy,                 \
                                        (const int*)row_idx, (long long)row0, inv_global_batch, l->act, rpb, w + m.pred,          \
                                        no_grad ? (float*)nullptr : w + m.g_pred, no_grad ? (float*)nullptr : w + m.g_int_h[ly - 1], \
                                        w + m.skinny_partial, w + m.loss_partial)
    if (K <= 256) DIB_HEAD(1); else if (K <= 512) DIB_HEAD(2); else DIB_HEAD(4);
#undef DIB_HEAD
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    if (flags & DIB_HEAD_DEFER_SUMS) return DIB_OK;   // dib_step_tail(DIB_TAIL_HEAD_WGRAD | DIB_TAIL_LOSS_HEAD) finishes both
    if (!no_grad)
      DIB_LAUNCH(dib_skinny_wgrad_reduce_kernel, dim3(K + 1), dim3(256), 0, st, (const float*)(w + m.skinny_partial), nblk,
                         K, 1, gt + l->int_w_off[ly], gt + l->int_b_off[ly]);
    DIB_LAUNCH(dib_loss_finalize_kernel, dim3(2), dim3(256), 0, st, (const float*)(w + m.loss_partial), nblk, (float)batch,
                       w + m.step_out + l->F);
  }
  return (int)hipGetLastError();
}

// The integration network's whole share of a step with the fused 1-unit head: hidden layers forward, output Dense(1) + loss,
// and (training) the head's backward, the dgrad chain back to dL/du and the hidden layers' weight gradients.
// = dib_integration_fwd_hidden + dib_output_head_fused(flags) + dib_integration_bwd_hidden; in the row-tile regime (small_regime) the
// forward, the head and the dgrad chain are ONE launch of dib_small_integration_kernel (16-row tiles, csrc/dib_small.h).
int dib_integration_head_step(dib_layout* l, int loss_kind, const float* y, int64_t ldy, const int32_t* row_idx, int64_t row0,
                              int batch, float inv_global_batch, int flags, const float* params, float* grads, void* ws,
                              dib_stream_t stream) {
  const bool no_grad = (flags & DIB_HEAD_NO_GRAD) != 0;
  if (!l || !y || !params || (!grads && !no_grad) || !ws || batch <= 0) return DIB_E_ARG;
  if (!dib_output_head_fused_supported(l, loss_kind)) return DIB_E_UNSUPPORTED;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  int rc;
  if (use_small_int(l, batch)) {
    hipStream_t st = (hipStream_t)stream;
    const auto m = l->map(batch);
    float* w = (float*)ws;
    const int mode = DIB_SMALL_INT_FWD | DIB_SMALL_INT_HEAD |
                     (no_grad ? DIB_SMALL_INT_INFER : (DIB_SMALL_INT_HEAD_GRAD | DIB_SMALL_INT_BWD));
    rc = small_integration(l, m, w, batch, params, mode, loss_kind, y, ldy, row_idx, row0, inv_global_batch, st);
    if (rc) return rc;
    // (DIB_HEAD_DEFER_WGRAD is honoured exactly when dib_backward will run the merged weight-gradient launch: same predicate)
    if (!no_grad && !((flags & DIB_HEAD_DEFER_WGRAD) && use_merged_wgrad(l, batch))) {
      rc = integration_bwd_impl(l, batch, params, grads, ws, stream, false, /*skip_dgrad=*/true);
      if (rc) return rc;
    }
    if (flags & DIB_HEAD_DEFER_SUMS) return DIB_OK;
    const int ly = l->n_int, K = l->int_width[ly - 1];
    ProfScope ps(kProfOther, st);
    if (!no_grad) {
      float* gt = wgrad_target(m, w, grads);
      DIB_LAUNCH(dib_skinny_wgrad_reduce_kernel, dim3(K + 1), dim3(256), 0, st, (const float*)(w + m.skinny_partial),
                         m.skinny_chunks, K, 1, gt + l->int_w_off[ly], gt + l->int_b_off[ly]);
    }
    DIB_LAUNCH(dib_loss_finalize_kernel, dim3(2), dim3(256), 0, st, (const float*)(w + m.loss_partial), m.skinny_chunks,
                       (float)batch, w + m.step_out + l->F);
    return (int)hipGetLastError();
  }
  rc = integration_fwd_impl(l, batch, params, ws, stream, false);
  if (rc) return rc;
  rc = dib_output_head_fused(l, loss_kind, y, ldy, row_idx, row0, batch, inv_global_batch, flags & ~DIB_HEAD_DEFER_WGRAD, params,
                             grads, ws, stream);
  if (rc || no_grad) return rc;
  // (large batches: DIB_HEAD_DEFER_WGRAD is ignored - each layer's weight gradient runs right after its dgrad, while the
  // operands are still in the infinity cache; dib_backward(DIB_BWD_INTEGRATION_DONE) then only runs the encoder bank)
  return integration_bwd_impl(l, batch, params, grads, ws, stream, false);
}

// Everything of a step's backward pass that follows the loss, in one entry (single-GPU callers; the data-parallel bucket
// protocol keeps the separate entries): [dib_integration_bwd unless DIB_BWD_INTEGRATION_DONE] + dib_encoder_bank_bwd, with
// the weight gradients of the integration network's hidden layers that dib_integration_head_step(DIB_HEAD_DEFER_WGRAD) left
// (DIB_BWD_INTEGRATION_DONE).  In the row-tile regime ALL weight gradients of the step - encoder layers 2.., integration
// layers - are ONE grouped launch over the per-batch descriptor table dib_workspace_init wrote into the workspace.
int dib_backward(dib_layout* l, int batch, const float* params, float* grads, const float* beta_dev, float inv_global_batch,
                 int flags, void* ws, dib_stream_t stream) {
  if (!l || !params || !grads || !beta_dev || !ws || batch <= 0) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  const bool int_done = (flags & DIB_BWD_INTEGRATION_DONE) != 0;
  const bool merged = use_merged_wgrad(l, batch) && (int_done || l->out_dim % 16 == 0);
  int rc;
  if (!merged) {
    // (int_done here means dib_integration_head_step already ran the integration network's weight gradients: it defers them
    // only under the predicate that makes `merged` true)
    rc = int_done ? DIB_OK : integration_bwd_impl(l, batch, params, grads, ws, stream, true);
    if (rc) return rc;
    return encoder_bank_bwd_stages(l, batch, params, grads, beta_dev, inv_global_batch, 3, ws, stream);
  }
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  if (!int_done) {   // dgrad chain from ws[G_PRED] (general output layer) down to ws[G_U]
    rc = small_integration(l, m, w, batch, params, DIB_SMALL_INT_LOAD_H | DIB_SMALL_INT_BWD_OUT | DIB_SMALL_INT_BWD, 0, nullptr, 0,
                           nullptr, 0, 0.f, st);
    if (rc) return rc;
  }
  rc = small_encoder_bwd(l, m, w, batch, params, beta_dev, inv_global_batch, st);
  if (rc) return rc;
  // encoder layers 1 .. n_enc (layer 0 comes out of the backward kernel as partials), integration hidden layers, and the
  // general output layer when this call ran its backward (the fused head reduces its own partials in the tail)
  const int count = l->n_enc * l->F + l->n_int + (int_done ? 0 : 1);
  return merged_wgrad(l, m, w, batch, wgrad_target(m, w, grads), 0, count, st);
}

// part: see part_bounds
int dib_grads_finalize_part(dib_layout* l, int batch, int part, float* grads, void* ws, dib_stream_t stream) {
  if (!l || !grads || !ws || batch <= 0 || part < -1 || part > 3) return DIB_E_ARG;
  const auto m = l->map(batch);
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  if (m.nsplit > 1) {
    // partial slabs are spaced align_up(n_params,4) apart
    const long long stride = align_up(l->n_params, 4);
    long long beg, end;
    part_bounds(l, part, &beg, &end);
    if (part == -1 || part == 1) end = stride;   // the last bucket carries the alignment tail of the buffer
    { ProfScope ps(kProfOther, (hipStream_t)stream);
    DIB_LAUNCH(dib_reduce_splits_kernel, dim3(grid_for((end - beg) / 4)), dim3(256), 0, st,
                       (const float*)(w + m.wgrad_partial + beg), end - beg, m.nsplit, stride, grads + beg); }
    int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  if (part != 1 && part != 3 && enc_dw1_parts(l, batch) > 0) {  // layer-1 weight/bias gradients: fixed-order sum of the backward's partials
    ProfScope ps(kProfOther, (hipStream_t)stream);
    DIB_LAUNCH(dib_dw1_reduce_kernel, dim3(l->F, 16), dim3(256), 0, st, (const float*)(w + m.dw1_partial),
                       enc_dw1_parts(l, batch), l->F, l->enc_units[0], l->dev_fused_offs, l->dev_fused_offs + 3 * l->F,
                       l->dev_featmap, grads);
  }
  return (int)hipGetLastError();
}

int dib_grads_finalize(dib_layout* l, int batch, float* grads, void* ws, dib_stream_t stream) {
  return dib_grads_finalize_part(l, batch, -1, grads, ws, stream);
}

int dib_metrics_accumulate(dib_layout* l, int batch, const float* beta_dev, float inv_global_batch,
                           float* metrics_acc, void* ws, dib_stream_t stream) {
  if (!l || !beta_dev || !metrics_acc || !ws || batch <= 0) return DIB_E_ARG;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_metrics_accumulate_kernel, dim3(cdiv(l->F + 3, 64)), dim3(64), 0, (hipStream_t)stream,
                     w + m.step_out, l->F, beta_dev, inv_global_batch, metrics_acc); }
  return (int)hipGetLastError();
}

// ---- the end of a step in one launch (csrc/dib_tail.h) ------------------------------------------------------------
int dib_step_tail(dib_layout* l, int batch, int part, int flags, float* params, float* grads, float* adam_m, float* adam_v,
                  const float* lr_dev, int64_t* t_dev, float beta1, float beta2, float eps, float grad_scale,
                  const float* beta_dev, float inv_global_batch, float* metrics_acc, void* ws, dib_stream_t stream) {
  if (!l || !ws || batch <= 0 || part < -1 || part > 3 || flags <= 0) return DIB_E_ARG;
  const bool adam = (flags & DIB_TAIL_ADAM) != 0, sgd = (flags & DIB_TAIL_SGD) != 0, finalize = (flags & DIB_TAIL_FINALIZE) != 0;
  if (adam && sgd) return DIB_E_ARG;
  if ((finalize || adam || sgd || (flags & DIB_TAIL_HEAD_WGRAD)) && !grads) return DIB_E_ARG;
  if ((adam || sgd) && (!params || !lr_dev)) return DIB_E_ARG;
  if (adam && (!adam_m || !adam_v || !t_dev)) return DIB_E_ARG;
  if ((flags & DIB_TAIL_BUMP) && !t_dev) return DIB_E_ARG;
  if ((flags & DIB_TAIL_METRICS) && (!beta_dev || !metrics_acc)) return DIB_E_ARG;
  if ((flags & DIB_TAIL_LOSS) && (flags & DIB_TAIL_LOSS_HEAD)) return DIB_E_ARG;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  const long long stride = align_up(l->n_params, 4);
  DibTailArgs a;
  std::memset(&a, 0, sizeof(a));
  a.params = params; a.grads = grads; a.m = adam_m; a.v = adam_v; a.lr_dev = lr_dev; a.t_dev = (long long*)t_dev;
  a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gscale = grad_scale; a.flags = flags; a.F = l->F;
  const bool touches = finalize || adam || sgd;   // this launch walks the part's gradient range
  long long beg = 0, end = 0;
  part_bounds(l, part, &beg, &end);
  if (part == -1 || part == 1) end = stride;      // the last bucket carries the alignment tail of the buffer
  const bool dw1_seg = finalize && enc_dw1_parts(l, batch) > 0 && part != 1 && part != 3;
  const bool head_seg = (flags & DIB_TAIL_HEAD_WGRAD) && (part == -1 || part == 1);
  if (head_seg && !dib_output_head_fused_supported(l, DIB_LOSS_BCE_LOGITS)) return DIB_E_UNSUPPORTED;
  if (touches) {
    a.gbeg = dw1_seg ? l->enc_w_off[1][0] : beg;
    a.gend = head_seg ? l->int_w_off[l->n_int] : end;
    if (finalize && m.nsplit > 1) { a.slabs = w + m.wgrad_partial; a.nsplit = m.nsplit; a.slab_stride = stride; }
    const long long n4 = (a.gend - a.gbeg) >> 2;
    if (n4 > 0 && (a.nsplit > 0 || adam || sgd)) a.nb_generic = (int)std::min<long long>(2048, (n4 + 255) / 256);
  }
  if (dw1_seg) {
    a.dw1_partial = w + m.dw1_partial; a.dw1_parts = enc_dw1_parts(l, batch); a.H1 = l->enc_units[0];
    a.w_off = l->dev_fused_offs; a.b_off = l->dev_fused_offs + 3 * l->F; a.featmap = l->dev_featmap;
    a.nb_dw1 = l->F * 16;
  }
  if (head_seg) {
    a.head_partial = w + m.skinny_partial; a.head_chunks = m.skinny_chunks; a.head_K = l->int_width[l->n_int - 1];
    a.head_w_off = l->int_w_off[l->n_int]; a.head_b_off = l->int_b_off[l->n_int];
    a.nb_head = a.head_K + 1;
  }
  a.step_out = w + m.step_out;
  if (flags & DIB_TAIL_KL) {
    a.kl_partial = w + m.kl_partial; a.kl_stride = l->F; a.nb_kl = l->F;
    a.kl_rows = enc_kl_rows(l, m, batch);
  }
  if (flags & (DIB_TAIL_LOSS | DIB_TAIL_LOSS_HEAD)) {
    a.loss_partial = w + m.loss_partial; a.nb_loss = 2; a.rows = (float)batch;
    a.loss_blocks = (flags & DIB_TAIL_LOSS_HEAD) ? m.skinny_chunks : m.loss_blocks;
  }
  a.beta_dev = beta_dev; a.inv_bg = inv_global_batch; a.metrics_acc = metrics_acc;
  a.sync = (unsigned*)(w + m.sync);
  int grid = a.nb_generic + a.nb_dw1 + a.nb_head + a.nb_kl + a.nb_loss;
  if (grid == 0 && !(flags & (DIB_TAIL_BUMP | DIB_TAIL_METRICS))) return DIB_OK;   // nothing to reduce, nothing to step
  grid = std::max(1, grid);
  ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_step_tail_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// ---- optimizers ------------------------------------------------------------------------------------
int dib_adam_step(float* params, const float* grads, float* mm, float* vv, int64_t n, const float* lr_dev,
                  int64_t* t_dev, float beta1, float beta2, float eps, float grad_scale, dib_stream_t stream) {
  if (!params || !grads || !mm || !vv || !lr_dev || !t_dev || n <= 0) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_adam_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, st, params, grads, mm, vv, (long long)n,
                     lr_dev, (const long long*)t_dev, beta1, beta2, eps, grad_scale); }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_bump_counter_kernel, dim3(1), dim3(1), 0, st, (long long*)t_dev); }
  return (int)hipGetLastError();
}

int dib_sgd_step(float* params, const float* grads, int64_t n, const float* lr_dev, float grad_scale,
                 dib_stream_t stream) {
  if (!params || !grads || !lr_dev || n <= 0) return DIB_E_ARG;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_sgd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, params, grads, (long long)n,
                     lr_dev, grad_scale); }
  return (int)hipGetLastError();
}

// ---- evaluation helpers (dib_encode_deterministic: host/encoder.h) ------------------------------------------------------
int dib_bhattacharyya(const float* mu1, const float* lv1, int n, const float* mu2, const float* lv2, int m, int dim,
                      float* out, dib_stream_t stream) {
  if (!mu1 || !lv1 || !mu2 || !lv2 || !out || n <= 0 || m <= 0 || dim <= 0) return DIB_E_ARG;
  DIB_LAUNCH(dib_bhattacharyya_kernel, dim3(grid_for((int64_t)n * m)), dim3(256), 0, (hipStream_t)stream, mu1,
                     lv1, n, mu2, lv2, m, dim, out);
  return (int)hipGetLastError();
}

int dib_positional_encoding(const float* x, int64_t ldx, int n, int d, int n_freq, float* out, dib_stream_t stream) {
  if (!x || !out || n <= 0 || d <= 0) return DIB_E_ARG;
  const int n_blocks = n_freq > 1 ? n_freq : 1;
  DIB_LAUNCH(dib_posenc_dense_kernel, dim3(grid_for((int64_t)n * d)), dim3(256), 0, (hipStream_t)stream, x,
                     (long long)ldx, n, d, n_blocks, out);
  return (int)hipGetLastError();
}

int dib_positional_encoding_rows(const float* x, int64_t ldx, const int32_t* row_idx, int n, int d, int n_freq, float* out,
                                 dib_stream_t stream) {
  if (!x || !row_idx || !out || n <= 0 || d <= 0) return DIB_E_ARG;
  const int n_blocks = n_freq > 1 ? n_freq : 1;
  DIB_LAUNCH(dib_posenc_rows_kernel, dim3(grid_for((int64_t)n * d)), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx,
                     (const int*)row_idx, n, d, n_blocks, out);
  return (int)hipGetLastError();
}

// grads = sum of the nsplit partial slabs (nsplit == 0: grads as given), Keras-Adam on (params, m, v), step count bumped - ONE
// launch (the generic segment of dib_step_tail_kernel) for parameter buffers that are not a dib_layout (dense.DenseStack)
static_assert(DIB_SYNC_WORDS == DIB_TAIL_SYNC_WORDS, "include/dib_hip.h DIB_SYNC_WORDS must cover the tail's arrival counters");
int dib_reduce_adam_step(const float* partial, int nsplit, int64_t stride, float* params, float* grads, float* adam_m,
                         float* adam_v, int64_t n, const float* lr_dev, int64_t* t_dev, float beta1, float beta2, float eps,
                         float grad_scale, uint32_t* sync, dib_stream_t stream) {
  if (!params || !grads || !adam_m || !adam_v || !lr_dev || !t_dev || !sync || n <= 0 || (n & 3) || nsplit < 0) return DIB_E_ARG;
  if (nsplit > 0 && (!partial || stride < n)) return DIB_E_ARG;
  DibTailArgs a;
  std::memset(&a, 0, sizeof(a));
  a.params = params; a.grads = grads; a.m = adam_m; a.v = adam_v; a.lr_dev = lr_dev; a.t_dev = (long long*)t_dev;
  a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gscale = grad_scale; a.flags = DIB_TAIL_ADAM | DIB_TAIL_BUMP;
  a.gbeg = 0; a.gend = n; a.slabs = partial; a.nsplit = nsplit; a.slab_stride = stride;
  a.nb_generic = (int)std::min<int64_t>(2048, (n / 4 + 255) / 256);
  a.sync = sync;
  ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_step_tail_kernel, dim3(a.nb_generic), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int dib_philox_normal_fill(float* eps, const int32_t* row_idx, int64_t row0, int batch, int F, int E, uint64_t seed,
                           uint32_t step, dib_stream_t stream) {
  if (!eps || batch <= 0 || F <= 0 || E <= 0) return DIB_E_ARG;
  DIB_LAUNCH(dib_eps_fill_kernel, dim3(grid_for((int64_t)batch * F * ((E + 3) / 4))), dim3(256), 0,
                     (hipStream_t)stream, eps, (const int*)row_idx, (long long)row0, batch, F, E,
                     (unsigned long long)seed, (unsigned)step);
  return (int)hipGetLastError();
}

float dib_philox_normal_ref(uint64_t seed, uint32_t step, uint32_t row, uint32_t feature, uint32_t e) {
  float out[4];
  dib_eps4(seed, step, row, feature, e >> 2, out);
  return out[e & 3];
}

}  // extern "C"
