// host/small.h - the row-tile integration kernel (csrc/dib_small.h): cluster sizing, the layout's launches, the plain-MLP entry
// points (include/dib_hip.h dib_mlp_small_*) and the companion protocol that pairs the two in one grid.

// A second, independent network for the NEXT dib_small_integration_kernel launch of this thread to carry in its grid
// (dib_integration_fwd_and_mlp_fwd / dib_backward_and_mlp_bwd arm it; whoever armed it launches it alone if nobody took it).
struct SmallCompanion { DibSmallIntArgs args; size_t lds = 0; bool armed = false; };
static thread_local SmallCompanion t_companion;

// workgroups per row tile of a row-tile network launch (dib_small.h "cluster mode"; 1 = the single-workgroup kernel): "int_cluster"
// while the launch stays within "int_cluster_wgs" workgroups, the network's hidden layers hold at least "int_cluster_min_weights"
// weights (below that a layer is a few microseconds on one CU and the exchanges cost more than they save) and the wider exchange
// buffer fits the LDS
static int small_cluster_size(const DibSmallIntArgs& a, size_t lds_bytes, int other_wgs = 0) {
  int cl = std::min(knobs().int_cluster, DIB_SMALL_CL_MAX);
  const int budget = std::min(knobs().int_cluster_wgs, device_cus());   // one workgroup per CU (141 KB of LDS each)
  // more row tiles: 4 per tile instead of 8 while the launch (with the other network of a paired grid: other_wgs) stays within the
  // budget - every workgroup must be resident for the networks to run side by side; 2 per tile measured no gain
  // (profiles/r06u_int_cluster_sweep.txt)
  while (cl > 4 && small_tiles(a.batch) * cl + other_wgs > budget) cl >>= 1;
  if (cl <= 1 || small_tiles(a.batch) * cl + other_wgs > budget || lds_bytes > kSmallMaxLds) return 1;
  if (a.mode & (DIB_SMALL_INT_HEAD_REDUCE)) return 1;   // (its last-arriver reduce counts workgroups, not tiles)
  long long weights = 0;
  for (int i = 0, k = a.K0; i < a.n_hidden; k = a.width[i], ++i) weights += (long long)k * a.width[i];
  return weights >= knobs().int_cluster_min_weights ? cl : 1;
}

// the network part of an argument set: input width, hidden widths and (as width[n_hidden]) the output layer's, where the layers sit
// in `params`, the activations
static void small_fill_net(DibSmallIntArgs& a, const float* params, int K0, int n_hidden, const int* width, const int64_t* w_off,
                           const int64_t* b_off, int act, int out_act) {
  a.params = params; a.K0 = K0; a.n_hidden = n_hidden;
  for (int i = 0; i <= n_hidden; ++i) { a.width[i] = width[i]; a.w_off[i] = w_off[i]; a.b_off[i] = b_off[i]; }
  a.act = act; a.out_act = out_act; a.out_dim = width[n_hidden];
}

// arms cluster mode on an argument set - `cl` workgroups per row tile, arrival counters `sync` - and returns the x dimension of
// its grid: 8 ceil(tiles / 8) x cl (dib_small.h dib_small_integration_cluster_kernel)
static int small_arm_cluster(DibSmallIntArgs& a, int cl, unsigned* sync) {
  a.cl = cl; a.cl_sync = sync; a.cl_agent_scope = knobs().int_cluster_short_exchange ? 0 : 1;
  return 8 * cdiv(small_tiles(a.batch), 8) * cl;
}

// one launch of dib_small_integration_kernel; `mode` = DIB_SMALL_INT_* bits.  Head arguments may be null / 0 without a head.
static int small_integration(dib_layout* l, const dib_layout::WsMap& m, float* w, int batch, const float* params, int mode,
                             int loss_kind, const float* y, int64_t ldy, const int32_t* row_idx, int64_t row0, float inv_bg,
                             hipStream_t st) {
  DibSmallIntArgs a;
  std::memset(&a, 0, sizeof(a));
  small_fill_net(a, params, l->F * l->E, l->n_int, l->int_width.data(), l->int_w_off.data(), l->int_b_off.data(), l->act, l->out_act);
  a.U = w + m.U; a.GU = w + m.g_u; a.batch = batch; a.mode = mode;
  // (xh: the exchange buffers of a cluster launch that writes no stashes; read in cluster mode only)
  for (int i = 0; i < l->n_int; ++i) { a.h[i] = w + m.int_h[i]; a.g[i] = w + m.g_int_h[i]; a.xh[i] = w + m.cl_x[i]; }
  a.pred = w + m.pred; a.g_pred = w + m.g_pred;
  a.loss_kind = loss_kind; a.Y = y; a.ldy = ldy; a.row_idx = (const int*)row_idx; a.row0 = row0; a.inv_bg = inv_bg;
  a.partial_w = w + m.skinny_partial; a.partial_l = w + m.loss_partial;
  // cluster mode: few row tiles, each on `cl` workgroups (dib_small.h); cl_extra: what the cluster kernels' wider exchange buffer adds
  // to a launch (the two maps differ in that region alone, so it is the same for the companion)
  const size_t lds = (size_t)l->sb_int_lds;
  const size_t cl_extra = small_int_lds(a.K0, a.n_hidden, a.width, a.out_dim, true, true) - lds;
  unsigned* const sync = (unsigned*)(w + m.cl_sync);
  int cl = small_cluster_size(a, lds + cl_extra);
  if (t_companion.armed) {
    t_companion.armed = false;
    DibSmallIntPair p;
    p.s[0] = a; p.s[1] = t_companion.args;
    // the companion clusters by the same rule on its own size (training launches only: it has no exchange buffers for a launch
    // without stashes); its arrival counters are the second half of this workspace's
    DibSmallIntArgs& c = p.s[1];
    int ccl = (c.mode & DIB_SMALL_INT_INFER) || small_tiles(c.batch) > small_tiles(batch) ? 1 : small_cluster_size(c, t_companion.lds + cl_extra);
    // the two networks run side by side only while all their workgroups are resident (one per CU): the companion first gives up
    // its cluster, then this network sizes itself next to it
    if (small_tiles(batch) * cl + small_tiles(c.batch) * ccl > std::min(knobs().int_cluster_wgs, device_cus())) {
      ccl = 1;
      cl = small_cluster_size(a, lds + cl_extra, small_tiles(c.batch));
    }
    // the cluster grid carries BOTH networks' tiles and the wide exchange buffer: each network fitting on its own is not enough
    // (a companion above 140 KB next to a clustered network) - then both run one workgroup per tile in the plain paired grid
    const size_t both = std::max(lds, t_companion.lds);
    if (both + cl_extra > kSmallMaxLds) cl = ccl = 1;
    ProfScope ps(kProfOther, st);
    if (cl > 1 || ccl > 1) {   // (the companion's arrival counters follow this network's)
      const int gx = std::max(small_arm_cluster(p.s[0], cl, sync),
                              small_arm_cluster(c, ccl, sync + (size_t)small_tiles(batch) * DIB_SMALL_CL_SYNC_WORDS));
      return launch_lds<&dib_small_integration_pair_cluster_kernel>(dim3(gx, 2), dim3(DIB_SMALL_THREADS), both + cl_extra, st, p);
    }
    return launch_lds<&dib_small_integration_pair_kernel>(dim3(std::max(small_tiles(batch), small_tiles(c.batch)), 2),
                                                          dim3(DIB_SMALL_THREADS), both, st, p);
  }
  ProfScope ps(kProfOther, st);
  if (cl > 1) {
    const int gx = small_arm_cluster(a, cl, sync);
    return launch_lds<&dib_small_integration_cluster_kernel>(dim3(gx), dim3(DIB_SMALL_THREADS), lds + cl_extra, st, a);
  }
  return launch_lds<&dib_small_integration_kernel>(dim3(small_tiles(batch)), dim3(DIB_SMALL_THREADS), lds, st, a);
}

// ---- plain MLP on the row-tile kernels (include/dib_hip.h dib_mlp_small_*): dib_small_integration_kernel with its input
// tile built from the batch's rows of X (DIB_SMALL_INT_POSENC_IN) and the dgrad chain stopped at the first layer ----
static int mlp_n_freq(const dib_mlp_desc* d) { return d->n_freq > 1 ? d->n_freq : 1; }
// dynamic LDS bytes of the single-workgroup kernel for this MLP; head: with the 1-unit head's scratch (dib_mlp_small_head_step)
static size_t mlp_small_lds(const dib_mlp_desc* d, bool head) {
  return small_int_lds(d->in_dim * mlp_n_freq(d), d->n_hidden, d->width, d->width[d->n_hidden], false, head);
}
static void mlp_small_fill(const dib_mlp_desc* d, DibSmallIntArgs& a, const float* params, int n) {
  small_fill_net(a, params, d->in_dim * mlp_n_freq(d), d->n_hidden, d->width, d->w_off, d->b_off, d->act, 0);
  a.batch = n; a.in_dim = d->in_dim; a.n_freq = mlp_n_freq(d);
}
static int mlp_small_launch(const dib_mlp_desc* d, const DibSmallIntArgs& a, hipStream_t st) {
  const size_t lds = mlp_small_lds(d, false);
  ProfScope ps(kProfOther, st);
  return launch_lds<&dib_small_integration_kernel>(dim3(small_tiles(a.batch)), dim3(DIB_SMALL_THREADS), lds, st, a);
}
// argument sets of the two passes (validated); DIB_OK, or the error the stand-alone entry point reports
static int mlp_small_fwd_args(const dib_mlp_desc* d, const float* params, const float* x, int64_t ldx, const int32_t* row_idx, int n,
                              float* a0, float* const* h, float* out, DibSmallIntArgs& a) {
  if (!d || !params || !x || !out || n <= 0) return DIB_E_ARG;
  if (!dib_mlp_small_supported(d, n)) return DIB_E_UNSUPPORTED;
  bool stash = a0 != nullptr;
  for (int i = 0; i < d->n_hidden; ++i) stash = stash && h != nullptr && h[i] != nullptr;
  if (a0 != nullptr && !stash) return DIB_E_ARG;
  std::memset(&a, 0, sizeof(a));
  a.mode = DIB_SMALL_INT_FWD | DIB_SMALL_INT_OUT | DIB_SMALL_INT_POSENC_IN | (stash ? 0 : DIB_SMALL_INT_INFER);
  a.X = x; a.ldx = ldx; a.row_idx = (const int*)row_idx; a.row0 = 0; a.a0 = a0; a.pred = out;
  if (stash) for (int i = 0; i < d->n_hidden; ++i) a.h[i] = h[i];
  mlp_small_fill(d, a, params, n);
  return DIB_OK;
}
static int mlp_small_bwd_args(const dib_mlp_desc* d, const float* params, const float* g_out, float* const* h, float* const* g, int n,
                              DibSmallIntArgs& a) {
  if (!d || !params || !g_out || !h || !g || n <= 0) return DIB_E_ARG;
  if (!dib_mlp_small_supported(d, n)) return DIB_E_UNSUPPORTED;
  std::memset(&a, 0, sizeof(a));
  a.mode = DIB_SMALL_INT_LOAD_H | DIB_SMALL_INT_BWD_OUT | DIB_SMALL_INT_BWD | DIB_SMALL_INT_NO_GU;
  a.g_pred = const_cast<float*>(g_out);
  for (int i = 0; i < d->n_hidden; ++i) {
    if (!h[i] || !g[i]) return DIB_E_ARG;
    a.h[i] = h[i]; a.g[i] = g[i];
  }
  mlp_small_fill(d, a, params, n);
  return DIB_OK;
}
// the companion protocol: arm, run the model's entry point, launch alone if the model's path had no row-tile launch to share
static int with_companion(const dib_mlp_desc* d, const DibSmallIntArgs& c, hipStream_t st, int model_rc_fn(void*), void* ctx) {
  t_companion.args = c;
  t_companion.lds = mlp_small_lds(d, false);
  t_companion.armed = true;
  int rc = model_rc_fn(ctx);
  if (t_companion.armed) {
    t_companion.armed = false;
    if (!rc) rc = mlp_small_launch(d, c, st);
  }
  return rc;
}

extern "C" {

int dib_mlp_small_supported(const dib_mlp_desc* d, int batch) {
  if (!d || !knobs().small_batch || !knobs().mlp_row_tiles || batch < 1 || batch > kSmallMaxBatch) return 0;
  if (!small_int_shape_ok(d->n_hidden, d->width, d->act)) return 0;
  // its own: any input of up to 1024 encoded columns; the output layer on row tiles too
  if (d->in_dim < 1 || (int64_t)d->in_dim * mlp_n_freq(d) > 1024) return 0;
  const int out = d->width[d->n_hidden];
  if (out < 16 || out % 16 != 0 || out > 1024) return 0;
  return mlp_small_lds(d, false) <= kSmallAdmitLds ? 1 : 0;
}
int dib_mlp_small_fwd(const dib_mlp_desc* d, const float* params, const float* x, int64_t ldx, const int32_t* row_idx, int n,
                      float* a0, float* const* h, float* out, dib_stream_t stream) {
  if (n == 0) return DIB_OK;
  DibSmallIntArgs a;
  if (int rc = mlp_small_fwd_args(d, params, x, ldx, row_idx, n, a0, h, out, a)) return rc;
  return mlp_small_launch(d, a, (hipStream_t)stream);
}
int dib_mlp_small_bwd(const dib_mlp_desc* d, const float* params, const float* g_out, float* const* h, float* const* g, int n,
                      dib_stream_t stream) {
  if (n == 0) return DIB_OK;
  DibSmallIntArgs a;
  if (int rc = mlp_small_bwd_args(d, params, g_out, h, g, n, a)) return rc;
  return mlp_small_launch(d, a, (hipStream_t)stream);
}
int dib_mlp_small_head_supported(const dib_mlp_desc* d, int n) {
  if (!d || !knobs().small_batch || !knobs().mlp_row_tiles || n < 1 || n > kSmallMaxBatch) return 0;
  if (!small_int_shape_ok(d->n_hidden, d->width, d->act)) return 0;
  // its own: an input of whole 16-unit tiles (dL/dx), no positional encoding, the 1-unit output
  if (d->in_dim < 16 || d->in_dim % 16 || d->in_dim > 1024 || d->n_freq > 1) return 0;
  if (d->width[d->n_hidden] != 1) return 0;
  return mlp_small_lds(d, true) <= kSmallAdmitLds ? 1 : 0;
}
int64_t dib_mlp_small_head_workspace_bytes(const dib_mlp_desc* d, int n) {
  if (!d || n < 1 || d->n_hidden < 1 || d->n_hidden > 3) return DIB_E_ARG;
  return ((int64_t)small_tiles(n) * (d->width[d->n_hidden - 1] + 1 + 2) + 16) * (int64_t)sizeof(float);
}
// the head step's argument set on (one replica's) buffers; DIB_OK or the entry point's error.  ws: partials, then the arrival word
static int mlp_small_head_args(const dib_mlp_desc* d, const float* params, const float* x, int n, const float* y, int64_t ldy,
                               int loss_kind, float inv_global_batch, float* const* h, float* const* g, float* pred, float* g_pred,
                               float* g_x, float* grads, float* sums3, void* ws, DibSmallIntArgs& a) {
  if (!d || !params || !x || !y || !h || !g || !pred || !g_pred || !grads || !sums3 || !ws || n <= 0) return DIB_E_ARG;
  if (loss_kind != DIB_LOSS_BCE_LOGITS && loss_kind != DIB_LOSS_MSE) return DIB_E_UNSUPPORTED;
  if (!dib_mlp_small_head_supported(d, n)) return DIB_E_UNSUPPORTED;
  std::memset(&a, 0, sizeof(a));
  a.mode = DIB_SMALL_INT_FWD | DIB_SMALL_INT_HEAD | DIB_SMALL_INT_HEAD_GRAD | DIB_SMALL_INT_BWD | DIB_SMALL_INT_HEAD_REDUCE |
           (g_x ? 0 : DIB_SMALL_INT_NO_GU);
  small_fill_net(a, params, d->in_dim, d->n_hidden, d->width, d->w_off, d->b_off, d->act, 0);   // (the 1-unit output: out_dim = 1)
  a.U = x; a.GU = g_x; a.batch = n;
  for (int i = 0; i < d->n_hidden; ++i) {
    if (!h[i] || !g[i]) return DIB_E_ARG;
    a.h[i] = h[i]; a.g[i] = g[i];
  }
  a.pred = pred; a.g_pred = g_pred; a.loss_kind = loss_kind; a.Y = y; a.ldy = ldy; a.row_idx = nullptr; a.row0 = 0;
  a.inv_bg = inv_global_batch;
  const int tiles = small_tiles(n), KL = d->width[d->n_hidden - 1];
  float* w = (float*)ws;
  a.partial_w = w; a.partial_l = w + (int64_t)tiles * (KL + 1);
  a.sync = (unsigned*)(a.partial_l + 2 * tiles);   // zero at first use (the caller zero-fills the workspace once)
  a.head_gw = grads + d->w_off[d->n_hidden]; a.head_gb = grads + d->b_off[d->n_hidden];
  a.sums3 = sums3; a.loss_scale = inv_global_batch;
  return DIB_OK;
}
int dib_mlp_small_head_step(const dib_mlp_desc* d, const float* params, const float* x, int n, const float* y, int64_t ldy,
                            int loss_kind, float inv_global_batch, float* const* h, float* const* g, float* pred, float* g_pred,
                            float* g_x, float* grads, float* sums3, void* ws, dib_stream_t stream) {
  DibSmallIntArgs a;
  if (int rc = mlp_small_head_args(d, params, x, n, y, ldy, loss_kind, inv_global_batch, h, g, pred, g_pred, g_x, grads, sums3, ws, a))
    return rc;
  const size_t lds = mlp_small_lds(d, true);
  ProfScope ps(kProfOther, (hipStream_t)stream);
  return launch_lds<&dib_small_integration_kernel>(dim3(small_tiles(n)), dim3(DIB_SMALL_THREADS), lds, (hipStream_t)stream, a);
}

// ---- R replicas of the head step in ONE launch (csrc/dib_small.h dib_small_integration_batched_kernel): grid (row tiles, R) ----
int dib_mlp_small_head_batched_supported(const dib_mlp_desc* d, int n, int replicas) {
  return replicas >= 1 && replicas <= 65535 && dib_mlp_small_head_supported(d, n) ? 1 : 0;
}
// floats between the replicas' workspace slices: the single entry's workspace, rounded up to 64 bytes
static int64_t mlp_small_head_ws_stride(const dib_mlp_desc* d, int n) {
  return align_up(dib_mlp_small_head_workspace_bytes(d, n), 64) / (int64_t)sizeof(float);
}
int64_t dib_mlp_small_head_batched_workspace_bytes(const dib_mlp_desc* d, int n, int replicas) {
  if (!d || n < 1 || replicas < 1 || d->n_hidden < 1 || d->n_hidden > 3) return DIB_E_ARG;
  return (int64_t)replicas * mlp_small_head_ws_stride(d, n) * (int64_t)sizeof(float);
}
int dib_mlp_small_head_step_batched(const dib_mlp_desc* d, const float* params, int64_t param_stride, const float* x, int n,
                                    int replicas, const float* y, int64_t ldy, int loss_kind, float inv_global_batch,
                                    float* const* h, float* const* g, float* pred, float* g_pred, float* g_x, float* grads,
                                    int64_t grad_stride, float* sums3, void* ws, dib_stream_t stream) {
  if (param_stride < 0 || grad_stride < 0) return DIB_E_ARG;
  DibSmallIntBatch p;
  if (int rc = mlp_small_head_args(d, params, x, n, y, ldy, loss_kind, inv_global_batch, h, g, pred, g_pred, g_x, grads, sums3, ws, p.a))
    return rc;
  if (!dib_mlp_small_head_batched_supported(d, n, replicas)) return DIB_E_UNSUPPORTED;
  p.param_stride = param_stride; p.grad_stride = grad_stride; p.ws_stride = mlp_small_head_ws_stride(d, n);
  const size_t lds = mlp_small_lds(d, true);
  ProfScope ps(kProfOther, (hipStream_t)stream);
  return launch_lds<&dib_small_integration_batched_kernel>(dim3(small_tiles(n), replicas), dim3(DIB_SMALL_THREADS), lds,
                                                           (hipStream_t)stream, p);
}

int dib_integration_fwd_and_mlp_fwd(dib_layout* l, int batch, const float* params, void* ws, const dib_mlp_desc* d,
                                    const float* mlp_params, const float* x, int64_t ldx, const int32_t* row_idx, int n, float* a0,
                                    float* const* h, float* out, dib_stream_t stream) {
  DibSmallIntArgs c;
  if (int rc = mlp_small_fwd_args(d, mlp_params, x, ldx, row_idx, n, a0, h, out, c)) return rc;
  struct Ctx { dib_layout* l; int batch; const float* params; void* ws; dib_stream_t stream; } ctx{l, batch, params, ws, stream};
  return with_companion(d, c, (hipStream_t)stream, [](void* p) {
    Ctx* q = (Ctx*)p;
    return dib_integration_fwd(q->l, q->batch, q->params, q->ws, q->stream);
  }, &ctx);
}
int dib_backward_and_mlp_bwd(dib_layout* l, int batch, const float* params, float* grads, const float* beta_dev,
                             float inv_global_batch, int flags, void* ws, const dib_mlp_desc* d, const float* mlp_params,
                             const float* g_out, float* const* h, float* const* g, int n, dib_stream_t stream) {
  DibSmallIntArgs c;
  if (int rc = mlp_small_bwd_args(d, mlp_params, g_out, h, g, n, c)) return rc;
  struct Ctx { dib_layout* l; int batch; const float* params; float* grads; const float* beta_dev; float inv; int flags; void* ws;
               dib_stream_t stream; } ctx{l, batch, params, grads, beta_dev, inv_global_batch, flags, ws, stream};
  return with_companion(d, c, (hipStream_t)stream, [](void* p) {
    Ctx* q = (Ctx*)p;
    return dib_backward(q->l, q->batch, q->params, q->grads, q->beta_dev, q->inv, q->flags, q->ws, q->stream);
  }, &ctx);
}

#ifdef DIB_SMALL_TIMING
// diagnostic build only (not declared in include/): phase marks of the last launches of the row-tile kernels (dib_small.h)
int dib_small_debug_read(long long* out64) {
  if (hipDeviceSynchronize() != hipSuccess) return DIB_E_ARG;
  return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(dib_small_dbg), 64 * sizeof(long long));
}
#endif

}  // extern "C"
