// host/measure.h - the measurement-partition model (include/dib_measure.h, csrc/dib_measure.h).

static bool measure_shape_ok(const dib_measure_desc* d) {
  if (!d) return false;
  if (d->in_dim < 1 || d->in_dim > 4 || d->E < 1 || d->E > 32 || d->A < 2 || d->A > 16 || d->L < 1 || d->L > 32) return false;
  if (d->H1 < 16 || d->H1 > 128 || d->H1 % 16 || d->H2 < 16 || d->H2 > 128 || d->H2 % 16) return false;   // 8 tiles in registers
  if (!(d->act >= 0 && d->act <= 2)) return false;
  for (int i = 0; i < 3; ++i) if (d->w_off[i] < 0 || d->b_off[i] < 0) return false;
  return true;
}

static DibMeasureArgs measure_args(const dib_measure_desc* d, const float* params) {
  DibMeasureArgs a;
  std::memset(&a, 0, sizeof(a));
  a.w1 = params + d->w_off[0]; a.b1 = params + d->b_off[0];
  a.w2 = params + d->w_off[1]; a.b2 = params + d->b_off[1];
  a.w3 = params + d->w_off[2]; a.b3 = params + d->b_off[2];
  a.E = d->E; a.H1 = d->H1; a.H2 = d->H2; a.A = d->A; a.L = d->L;
  a.slope = d->act == 0 ? 1.f : (d->act == 1 ? 0.f : 0.2f);
  return a;
}

// fixed_cap: the forward's KL partials are summed in workgroup order, so its grid (and with it the summation order) is a function
// of the row count alone - the same bits on any device and under any "num_cus" setting; the other kernels take one workgroup
// per CU (the grid is co-resident at the notebook's widths), which changes no result
static constexpr long long kMeasureFwdGrid = 256;
static int measure_grid(long long rows, bool fixed_cap = false) {
  const long long tiles = (rows + 15) / 16;
  const long long need = (tiles + DIB_MEASURE_WAVES - 1) / DIB_MEASURE_WAVES;
  const long long cap = fixed_cap ? kMeasureFwdGrid : (long long)split_rule_cus();
  return (int)std::max(1ll, std::min(need, cap));
}

// which: 0 = forward, 1 = backward, 2 = symbolize.  (The envelope's largest packing - E = 32, H1 = H2 = 128 - is 91 KB, below
// 160 KB with the kernels' static LDS.)
static int measure_launch(int which, const DibMeasureArgs& a, int grid, hipStream_t st) {
  const size_t lds = (size_t)dib_measure_lds_floats(a.E, a.H1, a.H2, which != 1) * sizeof(float);
  const dim3 g(grid), b(DIB_MEASURE_THREADS);
  if (which == 0) return launch_lds<&dib_measure_fwd_kernel<8>>(g, b, lds, st, a);
  if (which == 1) return launch_lds<&dib_measure_bwd_kernel<8>>(g, b, lds, st, a);
  return launch_lds<&dib_measure_symbolize_kernel<8>>(g, b, lds, st, a);
}

extern "C" {

int dib_measure_supported(const dib_measure_desc* d) { return measure_shape_ok(d) ? 1 : 0; }

int64_t dib_measure_workspace_bytes(const dib_measure_desc* d, int rows) {
  if (!measure_shape_ok(d) || rows <= 0) return DIB_E_UNSUPPORTED;
  return (int64_t)measure_grid(rows, true) * 8 + 64;
}

int dib_measure_fwd(const dib_measure_desc* d, const float* params, const float* enc, int rows, uint64_t seed, uint32_t step,
                    float beta, float kl_exponent, float* z, float* h1, float* h2, float* soft, float* out3, void* ws,
                    dib_stream_t stream) {
  if (!measure_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !enc || rows <= 0 || !z || !h1 || !h2 || !soft || !out3 || !ws) return DIB_E_ARG;
  DibMeasureArgs a = measure_args(d, params);
  const int grid = measure_grid(rows, true);
  a.enc = enc; a.rows = rows; a.seed = seed; a.step = step; a.beta = beta; a.kl_exp = kl_exponent;
  a.z = z; a.h1s = h1; a.h2s = h2; a.soft = soft; a.out3 = out3;
  a.counter = (unsigned*)ws;
  a.kl_part = (double*)((char*)ws + 64);
  return measure_launch(0, a, grid, (hipStream_t)stream);
}

int dib_measure_bwd(const dib_measure_desc* d, const float* params, const float* enc, int rows, uint64_t seed, uint32_t step,
                    const float* h1, const float* h2, const float* soft, const float* g_agg, const float* w_agg0,
                    int agg_width, const float* out3, float* g3, float* g2, float* g1, float* g_enc, dib_stream_t stream) {
  if (!measure_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !enc || rows <= 0 || rows % d->L || !h1 || !h2 || !soft || !g_agg || !w_agg0 || agg_width <= 0 || !out3 || !g3
      || !g2 || !g1 || !g_enc) return DIB_E_ARG;
  DibMeasureArgs a = measure_args(d, params);
  a.enc = enc; a.rows = rows; a.seed = seed; a.step = step;
  a.h1c = h1; a.h2c = h2; a.softc = soft; a.g_agg = g_agg; a.w_agg0 = w_agg0; a.agg_width = agg_width; a.out3c = out3;
  a.g3 = g3; a.g2 = g2; a.g1 = g1; a.g_enc = g_enc;
  return measure_launch(1, a, measure_grid(rows), (hipStream_t)stream);
}

// ---- R replicas per launch: the replica is the grid's y index (csrc/dib_measure.h) ----
// workspace: one arrival counter per replica, 64 bytes apart | KL partials [replicas][measure_grid(rows, true)] doubles
int64_t dib_measure_batched_workspace_bytes(const dib_measure_desc* d, int rows, int replicas) {
  if (!measure_shape_ok(d) || rows <= 0 || replicas <= 0) return DIB_E_UNSUPPORTED;
  return (int64_t)replicas * 64 + (int64_t)replicas * measure_grid(rows, true) * 8;
}

// launches of replicas [r0, r0 + n) at most DIB_MEASURE_BATCH_SEEDS at a time (one launch for ensembles up to that size)
static int measure_launch_batched(int which, DibMeasureBatchArgs ba, int grid, int replicas, const uint64_t* seeds, hipStream_t st) {
  const size_t lds = (size_t)dib_measure_lds_floats(ba.a.E, ba.a.H1, ba.a.H2, which == 0) * sizeof(float);
  const DibMeasureArgs a0 = ba.a;
  for (int r0 = 0; r0 < replicas; r0 += DIB_MEASURE_BATCH_SEEDS) {
    const int n = std::min(replicas - r0, DIB_MEASURE_BATCH_SEEDS);
    const long long r = r0, rows = a0.rows, ps = r * ba.param_stride;
    DibMeasureArgs& a = ba.a;
    a = a0;
    a.w1 += ps; a.b1 += ps; a.w2 += ps; a.b2 += ps; a.w3 += ps; a.b3 += ps;
    a.enc += r * rows * 2 * a.E;
    if (which == 0) {
      a.z += r * rows * a.E; a.h1s += r * rows * a.H1; a.h2s += r * rows * a.H2; a.soft += r * rows * a.A;
      a.out3 += r * 3; a.kl_part += r * grid; a.counter += r * ba.counter_stride;
    } else {
      a.h1c += r * rows * a.H1; a.h2c += r * rows * a.H2; a.softc += r * rows * a.A;
      a.g_agg += r * (rows / a.L) * a.agg_width; a.w_agg0 += r * ba.w_agg0_stride; a.out3c += r * 3;
      a.g3 += r * rows * a.A; a.g2 += r * rows * a.H2; a.g1 += r * rows * a.H1; a.g_enc += r * rows * 2 * a.E;
    }
    for (int i = 0; i < DIB_MEASURE_BATCH_SEEDS; ++i) ba.seeds[i] = i < n ? seeds[r0 + i] : 0;
    const dim3 g(grid, n), b(DIB_MEASURE_THREADS);
    const int rc = which == 0 ? launch_lds<&dib_measure_batched_fwd_kernel<8>>(g, b, lds, st, ba)
                              : launch_lds<&dib_measure_batched_bwd_kernel<8>>(g, b, lds, st, ba);
    if (rc) return rc;
  }
  return DIB_OK;
}

int dib_measure_fwd_batched(const dib_measure_desc* d, const float* params, int64_t param_stride, const float* enc, int rows,
                            int replicas, const uint64_t* seeds, uint32_t step, float beta, float kl_exponent, float* z, float* h1,
                            float* h2, float* soft, float* out3, void* ws, dib_stream_t stream) {
  if (!measure_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !enc || rows <= 0 || replicas <= 0 || !seeds || param_stride < 0 || param_stride % 4 || !z || !h1 || !h2 || !soft
      || !out3 || !ws) return DIB_E_ARG;
  DibMeasureBatchArgs ba;
  std::memset(&ba, 0, sizeof(ba));
  DibMeasureArgs& a = ba.a;
  a = measure_args(d, params);
  a.enc = enc; a.rows = rows; a.step = step; a.beta = beta; a.kl_exp = kl_exponent;
  a.z = z; a.h1s = h1; a.h2s = h2; a.soft = soft; a.out3 = out3;
  a.counter = (unsigned*)ws;
  a.kl_part = (double*)((char*)ws + (size_t)replicas * 64);
  ba.param_stride = param_stride; ba.counter_stride = 16;
  return measure_launch_batched(0, ba, measure_grid(rows, true), replicas, seeds, (hipStream_t)stream);
}

int dib_measure_bwd_batched(const dib_measure_desc* d, const float* params, int64_t param_stride, const float* enc, int rows,
                            int replicas, const uint64_t* seeds, uint32_t step, const float* h1, const float* h2,
                            const float* soft, const float* g_agg, const float* w_agg0, int64_t w_agg0_stride, int agg_width,
                            const float* out3, float* g3, float* g2, float* g1, float* g_enc, dib_stream_t stream) {
  if (!measure_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !enc || rows <= 0 || rows % d->L || replicas <= 0 || !seeds || param_stride < 0 || param_stride % 4 || !h1 || !h2
      || !soft || !g_agg || !w_agg0 || w_agg0_stride < 0 || agg_width <= 0 || !out3 || !g3 || !g2 || !g1 || !g_enc) return DIB_E_ARG;
  DibMeasureBatchArgs ba;
  std::memset(&ba, 0, sizeof(ba));
  DibMeasureArgs& a = ba.a;
  a = measure_args(d, params);
  a.enc = enc; a.rows = rows; a.step = step;
  a.h1c = h1; a.h2c = h2; a.softc = soft; a.g_agg = g_agg; a.w_agg0 = w_agg0; a.agg_width = agg_width; a.out3c = out3;
  a.g3 = g3; a.g2 = g2; a.g1 = g1; a.g_enc = g_enc;
  ba.param_stride = param_stride; ba.w_agg0_stride = w_agg0_stride;
  // the replicas share the CUs: each takes its share of 2 x CUs workgroups (two full rounds at the notebook's widths, where
  // one workgroup's LDS fills a CU), which stage its weights once and loop over its row tiles; the grid changes no result
  const int grid = std::max(1, std::min(measure_grid(rows), 2 * split_rule_cus() / replicas));
  return measure_launch_batched(1, ba, grid, replicas, seeds, (hipStream_t)stream);
}

int dib_measure_symbolize(const dib_measure_desc* d, const float* params, const float* enc, int64_t n, const float* noise,
                          int K, uint8_t* sym, int32_t* counts, dib_stream_t stream) {
  if (!measure_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !enc || n <= 0 || !noise || K <= 0 || !sym) return DIB_E_ARG;
  DibMeasureArgs a = measure_args(d, params);
  a.enc = enc; a.rows = n; a.noise = noise; a.K = K; a.sym = sym; a.counts = (int*)counts;
  return measure_launch(2, a, measure_grid(n), (hipStream_t)stream);
}

int dib_measure_posenc_rows(const float* x, int64_t ldx, const int32_t* row_idx, int n, int d, int n_freq, int first_exponent,
                            float* out, dib_stream_t stream) {
  if (!x || !row_idx || !out || n <= 0 || d <= 0 || first_exponent < -64 || first_exponent > 64) return DIB_E_ARG;
  const int n_blocks = n_freq > 1 ? n_freq : 1;
  DIB_LAUNCH(dib_measure_posenc_rows_kernel, dim3(grid_for((int64_t)n * d)), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx,
             (const int*)row_idx, n, d, n_blocks, std::ldexp(1.0f, first_exponent), out);
  return (int)hipGetLastError();
}

}  // extern "C"
