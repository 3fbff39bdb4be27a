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
