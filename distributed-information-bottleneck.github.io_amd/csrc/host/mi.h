// host/mi.h - the mutual-information estimates on Gaussian log-densities (csrc/dib_gauss_lse.h): the row kernels' sandwich and
// probe bounds (include/dib_hip.h, include/dib_st.h; csrc/dib_mi_rows.h), the set-transformer notebook's one-launch information
// maps (include/dib_st.h; csrc/dib_st_info.h) and the Monte-Carlo I(U;X) of a known channel (include/dib_mi_channel.h;
// csrc/dib_mi_channel.h).  The scalar-channel bounds of the Boolean circuits are in host/circuit.h.

// ---- the row kernels: dib_mi_prep_kernel's workspace of n points, (4 E + 1) n doubles ----
struct MiPrepWs {
  double *inv_sigma, *u, *c, *mu_t, *is_t;   // 1/sigma, u [n][E]; c [n]; mu, 1/sigma dimension-major [E][n]
};

static int64_t mi_prep_doubles(int64_t n, int E) { return (4ll * E + 1) * n; }

static MiPrepWs mi_prep_ws(double* ws, int n, int E) {
  MiPrepWs w;
  w.inv_sigma = ws;
  w.u = w.inv_sigma + (int64_t)n * E;
  w.c = w.u + (int64_t)n * E;
  w.mu_t = w.c + n;
  w.is_t = w.mu_t + (int64_t)n * E;
  return w;
}

static void mi_prep_launch(const MiPrepWs& w, const float* enc, int n, int E, uint64_t seed, uint32_t step, uint32_t feature,
                           float lv_off, hipStream_t st) {
  DIB_LAUNCH(dib_mi_prep_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, enc, n, E, (unsigned long long)seed, (unsigned)step,
             (unsigned)feature, w.inv_sigma, w.u, w.c, w.mu_t, w.is_t, lv_off);
}

// ---- the tiled kernels: one workspace layout, in doubles (the offsets are multiples of 32) ----
// folded table [rows][E] (double2) at 0, c [rows] at off_c, partials [S][G][npad] (max, sum) at off_part, own log-density
// [G][npad] at off_own
struct TiledWs {
  int64_t off_c = 0, off_part = 0, off_own = 0, bytes = 0;
};

static TiledWs tiled_ws(int64_t rows, int E, int S, int G, int npad) {
  TiledWs w;
  w.off_c = align_up(rows * E * 2, 32);
  w.off_part = align_up(w.off_c + rows, 32);
  w.off_own = align_up(w.off_part + (int64_t)S * G * npad * 2, 32);
  w.bytes = (w.off_own + (int64_t)G * npad) * (int64_t)sizeof(double);
  return w;
}

// ---- information tracking of the set-transformer notebook (include/dib_st.h, csrc/dib_st_info.h) ----
struct StiPlan {
  int G = 0, tiles = 0, npad = 0, S = 1, rps = 0, rb = 0, emax = 0;
  size_t lds = 0;
  TiledWs ws;
};

// grid and workspace of one dib_sti_bounds_kernel launch; false = outside the envelope
static bool sti_plan(int sandwich, int n_probes, int chunk, int n_table_nbhd, int P, int E, int nb, int n_nbhd, StiPlan& p) {
  if (E < 4 || E > 256 || (E & 3) || n_table_nbhd <= 0 || P <= 0 || nb <= 0 || n_nbhd <= 0) return false;
  const int64_t N = (int64_t)n_nbhd * P, rows = (int64_t)n_table_nbhd * P;
  if (N > (1 << 30) || rows > (1ll << 40)) return false;
  int64_t cnt;
  if (sandwich) {
    if (N < 2) return false;
    p.G = nb;
    cnt = N;
  } else {
    if (n_probes <= 0 || chunk <= 0) return false;
    const int64_t g = (int64_t)cdiv(n_probes, chunk) * nb;
    if (g > 65535) return false;
    p.G = (int)g;
    cnt = std::min(chunk, n_probes);
  }
  if (p.G > 65535) return false;
  p.npad = (int)((cnt + 63) / 64 * 64);
  p.tiles = p.npad / 64;
  p.emax = E <= 32 ? 32 : (E <= 64 ? 64 : 0);
  p.rb = p.emax ? (E <= 32 ? 64 : 32) : (E <= 128 ? 16 : 4);
  p.lds = (size_t)p.rb * E * 16 + (size_t)p.rb * 8 + (p.emax ? 0 : (size_t)64 * E * 8) + 4 * 64 * 16;
  // row splits only where (probe tiles x groups) leave the chip short of workgroups; a function of the shape alone
  const int64_t blocks = (int64_t)p.tiles * p.G;
  int64_t S = std::max<int64_t>(1, std::min<int64_t>((2048 + blocks - 1) / blocks, (N + 255) / 256));
  p.rps = (int)((N + S - 1) / S);
  p.S = (int)((N + p.rps - 1) / p.rps);
  p.ws = tiled_ws(rows, E, p.S, p.G, p.npad);
  return true;
}

static int sti_launch(const StiPlan& p, DibStiArgs& a, int64_t rows, double* ws, hipStream_t st) {
  a.tab = (const double2*)ws;
  a.tab_c = ws + p.ws.off_c;
  a.part = (double2*)(ws + p.ws.off_part);
  a.lii = ws + p.ws.off_own;
  a.G = p.G; a.S = p.S; a.npad = p.npad; a.rps = p.rps; a.rb = p.rb;
  DIB_LAUNCH(dib_sti_table_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, a.enc_table, (long long)rows, a.E, a.lv_off,
             (double2*)ws, ws + p.ws.off_c);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  const dim3 grid(p.tiles, p.G, p.S);
  if (p.emax == 32) {
    DIB_LAUNCH(dib_sti_bounds_kernel<32>, grid, dim3(DIB_STI_THREADS), p.lds, st, a);
  } else if (p.emax == 64) {
    DIB_LAUNCH(dib_sti_bounds_kernel<64>, grid, dim3(DIB_STI_THREADS), p.lds, st, a);
  } else {
    // (the largest generic-path footprint - E = 256: 4 staged rows + the tile's samples - is 151 584 B, below the CU's 160 KB)
    return launch_lds<&dib_sti_bounds_kernel<0>>(grid, dim3(DIB_STI_THREADS), p.lds, st, a);
  }
  return (int)hipGetLastError();
}

// ---- Monte-Carlo I(U;X) of a known Gaussian channel (include/dib_mi_channel.h, csrc/dib_mi_channel.h) ----
struct MicPlan {
  int tiles = 0, npad = 0, S = 1, rps = 0, rb = 0, emax = 0;
  size_t lds = 0;
  TiledWs ws;
};

// grid and workspace of one dib_mic_terms_kernel launch; DIB_OK or the code both entry points return
static int mic_plan(int n_tables, int n_rows, int E, int n_groups, int n_samples, MicPlan& p) {
  if (n_tables <= 0 || n_rows <= 0 || E <= 0 || n_groups <= 0 || n_samples <= 0) return DIB_E_ARG;
  if (E > 64 || n_rows < 2 || n_rows > 65536 || n_samples > (1 << 20) || n_groups > 65535 || n_tables > 65536) return DIB_E_UNSUPPORTED;
  p.npad = (n_samples + 63) / 64 * 64;
  p.tiles = p.npad / 64;
  p.emax = E <= 32 ? 32 : 64;
  p.rb = E <= 32 ? 64 : 32;
  const int Ep = (E + 7) & ~7;   // staged rows are padded to blocks of 8 dimensions
  p.lds = (size_t)p.rb * Ep * 16 + (size_t)p.rb * 8 + 4 * 64 * 16;   // at most 37 376 B
  // row splits where one group's sample tiles alone would leave the chip short of workgroups: a function of (n_rows, n_samples)
  // and NOT of n_groups, so that a group's merge order - its bits - is the same whichever groups share the launch
  const int S = std::max(1, std::min(256 / p.tiles, (n_rows + 255) / 256));
  p.rps = (n_rows + S - 1) / S;
  p.S = (n_rows + p.rps - 1) / p.rps;
  p.ws = tiled_ws((int64_t)n_tables * n_rows, E, p.S, n_groups, p.npad);
  return DIB_OK;
}

extern "C" {

int64_t dib_mi_workspace_bytes(int n, int E) {
  if (n <= 0 || E <= 0) return DIB_E_ARG;
  return (int64_t)sizeof(double) * mi_prep_doubles(n, E);
}

int dib_mi_sandwich_rows(const float* enc_out, int n, int E, uint64_t seed, uint32_t step, uint32_t feature,
                         double* lower_rows, double* upper_rows, void* ws, dib_stream_t stream) {
  if (!enc_out || !lower_rows || !upper_rows || !ws || n <= 1 || E <= 0) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const MiPrepWs w = mi_prep_ws((double*)ws, n, E);
  mi_prep_launch(w, enc_out, n, E, seed, step, feature, 0.f, st);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  DIB_LAUNCH(dib_mi_rows_kernel, dim3(n), dim3(256), 0, st, enc_out, n, E, (const double*)w.inv_sigma, (const double*)w.u,
             (const double*)w.c, (const double*)w.mu_t, (const double*)w.is_t, lower_rows, upper_rows);
  return (int)hipGetLastError();
}

int64_t dib_mi_probe_workspace_bytes(int n_probes, int n_data, int E) {
  if (n_probes <= 0 || n_data <= 0 || E <= 0) return DIB_E_ARG;
  return (int64_t)sizeof(double) * mi_prep_doubles((int64_t)n_probes + n_data, E);   // per point set as dib_mi_workspace_bytes
}

int dib_mi_probe_bounds(const float* enc_probe, int n_probes, const float* enc_data, int n_data, int E, float logvar_offset,
                        uint64_t seed, uint32_t step, uint32_t feature, double* lower_rows, double* upper_rows,
                        double* u_probe_out, void* ws, dib_stream_t stream) {
  if (!enc_probe || !enc_data || !lower_rows || !upper_rows || !ws || n_probes <= 0 || n_data <= 0 || E <= 0) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const MiPrepWs p = mi_prep_ws((double*)ws, n_probes, E);
  const MiPrepWs d = mi_prep_ws((double*)ws + mi_prep_doubles(n_probes, E), n_data, E);
  mi_prep_launch(p, enc_probe, n_probes, E, seed, step, feature, logvar_offset, st);
  mi_prep_launch(d, enc_data, n_data, E, seed, step, feature + 1u, logvar_offset, st);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  DIB_LAUNCH(dib_mi_probe_rows_kernel, dim3(n_probes), dim3(256), 0, st, enc_probe, (const double*)p.u, (const double*)p.inv_sigma,
             (const double*)p.c, (const double*)d.mu_t, (const double*)d.is_t, (const double*)d.c, n_data, E, lower_rows,
             upper_rows);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  if (u_probe_out)
    return (int)hipMemcpyAsync(u_probe_out, p.u, (size_t)n_probes * E * sizeof(double), hipMemcpyDeviceToDevice, st);
  return DIB_OK;
}

int64_t dib_mi_probe_map_workspace_bytes(int n_probes, int chunk, int n_table_nbhd, int P, int E, int nb, int n_nbhd) {
  StiPlan p;
  if (!sti_plan(0, n_probes, chunk, n_table_nbhd, P, E, nb, n_nbhd, p)) return DIB_E_ARG;
  return p.ws.bytes;
}

int dib_mi_probe_map(const float* enc_probe, int n_probes, int chunk, const float* enc_table, int n_table_nbhd, int P, int E,
                     const int32_t* nbhd_idx, int nb, int n_nbhd, float logvar_offset, uint64_t seed, const uint32_t* steps,
                     double* lower, double* upper, double* u_out, void* ws, dib_stream_t stream) {
  StiPlan p;
  if (!sti_plan(0, n_probes, chunk, n_table_nbhd, P, E, nb, n_nbhd, p)) return DIB_E_ARG;
  if (!enc_probe || !enc_table || !nbhd_idx || !steps || !lower || !upper || !ws || ((uintptr_t)ws & 15)) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  DibStiArgs a;
  std::memset(&a, 0, sizeof(a));
  a.enc_probe = enc_probe; a.enc_table = enc_table; a.nbhd = (const int*)nbhd_idx; a.steps = steps; a.u_out = u_out;
  a.seed = (unsigned long long)seed; a.lv_off = logvar_offset; a.sandwich = 0; a.E = E; a.P = P; a.n_nbhd = n_nbhd;
  a.n_table_nbhd = n_table_nbhd; a.M = n_probes; a.C = chunk; a.nb = nb; a.gstride = chunk;
  int rc = sti_launch(p, a, (int64_t)n_table_nbhd * P, (double*)ws, st);
  if (rc) return rc;
  DIB_LAUNCH(dib_sti_combine_map_kernel, dim3(cdiv(n_probes, 256)), dim3(256), 0, st, a, lower, upper);
  return (int)hipGetLastError();
}

int64_t dib_mi_sandwich_batched_workspace_bytes(int n_table_nbhd, int P, int E, int nb, int n_nbhd) {
  StiPlan p;
  if (!sti_plan(1, 0, 0, n_table_nbhd, P, E, nb, n_nbhd, p)) return DIB_E_ARG;
  return p.ws.bytes;
}

int dib_mi_sandwich_batched(const float* enc_table, int n_table_nbhd, int P, int E, const int32_t* nbhd_idx, int nb, int n_nbhd,
                            float logvar_offset, uint64_t seed, uint32_t step, double* lower_batches, double* upper_batches,
                            double* lower_rows, double* upper_rows, double* u_out, void* ws, dib_stream_t stream) {
  StiPlan p;
  if (!sti_plan(1, 0, 0, n_table_nbhd, P, E, nb, n_nbhd, p)) return DIB_E_ARG;
  if (!enc_table || !nbhd_idx || !lower_batches || !upper_batches || !ws || ((uintptr_t)ws & 15)) return DIB_E_ARG;
  if ((lower_rows == nullptr) != (upper_rows == nullptr)) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  DibStiArgs a;
  std::memset(&a, 0, sizeof(a));
  a.enc_table = enc_table; a.nbhd = (const int*)nbhd_idx; a.u_out = u_out;
  a.seed = (unsigned long long)seed; a.step0 = step; a.lv_off = logvar_offset; a.sandwich = 1; a.E = E; a.P = P;
  a.n_nbhd = n_nbhd; a.n_table_nbhd = n_table_nbhd; a.nb = nb; a.gstride = n_nbhd * P;
  int rc = sti_launch(p, a, (int64_t)n_table_nbhd * P, (double*)ws, st);
  if (rc) return rc;
  DIB_LAUNCH(dib_sti_combine_sandwich_kernel, dim3(nb), dim3(256), 0, st, a, lower_batches, upper_batches, lower_rows, upper_rows);
  return (int)hipGetLastError();
}

int64_t dib_mi_monte_carlo_workspace_bytes(int n_tables, int n_rows, int E, int n_groups, int n_samples) {
  MicPlan p;
  if (int rc = mic_plan(n_tables, n_rows, E, n_groups, n_samples, p)) return rc;
  return p.ws.bytes;
}

int dib_mi_monte_carlo(const float* enc_tables, int n_tables, int n_rows, int E, const int32_t* group_table,
                       const int32_t* src_idx, int n_groups, int n_samples, uint64_t seed, uint32_t step0, double* group_means,
                       double* sample_terms, double* u_out, void* ws, dib_stream_t stream) {
  MicPlan p;
  if (int rc = mic_plan(n_tables, n_rows, E, n_groups, n_samples, p)) return rc;
  if (!enc_tables || !group_table || !src_idx || !group_means || !ws || ((uintptr_t)ws & 15)) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* w = (double*)ws;
  const int64_t rows = (int64_t)n_tables * n_rows;
  DibMicArgs a;
  std::memset(&a, 0, sizeof(a));
  a.enc = enc_tables; a.tab = (const double2*)w; a.tab_c = w + p.ws.off_c; a.group_table = (const int*)group_table;
  a.src = (const int*)src_idx; a.part = (double2*)(w + p.ws.off_part); a.lr = w + p.ws.off_own; a.u_out = u_out;
  a.seed = (unsigned long long)seed; a.step0 = step0;
  a.E = E; a.n_tables = n_tables; a.n_rows = n_rows; a.n_samples = n_samples; a.G = n_groups; a.S = p.S; a.npad = p.npad;
  a.rps = p.rps; a.rb = p.rb;
  DIB_LAUNCH(dib_sti_table_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, enc_tables, (long long)rows, E, 0.0f, (double2*)w,
             w + p.ws.off_c);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  const dim3 grid(p.tiles, n_groups, p.S);
  if (p.emax == 32) {
    DIB_LAUNCH(dib_mic_terms_kernel<32>, grid, dim3(DIB_MIC_THREADS), p.lds, st, a);
  } else {
    DIB_LAUNCH(dib_mic_terms_kernel<64>, grid, dim3(DIB_MIC_THREADS), p.lds, st, a);
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  DIB_LAUNCH(dib_mic_combine_kernel, dim3(n_groups), dim3(256), 0, st, a, group_means, sample_terms);
  return (int)hipGetLastError();
}

}  // extern "C"
