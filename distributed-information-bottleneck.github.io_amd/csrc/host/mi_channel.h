// host/mi_channel.h - Monte-Carlo I(U;X) of a known Gaussian channel (include/dib_mi_channel.h, csrc/dib_mi_channel.h).

struct MicPlan {
  int tiles = 0, npad = 0, S = 1, rps = 0, rb = 0, emax = 0;
  size_t lds = 0;
  int64_t off_c = 0, off_part = 0, off_lr = 0, bytes = 0;
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
  const int64_t rows = (int64_t)n_tables * n_rows;
  p.off_c = align_up(rows * E * 2, 32);   // doubles
  p.off_part = align_up(p.off_c + rows, 32);
  p.off_lr = align_up(p.off_part + (int64_t)p.S * n_groups * p.npad * 2, 32);
  p.bytes = (p.off_lr + (int64_t)n_groups * p.npad) * (int64_t)sizeof(double);
  return DIB_OK;
}

extern "C" {

int64_t dib_mi_monte_carlo_workspace_bytes(int n_tables, int n_rows, int E, int n_groups, int n_samples) {
  MicPlan p;
  if (int rc = mic_plan(n_tables, n_rows, E, n_groups, n_samples, p)) return rc;
  return p.bytes;
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
  a.enc = enc_tables; a.tab = (const double2*)w; a.tab_c = w + p.off_c; a.group_table = (const int*)group_table;
  a.src = (const int*)src_idx; a.part = (double2*)(w + p.off_part); a.lr = w + p.off_lr; a.u_out = u_out;
  a.seed = (unsigned long long)seed; a.step0 = step0;
  a.E = E; a.n_tables = n_tables; a.n_rows = n_rows; a.n_samples = n_samples; a.G = n_groups; a.S = p.S; a.npad = p.npad;
  a.rps = p.rps; a.rb = p.rb;
  DIB_LAUNCH(dib_sti_table_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, enc_tables, (long long)rows, E, 0.0f, (double2*)w,
             w + p.off_c);
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
