// host/compression.h - every feature's compression-scheme matrix in one evaluation (include/dib_compression.h;
// csrc/dib_compression.h): the display-row gather on the layout's column table and the one tiled matrices launch.

// DIB_OK inside the envelope, else the code every entry point returns
static int compression_envelope(int F, int E, int n_max) {
  if (F <= 0 || E <= 0 || n_max <= 0) return DIB_E_ARG;
  if (E > DIB_COMPRESSION_MAX_E || n_max > DIB_COMPRESSION_MAX_ROWS || F > DIB_COMPRESSION_MAX_F) return DIB_E_UNSUPPORTED;
  return DIB_OK;
}

extern "C" {

int dib_compression_supported(int F, int E, int n_max) { return compression_envelope(F, E, n_max) == DIB_OK ? 1 : 0; }

int dib_compression_gather(dib_layout* l, const float* x, int64_t ldx, int64_t n_rows, const int32_t* rows, int n_max,
                           float* xg, dib_stream_t stream) {
  if (!l || !x || !rows || !xg || n_rows <= 0 || ldx < l->sum_d) return DIB_E_ARG;
  if (int rc = compression_envelope(l->F, l->E, n_max)) return rc;
  if (!l->dev_colmap) return DIB_E_ARG;
  DIB_LAUNCH(dib_cmp_gather_kernel, dim3(cdiv((int64_t)n_max * l->sum_d, 256)), dim3(256), 0, (hipStream_t)stream, x,
             (long long)ldx, (long long)n_rows, rows, n_max, l->dev_colmap, l->sum_d, xg);
  return (int)hipGetLastError();
}

int dib_compression_matrices(const float* enc, int64_t plane_rows, int64_t row0, int F, int E, const int32_t* counts, int n_max,
                             float* dist, float* comp, dib_stream_t stream) {
  if (int rc = compression_envelope(F, E, n_max)) return rc;
  if (!enc || !counts || (!dist && !comp)) return DIB_E_ARG;
  if (plane_rows <= 0 || row0 < 0 || row0 + n_max > plane_rows) return DIB_E_ARG;
  const int nt = cdiv(n_max, DIB_CMP_TILE);
  DIB_LAUNCH(dib_cmp_matrices_kernel, dim3(nt * (nt + 1) / 2, F), dim3(DIB_CMP_THREADS), 0, (hipStream_t)stream, enc,
             (long long)plane_rows, (long long)row0, E, counts, n_max, dist, comp);
  return (int)hipGetLastError();
}

}  // extern "C"
