// host/tabular.h - the tabular front end's quantile transform (include/dib_tabular.h; csrc/dib_tabular.h): the envelope, the
// choice between the LDS-staged and the unstaged kernel, and the one launch.  -DDIB_TAB_NO_STAGE builds the library without the
// staged path: the variant tools/tabular_bench.py times beside the product.

// DIB_OK inside the envelope, else the code the entry point returns
static int tabular_envelope(int n_quantiles, int n_cols, int distribution) {
  if (n_quantiles <= 0 || n_cols <= 0) return DIB_E_ARG;
  if (n_quantiles < DIB_TABULAR_MIN_QUANTILES || n_quantiles > DIB_TABULAR_MAX_QUANTILES || n_cols > DIB_TABULAR_MAX_COLS ||
      (distribution != DIB_TABULAR_NORMAL && distribution != DIB_TABULAR_UNIFORM))
    return DIB_E_UNSUPPORTED;
  return DIB_OK;
}

extern "C" {

int dib_quantile_supported(int n_quantiles, int n_cols, int distribution) {
  return tabular_envelope(n_quantiles, n_cols, distribution) == DIB_OK ? 1 : 0;
}

int dib_quantile_transform(const float* x, int64_t ldx, int64_t n_rows, int n_cols, const double* quantiles,
                           const double* references, int n_quantiles, int distribution, float* out, int64_t ldo, double* u64,
                           dib_stream_t stream) {
  if (!x || !quantiles || !references || !out || n_rows <= 0) return DIB_E_ARG;
  if (int rc = tabular_envelope(n_quantiles, n_cols, distribution)) return rc;
  if (ldx < n_cols || ldo < n_cols) return DIB_E_ARG;
  // Staged in LDS (csrc/dib_tabular.h) when at least one column's table fits and the table has enough rows to pay for the copies:
  // every workgroup stages its column group's G * nq doubles, so a slab must hold several times that many elements.
  const int G = std::min<int64_t>(DIB_TAB_STAGE_BYTES / ((int64_t)n_quantiles * 8), n_cols);
#ifndef DIB_TAB_NO_STAGE
  if (G >= 1 && n_rows >= DIB_TAB_STAGE_MIN_ROWS_PER_QUANTILE * (int64_t)n_quantiles) {
    const int groups = cdiv(n_cols, G);
    const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(DIB_TAB_MAX_BLOCKS / groups, 65535),
                                                                 n_rows / (DIB_TAB_STAGE_MIN_ROWS_PER_QUANTILE * (int64_t)n_quantiles)));
    const int64_t rows_per_block = std::max<int64_t>((n_rows + slabs - 1) / slabs, (n_rows + 65534) / 65535);
    DIB_LAUNCH(dib_tab_quantile_staged_kernel, dim3(groups, (unsigned)((n_rows + rows_per_block - 1) / rows_per_block)),
               dim3(DIB_TAB_THREADS), (size_t)G * n_quantiles * 8, (hipStream_t)stream, x, (long long)ldx, (long long)n_rows, n_cols,
               quantiles, references, n_quantiles, distribution, out, (long long)ldo, u64, G, (long long)rows_per_block);
    return (int)hipGetLastError();
  }
#endif
  // a grid-stride loop over the elements: at most DIB_TAB_MAX_BLOCKS workgroups (two rounds of the 8 a CU holds), whatever n_rows is
  const int64_t blocks = std::min<int64_t>((n_rows * n_cols + DIB_TAB_THREADS - 1) / DIB_TAB_THREADS, DIB_TAB_MAX_BLOCKS);
  DIB_LAUNCH(dib_tab_quantile_kernel, dim3((unsigned)blocks), dim3(DIB_TAB_THREADS), 0, (hipStream_t)stream, x, (long long)ldx,
             (long long)n_rows, n_cols, quantiles, references, n_quantiles, distribution, out, (long long)ldo, u64);
  return (int)hipGetLastError();
}

}  // extern "C"
