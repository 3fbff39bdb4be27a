// host/subsets.h - the exhaustive subset informations (include/dib_subsets.h; csrc/dib_subsets.h): the envelope, the number of
// low key bits a workgroup folds in LDS, and the one launch.

// DIB_OK inside the envelope, else the code the entry point returns
static int subset_envelope(int B, int F, int K) {
  if (B <= 0 || F <= 0 || K <= 0) return DIB_E_ARG;
  if (B > DIB_SUBSET_MAX_BITS || F > B || K > DIB_SUBSET_MAX_CLASSES) return DIB_E_UNSUPPORTED;
  return DIB_OK;
}

// ints per row of the LDS table: K rounded up to even (a row later holds one aligned double)
static int subset_row_ints(int K) { return (K + 1) / 2 * 2; }

// low key bits of the fold: the most whose 3^L rows fit the LDS budget, or dib_set_tuning("subset_low_bits") clipped to that
static int subset_low_bits(int B, int K) {
  int most = 0;
  for (int64_t rows = 3; most < DIB_SUBSET_MAX_LOW_BITS && most < B &&
                         rows * subset_row_ints(K) * 4 + DIB_SUBSET_LDS_TAIL <= DIB_SUBSET_LDS_BYTES; rows *= 3)
    ++most;
  const int want = knobs().subset_low_bits;
  return want > 0 ? std::min(want, most) : most;
}

extern "C" {

int dib_subset_information_supported(int B, int F, int K) { return subset_envelope(B, F, K) == DIB_OK ? 1 : 0; }

int64_t dib_subset_information_workspace_bytes(int B, int K) { return subset_envelope(B, 1, K) == DIB_OK ? 0 : -1; }

int dib_subset_information(const int32_t* counts, int B, int K, const int* feature_bits, int F, int mask0, int n_masks,
                           double* out_bits, void* ws, dib_stream_t stream) {
  (void)ws;
  if (!counts || !feature_bits || !out_bits) return DIB_E_ARG;
  if (int rc = subset_envelope(B, F, K)) return rc;
  DibSubsetFeatures ft{};
  int off = 0;
  for (int f = 0; f < F; ++f) {
    if (feature_bits[f] < 1 || off + feature_bits[f] > B) return DIB_E_ARG;
    ft.offset[f] = (unsigned char)off;
    ft.width[f] = (unsigned char)feature_bits[f];
    off += feature_bits[f];
  }
  if (off != B || mask0 < 0 || n_masks < 1 || (int64_t)mask0 + n_masks > ((int64_t)1 << F)) return DIB_E_ARG;
  const int L = subset_low_bits(B, K), Ks = subset_row_ints(K);
  int64_t rows = 1;
  for (int j = 0; j < L; ++j) rows *= 3;
  DIB_LAUNCH(dib_subset_fold_kernel, dim3(1u << (B - L)), dim3(DIB_SUBSET_THREADS), (size_t)(rows * Ks * 4 + DIB_SUBSET_LDS_TAIL),
             (hipStream_t)stream, counts, B, K, Ks, L, ft, F, mask0, n_masks, out_bits);
  return (int)hipGetLastError();
}

}  // extern "C"
