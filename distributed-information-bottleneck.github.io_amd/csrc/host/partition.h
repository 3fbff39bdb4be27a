// host/partition.h - random-MLP partitions (include/dib_partition.h, csrc/dib_partition.h).

static bool partition_shape_ok(const dib_mlp_desc* d) {
  if (!d) return false;
  const int nh = d->n_hidden;
  if (d->in_dim < 1 || d->in_dim > 4 || d->n_freq > 1 || nh < 1 || nh > 3) return false;
  for (int l = 0; l < nh; ++l) if (d->width[l] < 16 || d->width[l] > 128 || d->width[l] % 16) return false;
  if (d->width[nh] < 2 || d->width[nh] > 16) return false;
  if (!(d->act >= DIB_ACT_LINEAR && d->act <= DIB_ACT_TANH)) return false;
  for (int l = 0; l <= nh; ++l) if (d->w_off[l] < 0 || d->b_off[l] < 0) return false;
  return true;
}

template <int ACT>
static int partition_launch(const DibPartitionArgs& a, hipStream_t st) {
  const auto fn = dib_partition_symbolize_kernel<ACT>;
  {
    // the envelope's largest packing (three hidden layers of 128): 140 KB, below 160 KB with the kernel's static LDS - raised to
    // that at once, ahead of the occupancy query below, so that the query sees one limit whatever sizes ran before
    const int w[4] = {128, 128, 128, 16};
    if (int rc = raise_dynamic_lds<&dib_partition_symbolize_kernel<ACT>>(dib_partition_lds_floats(3, w) * sizeof(float))) return rc;
  }
  const size_t lds = (size_t)dib_partition_lds_floats(a.n_hidden, a.width) * sizeof(float);
  // as many workgroups as are co-resident on "num_cus" CUs (the grid-stride loop then makes one pass per workgroup slot); no
  // result depends on the grid: every point is computed by one wave on its own and the counts are integer sums
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, DIB_PARTITION_THREADS, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  const long long tiles = (a.n + 15) / 16;
  const long long need = (tiles + DIB_PARTITION_WAVES - 1) / DIB_PARTITION_WAVES;
  const int grid = (int)std::max(1ll, std::min(need, (long long)split_rule_cus() * per_cu));
  return launch_lds<&dib_partition_symbolize_kernel<ACT>>(dim3(grid), dim3(DIB_PARTITION_THREADS), lds, st, a);
}

extern "C" {

int dib_partition_supported(const dib_mlp_desc* d) { return partition_shape_ok(d) ? 1 : 0; }

int dib_partition_symbolize(const dib_mlp_desc* d, const float* params, const void* x, int x_is_f64, int64_t ldx, int64_t n,
                            uint8_t* sym, float* logits, int64_t* counts, dib_stream_t stream) {
  if (!partition_shape_ok(d)) return DIB_E_UNSUPPORTED;
  if (!params || !x || !sym || n < 0 || ldx < d->in_dim || (x_is_f64 != 0 && x_is_f64 != 1)) return DIB_E_ARG;
  if (n == 0) return DIB_OK;
  DibPartitionArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int l = 0; l <= d->n_hidden; ++l) {
    a.w[l] = params + d->w_off[l];
    a.b[l] = params + d->b_off[l];
    a.width[l] = d->width[l];
  }
  a.x = x; a.x_f64 = x_is_f64; a.ldx = ldx; a.n = n;
  a.in_dim = d->in_dim; a.n_hidden = d->n_hidden;
  a.sym = sym; a.logits = logits; a.counts = (unsigned long long*)counts;
  const hipStream_t st = (hipStream_t)stream;
  switch (d->act) {
    case DIB_ACT_RELU: return partition_launch<DIB_ACT_RELU>(a, st);
    case DIB_ACT_LEAKY_RELU: return partition_launch<DIB_ACT_LEAKY_RELU>(a, st);
    case DIB_ACT_TANH: return partition_launch<DIB_ACT_TANH>(a, st);
    default: return partition_launch<DIB_ACT_LINEAR>(a, st);
  }
}

}  // extern "C"
