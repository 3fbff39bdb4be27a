// dib_measure_bodies.h - the bodies of dib_measure_fwd_kernel (DIB_MEASURE_BODY 1) and dib_measure_bwd_kernel (2) as TEXT, included
// into the single kernel and into its batched twin (csrc/dib_measure.h): both see `DibMeasureArgs a` and walk the row tiles by
// blockIdx.x / gridDim.x.  Text and not a shared __device__ function: behind a function the single kernels' generated code
// changed, and they keep theirs (tools/isa_diff.py).  No include guard - included once per kernel.
#if DIB_MEASURE_BODY == 1   // ---- fwd ----
  extern __shared__ float lds[];
  __shared__ double red[DIB_MEASURE_WAVES];
  __shared__ int last;
  const DibMeasureLds s = dib_measure_stage_fwd(lds, a);
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wave = threadIdx.x >> 6;
  const int E = a.E, A = a.A;
  const long long ntiles = (a.rows + 15) / 16;
  double kl_lane = 0.0;
  for (long long t = (long long)blockIdx.x * DIB_MEASURE_WAVES + wave; t < ntiles; t += (long long)gridDim.x * DIB_MEASURE_WAVES) {
    const long long row = t * 16 + m;
    const bool valid = row < a.rows;
    dib_f4 z[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      float eps[4] = {0.f, 0.f, 0.f, 0.f};
      const int e0 = 16 * it + 4 * g;
      if (valid && e0 < E) dib_eps4(a.seed, a.step, (uint32_t)row, 0u, (uint32_t)(e0 >> 2), eps);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + j;
        float v = 0.f;
        if (valid && e < E) {
          const float mu = a.enc[row * 2 * E + e], lv = a.enc[row * 2 * E + E + e];
          v = mu + eps[j] * expf(0.5f * lv);
          kl_lane += 0.5 * ((double)mu * mu + (double)expf(lv) - (double)lv - 1.0);
          a.z[row * E + e] = v;
        }
        z[it][j] = v;
      }
    }
    dib_f4 h1[MT], h2[MT], lg[1];
    dib_measure_chain<MT>(s, a, z, h1, h2, lg);
    if (valid) {
#pragma unroll
      for (int o = 0; o < MT; ++o) {
        if (16 * o < a.H1) *reinterpret_cast<dib_f4*>(a.h1s + row * a.H1 + 16 * o + 4 * g) = h1[o];
        if (16 * o < a.H2) *reinterpret_cast<dib_f4*>(a.h2s + row * a.H2 + 16 * o + 4 * g) = h2[o];
      }
    }
    // softmax over the A logits of the row: features 4 g .. 4 g + 3 in lane group g
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (4 * g + j < A) mx = fmaxf(mx, lg[0][j]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float ex[4], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { ex[j] = 4 * g + j < A ? expf(lg[0][j] - mx) : 0.f; sum += ex[j]; }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (valid) {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (4 * g + j < A) a.soft[row * A + 4 * g + j] = ex[j] / sum;
    }
  }
  // KL: lanes -> wave (fixed shuffle tree) -> workgroup (wave order) -> grid (workgroup order, last workgroup to arrive)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kl_lane += __shfl_xor(kl_lane, o, 64);
  if (lane == 0) red[wave] = kl_lane;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int w = 0; w < DIB_MEASURE_WAVES; ++w) v += red[w];
    a.kl_part[blockIdx.x] = v;
    __threadfence();
    last = atomicAdd(a.counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    double tot = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) tot += __hip_atomic_load(&a.kl_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double kl = tot / (double)a.rows;
    const double bl = (double)a.beta * (double)a.L;
    a.out3[0] = (float)kl;
    a.out3[1] = (float)(bl * pow(kl, (double)a.kl_exp));
    a.out3[2] = (float)(bl * (double)a.kl_exp * pow(kl, (double)a.kl_exp - 1.0) / (double)a.rows);
    *a.counter = 0u;
  }
#elif DIB_MEASURE_BODY == 2   // ---- bwd ----
  extern __shared__ float lds[];
  const int te = dib_measure_tiles(a.E), t1 = dib_measure_tiles(a.H1), t2 = dib_measure_tiles(a.H2);
  float* w3t = lds;
  float* w2t = w3t + 256 * t2;
  float* w1t = w2t + 256 * t1 * t2;
  dib_measure_stage(w3t, a.w3, a.H2, a.A, true);
  dib_measure_stage(w2t, a.w2, a.H1, a.H2, true);
  dib_measure_stage(w1t, a.w1, a.E, a.H1, true);
  __syncthreads();
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wave = threadIdx.x >> 6;
  const int E = a.E, A = a.A, L = a.L, HA = a.agg_width;
  const float coef = a.out3c[2];
  const long long ntiles = (a.rows + 15) / 16;
  for (long long t = (long long)blockIdx.x * DIB_MEASURE_WAVES + wave; t < ntiles; t += (long long)gridDim.x * DIB_MEASURE_WAVES) {
    const long long row = t * 16 + m;
    const bool valid = row < a.rows;
    const long long b = valid ? row / L : 0;
    const int l = valid ? (int)(row - b * L) : 0;
    // dL/d soft[a] = g_agg[b] . w_agg0[l * A + a] for every a < A: the row's four lanes take every fourth term of the
    // agg_width-long sums and add their partials with two fixed shuffles (all four lanes then hold the same sums); softmax
    // backward on the features 4 g .. 4 g + 3 of lane group g
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    if (valid) {
      const float* gr = a.g_agg + b * HA;
      const float* wr = a.w_agg0 + (long long)(l * A) * HA;
      for (int o = g; o < HA; o += 4) {
        const float gv = gr[o];
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < A) acc[k] = fmaf(gv, wr[(long long)k * HA + o], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k >= A) break;
      acc[k] += __shfl_xor(acc[k], 16, 64);
      acc[k] += __shfl_xor(acc[k], 32, 64);
    }
    float p[4], ds[4], dot = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * g + j;
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) v = q == k ? acc[q] : v;   // register select, no dynamic indexing
      p[j] = (valid && k < A) ? a.softc[row * A + k] : 0.f;
      ds[j] = (valid && k < A) ? v : 0.f;
      dot += p[j] * ds[j];
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    dib_f4 dl[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dl[0][j] = p[j] * (ds[j] - dot);
      if (valid && 4 * g + j < A) a.g3[row * A + 4 * g + j] = dl[0][j];
    }
    dib_f4 d2[MT], d1[MT], dz[2];
    dib_measure_layer_t<1, MT>(w3t, t2, 1, dl, d2);
#pragma unroll
    for (int o = 0; o < MT; ++o) {
      if (o >= t2) break;
      dib_f4 h = valid ? *reinterpret_cast<const dib_f4*>(a.h2c + row * a.H2 + 16 * o + 4 * g) : dib_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) d2[o][j] *= h[j] > 0.f ? 1.f : a.slope;
      if (valid) *reinterpret_cast<dib_f4*>(a.g2 + row * a.H2 + 16 * o + 4 * g) = d2[o];
    }
    dib_measure_layer_t<MT, MT>(w2t, t1, t2, d2, d1);
#pragma unroll
    for (int o = 0; o < MT; ++o) {
      if (o >= t1) break;
      dib_f4 h = valid ? *reinterpret_cast<const dib_f4*>(a.h1c + row * a.H1 + 16 * o + 4 * g) : dib_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) d1[o][j] *= h[j] > 0.f ? 1.f : a.slope;
      if (valid) *reinterpret_cast<dib_f4*>(a.g1 + row * a.H1 + 16 * o + 4 * g) = d1[o];
    }
    dib_measure_layer_t<MT, 2>(w1t, te, t1, d1, dz);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int e0 = 16 * it + 4 * g;
      if (!valid || e0 >= E) continue;
      float eps[4];
      dib_eps4(a.seed, a.step, (uint32_t)row, 0u, (uint32_t)(e0 >> 2), eps);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + j;
        if (e >= E) break;
        const float mu = a.enc[row * 2 * E + e], lv = a.enc[row * 2 * E + E + e];
        const float sg = expf(0.5f * lv);
        a.g_enc[row * 2 * E + e] = dz[it][j] + coef * mu;
        a.g_enc[row * 2 * E + E + e] = dz[it][j] * 0.5f * eps[j] * sg + coef * 0.5f * (expf(lv) - 1.f);
      }
    }
  }
#endif
