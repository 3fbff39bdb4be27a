// dib_circuit_bodies.h - the bodies of the Boolean-circuit kernels as text (csrc/dib_circuit.h includes this file once per kernel,
// DIB_CIRCUIT_BODY selecting the body): the single kernels run them on their arguments, the batched kernels
// (dib_circuit_batched_*_kernel, one replica per grid index) on locals of the same names that point at the replica's slices.
// Text, not a shared device function: the code generated for the single kernels stays what it was.
//   1  forward:   table, G, B, sc, seed, step, beta, row_in, row_out, u, y, kl          (workgroup blockIdx.x of the replica)
//   2  backward:  table, G, B, sc, seed, step, beta, rows, g_u, g_sc, g = the gate
//   3  MI bounds: sc, G, xs, n, nb, seed, part_ws, counters, out, g = the gate           (blockIdx.x = chunk, blockIdx.y = batch)
#if DIB_CIRCUIT_BODY == 1
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = idx >> 4, k = idx & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float tot = 0.f;
    for (int g = 0; g < G; ++g) {
      const float s = sc[g], lv = sc[G + g];
      const float v = 0.5f * (s * s + expf(lv) - lv - 1.f);
      kl[g] = v;
      tot += v;
    }
    kl[G] = beta * tot;
  }
  if (b >= B) return;
  const uint32_t mask = (1u << G) - 1u;
  // a caller's index is taken modulo 2^G: no read outside the table whatever it holds
  const uint32_t r = row_in ? ((uint32_t)row_in[b] & mask) : dib_circuit_draw_row(seed, step, (uint32_t)b, G);
  const uint32_t bits = table[r];
  float v = 0.f;
  if (k < G) {
    const float x = ((bits >> k) & 1u) ? 1.f : -1.f;
    v = x * sc[k] + expf(0.5f * sc[G + k]) * dib_circuit_eps(seed, step, (uint32_t)b, (uint32_t)k);
  }
  u[(long long)b * DIB_CIRCUIT_LD + k] = v;
  if (k == 0) {
    row_out[b] = (int32_t)r;
    y[b] = (float)((bits >> G) & 1u);
  }
#elif DIB_CIRCUIT_BODY == 2
  __shared__ double rs[256], rl[256];
  double as = 0.0, al = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const uint32_t bits = table[(uint32_t)rows[b] & ((1u << G) - 1u)];
    const double x = ((bits >> g) & 1u) ? 1.0 : -1.0;
    const double gu = (double)g_u[(long long)b * DIB_CIRCUIT_LD + g];
    as += gu * x;
    al += gu * (double)dib_circuit_eps(seed, step, (uint32_t)b, (uint32_t)g);
  }
  rs[threadIdx.x] = as;
  rl[threadIdx.x] = al;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      rs[threadIdx.x] += rs[threadIdx.x + s];
      rl[threadIdx.x] += rl[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double s = (double)sc[g], lv = (double)sc[G + g];
    g_sc[g] = (float)(rs[0] + (double)beta * s);
    g_sc[G + g] = (float)(rl[0] * 0.5 * exp(0.5 * lv) + (double)beta * 0.5 * (exp(lv) - 1.0));
  }
#elif DIB_CIRCUIT_BODY == 3
  __shared__ double rlo[DIB_CIRCUIT_MI_ROWS], rup[DIB_CIRCUIT_MI_ROWS];
  __shared__ int last;
  const int b = blockIdx.y, chunks = gridDim.x;
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  const int i = blockIdx.x * DIB_CIRCUIT_MI_ROWS + r;
  const bool valid = i < n;
  const float* x = xs + (long long)b * n;
  const float s = sc[g];
  const double l = (double)sc[G + g];
  const double sd = exp(0.5 * l);
  const double is = 1.0 / sd;
  const double c = -0.5 * l - 0.5 * DIB_LN2PI;   // log N(0; 0, sigma^2)
  const float mu_i = valid ? x[i] * s : 0.f;
  const double ui = valid ? (double)mu_i + sd * (double)dib_circuit_eps(seed, (uint32_t)b, (uint32_t)i, (uint32_t)g) : 0.0;
  double mx = -1.0e300, sm = 0.0;   // log-sum-exp over j != i
  if (valid) {
    for (int j = q; j < n; j += 4) {
      if (j == i) continue;
      const double d = (ui - (double)(x[j] * s)) * is;
      dib_lse_add(mx, sm, c - 0.5 * (d * d));
    }
  }
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const double m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sm, o, 64);
    dib_lse_merge(mx, sm, m2, s2);
  }
  if (q == 0) {
    double lo = 0.0, up = 0.0;
    if (valid) {
      const double d = (ui - (double)mu_i) * is;
      const double lii = c - 0.5 * (d * d);
      const double logn = log((double)n);
      dib_sandwich_pair(lii, dib_lse_value(mx, sm), logn, logn, lo, up);
    }
    rlo[r] = lo;
    rup[r] = up;
  }
  __syncthreads();
  const long long pair = (long long)g * nb + b;
  if (threadIdx.x == 0) {
    double lo = 0.0, up = 0.0;
    for (int k = 0; k < DIB_CIRCUIT_MI_ROWS; ++k) { lo += rlo[k]; up += rup[k]; }
    double* p = part_ws + (pair * chunks + blockIdx.x) * 2;
    p[0] = lo;
    p[1] = up;
    __threadfence();
    last = atomicAdd(counters + pair, 1u) == (unsigned)chunks - 1u;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    const double* p = part_ws + pair * chunks * 2;
    double lo = 0.0, up = 0.0;
    for (int k = 0; k < chunks; ++k) {
      lo += __hip_atomic_load(p + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      up += __hip_atomic_load(p + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    out[pair * 2] = lo / (double)n;
    out[pair * 2 + 1] = up / (double)n;
    counters[pair] = 0u;
  }
#else
#error "DIB_CIRCUIT_BODY: 1 (forward), 2 (backward) or 3 (MI bounds)"
#endif
