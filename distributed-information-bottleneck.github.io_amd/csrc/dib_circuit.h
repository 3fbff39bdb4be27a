// dib_circuit.h - the Boolean-circuit notebook's scalar-channel distributed IB (include/dib_circuit.h;
// complex_systems/InfoDecomp_Boolean_circuits.ipynb cells 4 and 6): everything of a training step in front of the predictor
// (row draw, gather, reparameterisation, KL), the gradient of the 2G encoder scalars behind it, and the sandwich bounds of
// every gate's channel for all evaluation batches in one launch.  The predictor itself runs on the row-tile head kernel
// (dib_mlp_small_head_step) and the grouped weight-gradient GEMM.
//
// Gate g's encoder (SimpleEncoder) holds two scalars, s_g and lv_g (params + sc_off: s[0..G) then lv[0..G)):
//   x in {-1, +1} -> N(x s_g, exp(lv_g)),  u = x s_g + exp(lv_g / 2) eps,  KL_g = 0.5 (s_g^2 + exp(lv_g) - lv_g - 1)
// (mu^2 = s^2 for x = +-1, so the notebook's batch mean of the per-row KL is this value).
//
// Row draw: r_b = x0 >> (32 - G), x0 the first output of Philox4x32-10 at counter (b, 0xFFFFFFFF, 0, step), key = seed.  The
// table has 2^G rows, so the top G bits of a uniform 32-bit word are an exactly uniform row (tf.random.categorical over zero
// logits: uniform, with replacement).  The counter's second word never equals a gate index, so the draw is independent of the
// eps draws, which keep the library's key (seed, step, row b, feature g, dim 0).
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

#define DIB_CIRCUIT_MAX_GATES 16
#define DIB_CIRCUIT_MAX_BATCH 2048
#define DIB_CIRCUIT_LD 16          // u's row pitch: 16 * ceil(G / 16) with G <= 16

__device__ __forceinline__ uint32_t dib_circuit_draw_row(uint64_t seed, uint32_t step, uint32_t b, int G) {
  const dib_u4 c = {b, 0xFFFFFFFFu, 0u, step};
  const dib_u4 r = dib_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return r.x >> (32 - G);
}

__device__ __forceinline__ float dib_circuit_eps(uint64_t seed, uint32_t step, uint32_t b, uint32_t g) {
  float e[4];
  dib_eps4(seed, step, b, g, 0u, e);
  return e[0];
}

// one thread per (row b, column k < 16): u [B][16] (pad columns 0), y [B], drawn rows [B]; workgroup 0 also writes
// kl[0..G) and kl[G] = beta * sum_g kl[g] (summed in gate order)
__global__ void __launch_bounds__(256)
dib_circuit_fwd_kernel(const uint32_t* __restrict__ table, int G, int B, const float* __restrict__ sc, uint64_t seed, uint32_t step,
                       float beta, const int32_t* __restrict__ row_in, int32_t* __restrict__ row_out, float* __restrict__ u,
                       float* __restrict__ y, float* __restrict__ kl) {
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
}

// one workgroup per gate: ds_g = sum_b g_u[b][g] x[b][g] + beta s_g, dlv_g = sum_b g_u[b][g] eps[b][g] exp(lv_g / 2) / 2 +
// beta (exp(lv_g) - 1) / 2 - float64 partials, strided over the batch, then a fixed tree: the same bits on any device
__global__ void __launch_bounds__(256)
dib_circuit_bwd_kernel(const uint32_t* __restrict__ table, int G, int B, const float* __restrict__ sc, uint64_t seed, uint32_t step,
                       float beta, const int32_t* __restrict__ rows, const float* __restrict__ g_u, float* __restrict__ g_sc) {
  __shared__ double rs[256], rl[256];
  const int g = blockIdx.x;
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
}

// Sandwich bounds of every gate's channel for nb evaluation batches of n points (x [nb][n] = +-1), eps of point i of batch b
// keyed (seed, b, i, g).  Per point the arithmetic of dib_mi_prep_kernel + dib_mi_rows_kernel on the encoder output
// (x s_g, lv_g): u_i = mu_i + sigma eps_i, l_ij = c - ((u_i - mu_j) / sigma)^2 / 2 (every point of a gate shares sigma and c),
// lower_i = l_ii - (LSE_j l_ij - log n), upper_i = l_ii - (LSE_{j != i} l_ij - log n), in float64 with a log-sum-exp.
// A workgroup takes 64 points of one (gate, batch), four lanes per point (every fourth j, merged by two shuffles); it sums its
// 64 rows in order into a partial, and the last of the (gate, batch)'s ceil(n / 64) workgroups to arrive sums the partials in
// order: out[g][b] = {lower, upper} (nats), the same bits every call.
#define DIB_CIRCUIT_MI_ROWS 64

__global__ void __launch_bounds__(256)
dib_circuit_mi_kernel(const float* __restrict__ sc, int G, const float* __restrict__ xs, int n, int nb, uint64_t seed,
                      double* __restrict__ part_ws, unsigned* __restrict__ counters, double* __restrict__ out) {
  __shared__ double rlo[DIB_CIRCUIT_MI_ROWS], rup[DIB_CIRCUIT_MI_ROWS];
  __shared__ int last;
  const int b = blockIdx.y, g = blockIdx.z, chunks = gridDim.x;
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
}
