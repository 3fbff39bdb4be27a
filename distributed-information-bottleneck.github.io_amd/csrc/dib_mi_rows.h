// dib_mi_rows.h - the row kernels of the mutual-information bounds (include/dib_hip.h dib_mi_sandwich_rows, include/dib_st.h
// dib_mi_probe_bounds): one workgroup per sample, the data points strided over its 256 threads, on the arithmetic of
// dib_gauss_lse.h.
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

// ---------------------------------------------------------------------------------------------
// Mutual-information sandwich bounds (reference utils.py:10-73, Poole et al. 2019): for a batch of N
// encoded points with p(u|x_j) = N(mu_j, diag(exp(logvar_j))) and one sample u_i ~ p(u|x_i),
//   log p_ij = -1/2 sum_e ((u_ie - mu_je)/sigma_je)^2 - 1/2 sum_e logvar_je - E/2 ln(2 pi)
//   InfoNCE lower_i = log p_ii - log( 1/N sum_j    p_ij )
//   leave-one-out upper_i = log p_ii - log( 1/N sum_{j!=i} p_ij )      (the reference divides by N, not N-1)
// Everything in float64 like the reference (utils.py:39-40), but with a log-sum-exp so that well separated
// Gaussians do not underflow to log(0) as the reference's exp-then-log does.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
dib_mi_prep_kernel(const float* __restrict__ enc_out /*[N][2E]*/, int n, int E, unsigned long long seed, unsigned step,
                   unsigned feature, double* __restrict__ inv_sigma /*[N][E]*/, double* __restrict__ u /*[N][E]*/,
                   double* __restrict__ cj /*[N]*/, double* __restrict__ mu_t /*[E][N]*/, double* __restrict__ is_t /*[E][N]*/,
                   float lv_off = 0.f /* set transformer: logvar - 3 */) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const float* mu = enc_out + (long long)j * 2 * E;
  const float* lv = mu + E;
  double slv = 0.0;
  for (int q = 0; q < (E + 3) / 4; ++q) {
    float eps[4];
    dib_eps4(seed, step, (uint32_t)j, feature, (uint32_t)q, eps);
    for (int t = 0; t < 4 && 4 * q + t < E; ++t) {
      const int e = 4 * q + t;
      const double l = (double)lv[e] + (double)lv_off;
      const double sd = exp(0.5 * l);
      inv_sigma[(long long)j * E + e] = 1.0 / sd;
      u[(long long)j * E + e] = (double)mu[e] + sd * (double)eps[t];
      // dimension-major copies for the row kernels: thread j of a row's workgroup reads [e][j] - consecutive threads,
      // consecutive addresses (the point-major arrays made every load of the N^2 E inner loop touch 64 cache lines per
      // wave: 218 us per 1024 x 1024 x 32 evaluation; round 3)
      mu_t[(long long)e * n + j] = (double)mu[e];
      is_t[(long long)e * n + j] = 1.0 / sd;
      slv += l;
    }
  }
  cj[j] = -0.5 * slv - 0.5 * (double)E * DIB_LN2PI;
}

__global__ void __launch_bounds__(256)
dib_mi_rows_kernel(const float* __restrict__ enc_out, int n, int E, const double* __restrict__ inv_sigma,
                   const double* __restrict__ u, const double* __restrict__ cj, const double* __restrict__ mu_t,
                   const double* __restrict__ is_t, double* __restrict__ lower_rows, double* __restrict__ upper_rows) {
  __shared__ double smx[256], ssm[256];
  const int i = blockIdx.x;
  const double* ui = u + (long long)i * E;
  double mx = -1.0e300, sm = 0.0;  // log-sum-exp over j != i
  for (int j = threadIdx.x; j < n; j += 256) {
    if (j == i) continue;
    double q = 0.0;
    for (int e = 0; e < E; ++e) {
      const double d = (ui[e] - mu_t[(long long)e * n + j]) * is_t[(long long)e * n + j];
      q = fma(d, d, q);
    }
    dib_lse_add(mx, sm, cj[j] - 0.5 * q);
  }
  dib_lse_block_merge_256(smx, ssm, mx, sm);
  if (threadIdx.x == 0) {
    const float* mu = enc_out + (long long)i * 2 * E;
    const double* is = inv_sigma + (long long)i * E;
    double q = 0.0;
    for (int e = 0; e < E; ++e) {
      const double d = (ui[e] - (double)mu[e]) * is[e];
      q = fma(d, d, q);
    }
    const double lii = cj[i] - 0.5 * q;
    const double logn = log((double)n);
    dib_sandwich_pair(lii, dib_lse_value(smx[0], ssm[0]), logn, logn, lower_rows[i], upper_rows[i]);
  }
}

// Per-particle information map of the set-transformer notebook (probe-grid MI bounds, cell 8 "Now use probe points along
// with a bunch of real points ..."): M probe Gaussians with one sample u_i each, N data Gaussians,
//   lii = log p(u_i | probe_i),  lij = log p(u_i | data_j)
//   lower_i = lii - ( LSE(lii, li1 .. liN) - log(N + 1) )       infonce_per (N + 1 terms in the mean)
//   upper_i = lii - ( LSE(li1 .. liN)      - log N )            loo_per
// float64 with a log-sum-exp (the notebook's exp-then-log underflows for separated Gaussians).  One workgroup per probe.
__global__ void __launch_bounds__(256)
dib_mi_probe_rows_kernel(const float* __restrict__ enc_probe, const double* __restrict__ u_probe,
                         const double* __restrict__ is_probe, const double* __restrict__ c_probe,
                         const double* __restrict__ mu_t_data /*[E][n_data]*/, const double* __restrict__ is_t_data,
                         const double* __restrict__ c_data, int n_data, int E, double* __restrict__ lower_rows,
                         double* __restrict__ upper_rows) {
  __shared__ double smx[256], ssm[256];
  const int i = blockIdx.x;
  const double* ui = u_probe + (long long)i * E;
  double mx = -1.0e300, sm = 0.0;
  for (int j = threadIdx.x; j < n_data; j += 256) {
    double q = 0.0;
    for (int e = 0; e < E; ++e) {
      const double d = (ui[e] - mu_t_data[(long long)e * n_data + j]) * is_t_data[(long long)e * n_data + j];
      q = fma(d, d, q);
    }
    dib_lse_add(mx, sm, c_data[j] - 0.5 * q);
  }
  dib_lse_block_merge_256(smx, ssm, mx, sm);
  if (threadIdx.x == 0) {
    const float* mu = enc_probe + (long long)i * 2 * E;
    const double* is = is_probe + (long long)i * E;
    double q = 0.0;
    for (int e = 0; e < E; ++e) {
      const double d = (ui[e] - (double)mu[e]) * is[e];
      q = fma(d, d, q);
    }
    const double lii = c_probe[i] - 0.5 * q;
    dib_sandwich_pair(lii, dib_lse_value(smx[0], ssm[0]), log((double)n_data + 1.0), log((double)n_data), lower_rows[i],
                      upper_rows[i]);
  }
}
