// dib_gauss_lse.h - the one float64 arithmetic under every information estimate of the library (device functions only):
//   l_ij = c_j - 1/2 sum_e ((u_ie - mu_je) / sigma_je)^2,   c_j = -1/2 sum_e logvar_je - E/2 ln(2 pi)
// accumulated with a streaming (max, sum) log-sum-exp, merged in a fixed order, and closed with
//   lower = l_ii - (LSE(l_ii, others) - log n),   upper = l_ii - (LSE(others) - log n').
// Used by dib_mi_rows.h (one workgroup per sample), dib_circuit.h (scalar channels) and the two tiled families dib_st_info.h /
// dib_mi_channel.h (lane = sample, wave = every fourth row of a block of rows staged in LDS as (1/sigma, mu/sigma) pairs, so
// that a term costs two FMAs: d = u_e (1/sigma_e) - mu_e/sigma_e, q += d d).  Every order of summation is fixed: no atomics.
#pragma once
#include "dib_common.h"

#define DIB_LN2PI 1.8378770664093454835606594728112

// an empty accumulator is (mx, sm) = (-1.0e300, 0)
__device__ __forceinline__ void dib_lse_add(double& mx, double& sm, double v) {
  if (v > mx) { sm = sm * exp(mx - v) + 1.0; mx = v; }
  else sm += exp(v - mx);
}

__device__ __forceinline__ void dib_lse_merge(double& mx, double& sm, double m2, double s2) {
  const double m = mx > m2 ? mx : m2;
  sm = sm * exp(mx - m) + s2 * exp(m2 - m);
  mx = m;
}

__device__ __forceinline__ double dib_lse_value(double mx, double sm) { return sm > 0.0 ? mx + log(sm) : -INFINITY; }

__device__ __forceinline__ double dib_logaddexp(double x, double y) {
  const double m = x > y ? x : y;
  return m + log(exp(x - m) + exp(y - m));
}

// the closing formula: the sample's own log-density joins the others in the lower bound only
__device__ __forceinline__ void dib_sandwich_pair(double l_own, double lse_others, double log_n_lower, double log_n_upper,
                                                  double& lower, double& upper) {
  lower = l_own - (dib_logaddexp(l_own, lse_others) - log_n_lower);
  upper = l_own - (lse_others - log_n_upper);
}

// the 256 threads' partials by a fixed tree; the result is (smx[0], ssm[0]), visible to every thread
__device__ __forceinline__ void dib_lse_block_merge_256(double* smx, double* ssm, double mx, double sm) {
  smx[threadIdx.x] = mx;
  ssm[threadIdx.x] = sm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      double m = smx[threadIdx.x], t = ssm[threadIdx.x];
      dib_lse_merge(m, t, smx[threadIdx.x + s], ssm[threadIdx.x + s]);
      smx[threadIdx.x] = m;
      ssm[threadIdx.x] = t;
    }
    __syncthreads();
  }
}

// the row splits' partials part[s * stride + idx] of one sample, merged in split order: (max, sum)
__device__ __forceinline__ double2 dib_lse_of_splits(const double2* part, int S, long long stride, long long idx) {
  double2 p = part[idx];
  double m = p.x, sum = p.y;
  for (int s = 1; s < S; ++s) {
    p = part[s * stride + idx];
    dib_lse_merge(m, sum, p.x, p.y);
  }
  return make_double2(m, sum);
}

// q[k] = sum_e (u_e w.x - w.y)^2 of the NR staged rows t, t + 4 pitch (independent FMA chains) against one sample: u in
// registers (EMAX > 0: E <= EMAX, one branch per BLK dimensions - the rows are staged in whole blocks) or in the [E][64] LDS
// image u_lds (EMAX == 0)
template <int EMAX, int BLK, int NR>
__device__ __forceinline__ void dib_gauss_q(const double2* t, int pitch, int E, const double (&u)[EMAX > 0 ? EMAX : 1],
                                            const double* u_lds, int lane, double (&q)[NR]) {
  if (EMAX > 0) {
#pragma unroll
    for (int c = 0; c < (EMAX > 0 ? EMAX : BLK) / BLK; ++c) {
      if (BLK * c < E) {
#pragma unroll
        for (int k = 0; k < BLK; ++k) {
          const int e = BLK * c + k;
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const double2 w = t[(long long)r * 4 * pitch + e];
            const double d = fma(u[EMAX > 0 ? e : 0], w.x, -w.y);
            q[r] = fma(d, d, q[r]);
          }
        }
      }
    }
  } else {
    for (int e = 0; e < E; ++e) {
      const double ue = u_lds[e * 64 + lane];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const double2 w = t[(long long)r * 4 * pitch + e];
        const double d = fma(ue, w.x, -w.y);
        q[r] = fma(d, d, q[r]);
      }
    }
  }
}

// one wave's rows (wave, wave + 4, ...) of a staged block st [nrow][pitch], st_c [nrow] into the sample's (mx, sm): two rows per
// pass, then the tail.  EXCL: the row at staged position `skip` contributes -inf (a sample's own row, by position).
template <int EMAX, int BLK, bool EXCL>
__device__ __forceinline__ void dib_gauss_block_lse(const double2* st, const double* st_c, int pitch, int E, int nrow, int wave,
                                                    int lane, const double (&u)[EMAX > 0 ? EMAX : 1], const double* u_lds,
                                                    int skip, double& mx, double& sm) {
  int r = wave;
  for (; r + 4 < nrow; r += 8) {
    double q[2] = {0.0, 0.0};
    dib_gauss_q<EMAX, BLK, 2>(st + (long long)r * pitch, pitch, E, u, u_lds, lane, q);
    double v0 = st_c[r] - 0.5 * q[0], v1 = st_c[r + 4] - 0.5 * q[1];
    if (EXCL && r == skip) v0 = -INFINITY;
    if (EXCL && r + 4 == skip) v1 = -INFINITY;
    dib_lse_add(mx, sm, v0);
    dib_lse_add(mx, sm, v1);
  }
  for (; r < nrow; r += 4) {
    double q[1] = {0.0};
    dib_gauss_q<EMAX, BLK, 1>(st + (long long)r * pitch, pitch, E, u, u_lds, lane, q);
    double v0 = st_c[r] - 0.5 * q[0];
    if (EXCL && r == skip) v0 = -INFINITY;
    dib_lse_add(mx, sm, v0);
  }
}

// the four waves' partials of each lane's sample, merged in wave order through red [4][64]; wave 0 leaves with the result
// (every lane of wave 0 merges, a lane without a sample carries a value its caller never stores)
__device__ __forceinline__ void dib_lse_merge_waves(double2* red, int wave, int lane, double& mx, double& sm) {
  __syncthreads();
  red[wave * 64 + lane] = make_double2(mx, sm);
  __syncthreads();
  if (wave == 0)
    for (int w = 1; w < 4; ++w) dib_lse_merge(mx, sm, red[w * 64 + lane].x, red[w * 64 + lane].y);
}
