// dib_st_info.h - information tracking of the set-transformer notebook (include/dib_st.h dib_mi_probe_map /
// dib_mi_sandwich_batched): the per-particle probe-grid map and the batched sandwich bounds on I(U;X), each as ONE tiled launch
// (+ a table prep and a fixed-order combine) over an encoded table of validation particles.
//
// Both evaluate l_ij = log N(u_i; mu_j, diag(sigma_j^2)) with the arithmetic of dib_gauss_lse.h (the row loop, the merges and the
// closing formula live there).  The data Gaussians come from the table [n_rows][2E] (mu | raw logvar): a group's rows are the
// neighbourhoods it names (neighbourhood k = rows k P .. k P + P - 1).  dib_sti_table_kernel folds 1 / sigma into the table once:
// (1/sigma_e, mu_e/sigma_e) per dimension and c_j per row.
//
// dib_sti_bounds_kernel: grid (probe tiles of 64, groups, row splits), 256 threads.  Lane = probe, wave = every fourth row of a
// block of `rb` data rows staged in LDS (every lane of a wave reads the same row: broadcasts).  A probe's sample u lives in
// registers (EMAX = 32 / 64: E <= EMAX) or in LDS (EMAX = 0: any E <= 256), drawn from the library's Philox noise exactly as
// dib_mi_prep_kernel draws it (row = the probe's index in its chunk / batch, feature 0).  Each workgroup leaves one partial
// (max, sum) per probe; dib_sti_combine_* merge the splits and the batches in a fixed order (no atomics, bit-reproducible).
//   map mode (probes = enc_probe rows, group g = chunk c * nb + batch b, noise step steps[g]):
//     lower = l_ii - (LSE(l_ii, l_i1 .. l_iN) - log(N + 1)),  upper = l_ii - (LSE(l_i1 .. l_iN) - log N), mean over the nb batches
//   sandwich mode (probes = the batch's own n rows, group = batch b, noise step step0 + b):
//     lower_i = l_ii - (LSE_j l_ij - log n),  upper_i = l_ii - (LSE_{j != i} l_ij - log n), j != i by POSITION (a neighbourhood
//     drawn twice contributes its rows twice); per-batch means.
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

#define DIB_STI_THREADS 256

struct DibStiArgs {
  const float* enc_probe;      // map mode: [M][2E]; sandwich mode: unused (the probes are table rows)
  const float* enc_table;      // [n_rows][2E]
  const double2* tab;          // [n_rows][E] (1/sigma, mu/sigma)
  const double* tab_c;         // [n_rows]
  const int* nbhd;             // [G][n_nbhd] neighbourhood indices
  const unsigned* steps;       // [G] noise step per group (map mode)
  double2* part;               // [S][G][npad] partial (max, sum) of the data log-sum-exp
  double* lii;                 // [G][npad]
  double* u_out;               // optional [G][gstride][E]
  unsigned long long seed;
  unsigned step0;
  float lv_off;
  int sandwich, E, P, n_nbhd, n_table_nbhd, M, C, nb, G, S, npad, rps, rb, gstride;
};

// (1/sigma, mu/sigma) per (row, dimension) and c per row; one thread per row, dimensions in order (c as dib_mi_prep_kernel)
__global__ void __launch_bounds__(256)
dib_sti_table_kernel(const float* __restrict__ enc, long long n_rows, int E, float lv_off, double2* __restrict__ tab,
                     double* __restrict__ tab_c) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_rows) return;
  const float* mu = enc + j * 2 * E;
  const float* lv = mu + E;
  double slv = 0.0;
  for (int e = 0; e < E; ++e) {
    const double l = (double)lv[e] + (double)lv_off;
    const double is = 1.0 / exp(0.5 * l);
    tab[j * E + e] = make_double2(is, (double)mu[e] * is);
    slv += l;
  }
  tab_c[j] = -0.5 * slv - 0.5 * (double)E * DIB_LN2PI;
}

// table row of data row j of group g (-1: an index outside the table)
__device__ __forceinline__ long long dib_sti_row(const DibStiArgs& a, int g, int j) {
  const int k = a.nbhd[(long long)g * a.n_nbhd + j / a.P];
  if (k < 0 || k >= a.n_table_nbhd) return -1;
  return (long long)k * a.P + j % a.P;
}

template <int EMAX>
__global__ void __launch_bounds__(DIB_STI_THREADS)
dib_sti_bounds_kernel(DibStiArgs a) {
  extern __shared__ double2 sti_lds[];
  const int E = a.E, rb = a.rb;
  double2* st = sti_lds;                                  // [rb][E] staged (1/sigma, mu/sigma)
  double* st_c = (double*)(st + (long long)rb * E);       // [rb]
  double* u_lds = st_c + rb;                              // EMAX == 0: [E][64]
  double2* red = (double2*)(u_lds + (EMAX == 0 ? 64 * E : 0));   // [4][64] per-wave partials
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.y, s = blockIdx.z;
  const int pi = blockIdx.x * 64 + lane;
  const int N = a.n_nbhd * a.P;
  int cnt;
  const float* enc;
  unsigned step;
  bool bad = false;
  if (a.sandwich) {
    cnt = N;
    step = a.step0 + (unsigned)g;
    long long r = pi < cnt ? dib_sti_row(a, g, pi) : 0;
    if (r < 0) { bad = true; r = 0; }
    enc = a.enc_table + r * 2 * E;
  } else {
    const int c = g / a.nb;
    cnt = min(a.C, a.M - c * a.C);
    step = a.steps[g];
    enc = a.enc_probe + ((long long)c * a.C + (pi < cnt ? pi : 0)) * 2 * E;
  }
  const bool act = pi < cnt;
  // the probe's sample and own log-density, in dib_mi_prep_kernel's / dib_mi_probe_rows_kernel's arithmetic
  double u[EMAX > 0 ? EMAX : 1];
  double lii = 0.0;
  {
    double slv = 0.0, q = 0.0;
    const float* mu = enc;
    const float* lv = enc + E;
    constexpr int kQuads = EMAX / 4;   // registers: a compile-time trip count, fully unrolled; LDS: E / 4 quads, not unrolled
#pragma unroll kQuads > 0 ? kQuads : 1
    for (int qd = 0; qd < (EMAX > 0 ? kQuads : E / 4); ++qd) {
      if (EMAX == 0 || 4 * qd < E) {
        float eps[4];
        dib_eps4(a.seed, step, (uint32_t)pi, 0u, (uint32_t)qd, eps);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int e = 4 * qd + t;
          const double l = (double)lv[e] + (double)a.lv_off;
          const double sd = exp(0.5 * l);
          const double is = 1.0 / sd;
          const double ue = (double)mu[e] + sd * (double)eps[t];
          const double d = (ue - (double)mu[e]) * is;
          q = fma(d, d, q);
          slv += l;
          if (EMAX > 0) u[EMAX > 0 ? e : 0] = ue;
          else if (wave == 0) u_lds[e * 64 + lane] = ue;
        }
      }
    }
    const double c = -0.5 * slv - 0.5 * (double)E * DIB_LN2PI;
    lii = bad ? (double)NAN : c - 0.5 * q;
  }
  if (a.u_out && act && s == 0 && wave == 0) {
    double* uo = a.u_out + ((long long)g * a.gstride + pi) * E;
    if (EMAX > 0) {
#pragma unroll
      for (int e = 0; e < (EMAX > 0 ? EMAX : 1); ++e)
        if (e < E) uo[e] = u[e];
    } else {
      for (int e = 0; e < E; ++e) uo[e] = u_lds[e * 64 + lane];
    }
  }
  double mx = -1.0e300, sm = 0.0;
  const int r0 = s * a.rps, r1 = min(N, r0 + a.rps);
  for (int base = r0; base < r1; base += rb) {
    const int nrow = min(rb, r1 - base);
    __syncthreads();   // the previous block's rows are consumed (and, EMAX == 0, u_lds is written)
    for (int idx = threadIdx.x; idx < rb * E; idx += DIB_STI_THREADS) {
      const int r = idx / E, e = idx - r * E;
      double2 v = make_double2(0.0, 0.0);
      if (r < nrow) {
        const long long tr = dib_sti_row(a, g, base + r);
        if (tr >= 0) v = a.tab[tr * E + e];
      }
      st[idx] = v;
    }
    for (int r = threadIdx.x; r < rb; r += DIB_STI_THREADS) {
      double c = -INFINITY;
      if (r < nrow) {
        const long long tr = dib_sti_row(a, g, base + r);
        c = tr >= 0 ? a.tab_c[tr] : (double)NAN;
      }
      st_c[r] = c;
    }
    __syncthreads();
    if (!act) continue;
    dib_gauss_block_lse<EMAX, 1, true>(st, st_c, E, E, nrow, wave, lane, u, u_lds, a.sandwich ? pi - base : -1, mx, sm);
  }
  // the four waves' partials of each probe, merged in wave order
  dib_lse_merge_waves(red, wave, lane, mx, sm);
  if (wave == 0 && act) {
    a.part[((long long)s * a.G + g) * a.npad + pi] = make_double2(mx, sm);
    if (s == 0) a.lii[(long long)g * a.npad + pi] = lii;
  }
}

// log-sum-exp over the data rows of probe i of group g: its splits in split order
__device__ __forceinline__ double dib_sti_data_lse(const DibStiArgs& a, int g, int i) {
  const double2 p = dib_lse_of_splits(a.part, a.S, (long long)a.G * a.npad, (long long)g * a.npad + i);
  return dib_lse_value(p.x, p.y);
}

// map mode: one thread per probe; batches summed in order b = 0 .. nb-1, then / nb
__global__ void __launch_bounds__(256)
dib_sti_combine_map_kernel(DibStiArgs a, double* __restrict__ lower, double* __restrict__ upper) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.M) return;
  const int c = i / a.C, p = i - c * a.C;
  const double N = (double)a.n_nbhd * a.P;
  double lo = 0.0, up = 0.0;
  for (int b = 0; b < a.nb; ++b) {
    const int g = c * a.nb + b;
    const double l = a.lii[(long long)g * a.npad + p];
    double li, ui;
    dib_sandwich_pair(l, dib_sti_data_lse(a, g, p), log(N + 1.0), log(N), li, ui);
    lo += li;
    up += ui;
  }
  lower[i] = lo / (double)a.nb;
  upper[i] = up / (double)a.nb;
}

// sandwich mode: one workgroup per batch; per-row bounds (optionally written), their means by a fixed tree
__global__ void __launch_bounds__(256)
dib_sti_combine_sandwich_kernel(DibStiArgs a, double* __restrict__ lower_b, double* __restrict__ upper_b,
                                double* __restrict__ lower_rows, double* __restrict__ upper_rows) {
  __shared__ double slo[256], sup[256];
  const int g = blockIdx.x;
  const int n = a.n_nbhd * a.P;
  const double logn = log((double)n);
  double lo = 0.0, up = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double l = a.lii[(long long)g * a.npad + i];
    double li, ui;
    dib_sandwich_pair(l, dib_sti_data_lse(a, g, i), logn, logn, li, ui);
    if (lower_rows) { lower_rows[(long long)g * n + i] = li; upper_rows[(long long)g * n + i] = ui; }
    lo += li;
    up += ui;
  }
  slo[threadIdx.x] = lo;
  sup[threadIdx.x] = up;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      slo[threadIdx.x] += slo[threadIdx.x + w];
      sup[threadIdx.x] += sup[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    lower_b[g] = slo[0] / (double)n;
    upper_b[g] = sup[0] / (double)n;
  }
}
