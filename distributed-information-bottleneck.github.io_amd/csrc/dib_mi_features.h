// dib_mi_features.h - the sandwich bounds on I(U_f;X_f) of EVERY feature of a DistributedIBNet in one evaluation
// (include/dib_mi_features.h): the InfoNCE lower and leave-one-out upper bound of dib_mi_sandwich_rows, for all
// (feature, evaluation batch) groups of a feature-major encoding [F][plane_rows][2E] - the encoder bank's DIB_WS_ENC_OUT - as
// three launches whatever F and nb are: table prep, tiled bounds, fixed-order combine.
//
// The arithmetic is dib_gauss_lse.h's, the register / LDS split that of dib_sti_bounds_kernel and dib_mic_terms_kernel.  What
// differs from those two families is the addressing and the noise key: group g = (feature f, batch b) = f nb + b is the n
// CONTIGUOUS rows row0 + b n .. of plane f (no index list), and its samples are keyed (seed, step0 + b, row i, feature0 + f) -
// the keys of dib_mi_sandwich_rows on that slice, which the sibling families cannot produce (they key feature 0).
//
// dib_mif_table_kernel folds 1 / sigma into the groups' rows once: (1/sigma_e, mu_e/sigma_e) per dimension and c_j per row,
// packed group-major [G][n].  dib_mif_bounds_kernel<EMAX>: grid (sample tiles of 64, groups, row splits), 256 threads.  Lane =
// sample, wave = every fourth row of a block of `rb` rows staged in LDS (a wave reads one row: broadcasts), two rows per pass.
// EMAX = 32 / 64: the sample lives in registers, any E <= EMAX - a partial last quad of the noise is guarded as in
// dib_mi_prep_kernel, and the staged rows are padded with (0, 0) to blocks of 8 dimensions (the samples with 0) so that the
// dimension loop branches once per block and a padded dimension adds exactly 0.  EMAX = 0: the tile's samples live in LDS
// ([E][64]), E a multiple of 4 up to 256.  Each workgroup leaves one (max, sum) per sample; dib_mif_combine_kernel merges the
// splits in split order, closes the two bounds and reduces a group's rows by a fixed tree.  The split count is a function of n
// alone (host/mi_features.h): a group's bits do not depend on F, nb, or the groups that share its launch.
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

#define DIB_MIF_THREADS 256

struct DibMifArgs {
  const float* enc;            // [F][plane_rows][2E] (mu | logvar)
  const double2* tab;          // [G * n][E] (1/sigma, mu/sigma), group-major
  const double* tab_c;         // [G * n]
  double2* part;               // [S][G][npad] partial (max, sum) of the log-sum-exp over the split's rows, own row excluded
  double* lii;                 // [G][npad] the sample's own log-density
  double* u_out;               // optional [G][n][E]
  unsigned long long seed;
  long long plane_rows, row0;
  unsigned step0, feature0;
  int E, n, nb, G, S, npad, rps, rb;
};

// first row of group g in enc (rows of 2E floats)
__device__ __forceinline__ long long dib_mif_group_row(const DibMifArgs& a, int g) {
  const int f = g / a.nb, b = g - f * a.nb;
  return (long long)f * a.plane_rows + a.row0 + (long long)b * a.n;
}

// one thread per (group, row), dimensions in order: dib_sti_table_kernel's arithmetic on the groups' rows
__global__ void __launch_bounds__(256)
dib_mif_table_kernel(DibMifArgs a, double2* __restrict__ tab, double* __restrict__ tab_c) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (long long)a.G * a.n) return;
  const int g = (int)(j / a.n), i = (int)(j - (long long)g * a.n);
  const int E = a.E;
  const float* mu = a.enc + (dib_mif_group_row(a, g) + i) * 2 * E;
  const float* lv = mu + E;
  double slv = 0.0;
  for (int e = 0; e < E; ++e) {
    const double l = (double)lv[e];
    const double is = 1.0 / exp(0.5 * l);
    tab[j * E + e] = make_double2(is, (double)mu[e] * is);
    slv += l;
  }
  tab_c[j] = -0.5 * slv - 0.5 * (double)E * DIB_LN2PI;
}

template <int EMAX>
__global__ void __launch_bounds__(DIB_MIF_THREADS)
dib_mif_bounds_kernel(DibMifArgs a) {
  extern __shared__ double2 mif_lds[];
  const int E = a.E, rb = a.rb, n = a.n;
  const int pitch = EMAX > 0 ? (E + 7) & ~7 : E;          // registers: staged rows padded to whole blocks of 8 dimensions
  double2* st = mif_lds;                                  // [rb][pitch] staged (1/sigma, mu/sigma)
  double* st_c = (double*)(st + (long long)rb * pitch);   // [rb] (rb is even: what follows stays 16-byte aligned)
  double* u_lds = st_c + rb;                              // EMAX == 0: [E][64]
  double2* red = (double2*)(u_lds + (EMAX == 0 ? 64 * E : 0));   // [4][64] per-wave partials
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.y, s = blockIdx.z;
  const int pi = blockIdx.x * 64 + lane;
  const bool act = pi < n;
  const int f = g / a.nb, b = g - f * a.nb;
  const unsigned step = a.step0 + (unsigned)b, feature = a.feature0 + (unsigned)f;
  // the sample and its own log-density, in dib_mi_prep_kernel's / dib_mi_rows_kernel's arithmetic
  double u[EMAX > 0 ? EMAX : 1];
  double lii = 0.0;
  {
    double slv = 0.0, q = 0.0;
    const float* mu = a.enc + (dib_mif_group_row(a, g) + (act ? pi : 0)) * 2 * E;
    const float* lv = mu + E;
    constexpr int kQuads = EMAX / 4;   // registers: a compile-time trip count, fully unrolled; LDS: E / 4 quads, not unrolled
#pragma unroll kQuads > 0 ? kQuads : 1
    for (int qd = 0; qd < (EMAX > 0 ? kQuads : E / 4); ++qd) {
      float eps[4] = {0.f, 0.f, 0.f, 0.f};
      if (EMAX == 0 || 4 * qd < E) dib_eps4(a.seed, step, (uint32_t)pi, feature, (uint32_t)qd, eps);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int e = 4 * qd + t;
        double ue = 0.0;
        if (EMAX == 0 || e < E) {   // (a partial last quad: the dimensions past E take no noise and stay 0)
          const double l = (double)lv[e];
          const double sd = exp(0.5 * l);
          const double is = 1.0 / sd;
          ue = (double)mu[e] + sd * (double)eps[t];
          const double d = (ue - (double)mu[e]) * is;
          q = fma(d, d, q);
          slv += l;
        }
        if (EMAX > 0) u[EMAX > 0 ? e : 0] = ue;
        else if (wave == 0) u_lds[e * 64 + lane] = ue;
      }
    }
    lii = -0.5 * slv - 0.5 * (double)E * DIB_LN2PI - 0.5 * q;
  }
  if (a.u_out && act && s == 0 && wave == 0) {
    double* uo = a.u_out + ((long long)g * n + pi) * E;
    if (EMAX > 0) {
#pragma unroll
      for (int e = 0; e < (EMAX > 0 ? EMAX : 1); ++e)
        if (e < E) uo[e] = u[e];
    } else {
      for (int e = 0; e < E; ++e) uo[e] = u_lds[e * 64 + lane];
    }
  }
  double mx = -1.0e300, sm = 0.0;
  const long long trow0 = (long long)g * n;                // the group's first row in the folded table
  const int r0 = s * a.rps, r1 = min(n, r0 + a.rps);
  for (int base = r0; base < r1; base += rb) {
    const int nrow = min(rb, r1 - base);
    __syncthreads();   // the previous block's rows are consumed (and, EMAX == 0, u_lds is written)
    const double2* src = a.tab + (trow0 + base) * E;
    for (int idx = threadIdx.x; idx < nrow * pitch; idx += DIB_MIF_THREADS) {
      const int j = idx / pitch, e = idx - j * pitch;
      st[idx] = e < E ? src[(long long)j * E + e] : make_double2(0.0, 0.0);
    }
    for (int j = threadIdx.x; j < nrow; j += DIB_MIF_THREADS) st_c[j] = a.tab_c[trow0 + base + j];
    __syncthreads();
    if (!act) continue;
    dib_gauss_block_lse<EMAX, (EMAX > 0 ? 8 : 1), true>(st, st_c, pitch, E, nrow, wave, lane, u, u_lds, pi - base, mx, sm);
  }
  // the four waves' partials of each sample, merged in wave order
  dib_lse_merge_waves(red, wave, lane, mx, sm);
  if (wave == 0 && act) {
    a.part[((long long)s * a.G + g) * a.npad + pi] = make_double2(mx, sm);
    if (s == 0) a.lii[(long long)g * a.npad + pi] = lii;
  }
}

// one workgroup per group: the splits of each row merged in split order, the two bounds (optionally written), the group's means
// by a fixed tree (thread i sums rows i, i + 256, ... in order); out [G][2]
__global__ void __launch_bounds__(256)
dib_mif_combine_kernel(DibMifArgs a, double* __restrict__ out, double* __restrict__ lower_rows, double* __restrict__ upper_rows) {
  __shared__ double slo[256], sup[256];
  const int g = blockIdx.x;
  const int n = a.n;
  const double logn = log((double)n);
  double lo = 0.0, up = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double2 p = dib_lse_of_splits(a.part, a.S, (long long)a.G * a.npad, (long long)g * a.npad + i);
    double li, ui;
    dib_sandwich_pair(a.lii[(long long)g * a.npad + i], dib_lse_value(p.x, p.y), logn, logn, li, ui);
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
    out[2 * (long long)g] = slo[0] / (double)n;
    out[2 * (long long)g + 1] = sup[0] / (double)n;
  }
}
