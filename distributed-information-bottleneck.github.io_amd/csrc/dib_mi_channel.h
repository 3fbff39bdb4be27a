// dib_mi_channel.h - Monte-Carlo I(U;X) of a channel with known diagonal-Gaussian conditionals (include/dib_mi_channel.h; the
// reference's MI-bound characterization notebook, paper Fig. S4): term = l_r - (LSE_j l_j - log n_rows) per sample, the sample
// drawn from row r of the group's table, l_j over every row of that table, float64 with a log-sum-exp.
//
// The arithmetic is dib_gauss_lse.h's, on tables folded by dib_sti_table_kernel (dib_st_info.h).  What differs is where a
// sample's own conditional comes from: not an extra term beside the data rows but ONE of them, chosen by index - so l_r is
// evaluated from the folded row r with the very FMA sequence of the row loop (the same bits as that row's l_j: for Gaussians far
// apart l_r - LSE is exactly -log(multiplicity)), and no row is ever excluded.
//
// dib_mic_terms_kernel<EMAX>: grid (sample tiles of 64, groups, row splits), 256 threads.  Lane = sample (u in registers,
// E <= EMAX = 32 / 64), wave = every fourth row of a block of `rb` rows staged in LDS (a wave reads one row: broadcasts), two
// rows per pass.  The staged rows are padded to blocks of 8 dimensions with (0, 0) and the samples with 0, so the dimension
// loop branches once per block (16 LDS reads in flight) and a padded dimension adds exactly 0 to q.  Each workgroup leaves one
// (max, sum) per sample; dib_mic_combine_kernel merges the splits in order, forms the terms and reduces a group's terms by a
// fixed tree.  The split count is a function of (n_rows, n_samples) alone (host/mi.h), never of the number of groups:
// a group's bits do not depend on which other groups share its launch.
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

#define DIB_MIC_THREADS 256

struct DibMicArgs {
  const float* enc;            // [n_tables][n_rows][2E]
  const double2* tab;          // [n_tables * n_rows][E] (1/sigma, mu/sigma)
  const double* tab_c;         // [n_tables * n_rows]
  const int* group_table;      // [G]
  const int* src;              // [G][n_samples]
  double2* part;               // [S][G][npad] partial (max, sum) of the log-sum-exp over the split's rows
  double* lr;                  // [G][npad] the sample's own log-density (NaN: an index outside the tables)
  double* u_out;               // optional [G][n_samples][E]
  unsigned long long seed;
  unsigned step0;
  int E, n_tables, n_rows, n_samples, G, S, npad, rps, rb;
};

template <int EMAX>
__global__ void __launch_bounds__(DIB_MIC_THREADS)
dib_mic_terms_kernel(DibMicArgs a) {
  extern __shared__ double2 mic_lds[];
  const int E = a.E, rb = a.rb;
  const int Ep = (E + 7) & ~7;                            // staged rows are padded with (0, 0) to whole blocks of 8 dimensions
  double2* st = mic_lds;                                  // [rb][Ep] staged (1/sigma, mu/sigma)
  double* st_c = (double*)(st + (long long)rb * Ep);      // [rb] (rb is even: what follows stays 16-byte aligned)
  double2* red = (double2*)(st_c + rb);                   // [4][64] per-wave partials
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.y, s = blockIdx.z;
  const int si = blockIdx.x * 64 + lane;
  const bool act = si < a.n_samples;
  bool bad = false;
  int t = a.group_table[g];
  if (t < 0 || t >= a.n_tables) { bad = true; t = 0; }
  int r = act ? a.src[(long long)g * a.n_samples + si] : 0;
  if (r < 0 || r >= a.n_rows) { bad = true; r = 0; }
  const long long row0 = (long long)t * a.n_rows;          // the table's first row in the stacked arrays
  // the sample, in dib_mi_prep_kernel's arithmetic: u = mu + exp(logvar / 2) eps, eps keyed (seed, step0 + g, sample, 0)
  double u[EMAX];
  {
    const float* mu = a.enc + (row0 + r) * 2 * E;
    const float* lv = mu + E;
#pragma unroll
    for (int qd = 0; qd < EMAX / 4; ++qd) {
      float eps[4] = {0.f, 0.f, 0.f, 0.f};
      if (4 * qd < E) dib_eps4(a.seed, a.step0 + (unsigned)g, (uint32_t)si, 0u, (uint32_t)qd, eps);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = 4 * qd + k;
        double ue = 0.0;
        if (e < E) ue = (double)mu[e] + exp(0.5 * (double)lv[e]) * (double)eps[k];
        u[e] = ue;
      }
    }
  }
  if (a.u_out && act && s == 0 && wave == 0) {
    double* uo = a.u_out + ((long long)g * a.n_samples + si) * E;
#pragma unroll
    for (int e = 0; e < EMAX; ++e)
      if (e < E) uo[e] = u[e];
  }
  if (s == 0 && wave == 0 && act) {
    // own log-density from the folded row r: the FMA sequence of the row loop below
    double q[1] = {0.0};
    dib_gauss_q<EMAX, 1, 1>(a.tab + (row0 + r) * E, 0, E, u, nullptr, lane, q);
    a.lr[(long long)g * a.npad + si] = bad ? (double)NAN : a.tab_c[row0 + r] - 0.5 * q[0];
  }
  double mx = -1.0e300, sm = 0.0;
  const int r0 = s * a.rps, r1 = min(a.n_rows, r0 + a.rps);
  for (int base = r0; base < r1; base += rb) {
    const int nrow = min(rb, r1 - base);
    __syncthreads();   // the previous block's rows are consumed
    const double2* src = a.tab + (row0 + base) * E;
    for (int idx = threadIdx.x; idx < nrow * Ep; idx += DIB_MIC_THREADS) {
      const int j = idx / Ep, e = idx - j * Ep;
      st[idx] = e < E ? src[j * E + e] : make_double2(0.0, 0.0);
    }
    for (int j = threadIdx.x; j < nrow; j += DIB_MIC_THREADS) st_c[j] = a.tab_c[row0 + base + j];
    __syncthreads();
    if (!act) continue;
    dib_gauss_block_lse<EMAX, 8, false>(st, st_c, Ep, E, nrow, wave, lane, u, nullptr, 0, mx, sm);
  }
  // the four waves' partials of each sample, merged in wave order
  dib_lse_merge_waves(red, wave, lane, mx, sm);
  if (wave == 0 && act) a.part[((long long)s * a.G + g) * a.npad + si] = make_double2(mx, sm);
}

// one workgroup per group: the splits of each sample merged in split order, term = l_r - (LSE - log n_rows) (optionally written),
// the group's mean by a fixed tree (thread i sums samples i, i + 256, ... in order)
__global__ void __launch_bounds__(256)
dib_mic_combine_kernel(DibMicArgs a, double* __restrict__ group_means, double* __restrict__ sample_terms) {
  __shared__ double ssum[256];
  const int g = blockIdx.x;
  const double logn = log((double)a.n_rows);
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.n_samples; i += 256) {
    const double2 p = dib_lse_of_splits(a.part, a.S, (long long)a.G * a.npad, (long long)g * a.npad + i);
    // (not dib_lse_value: every row is summed, so the sum is 0 only where its log is -inf anyway, and a NaN table stays NaN)
    const double term = a.lr[(long long)g * a.npad + i] - (p.x + log(p.y) - logn);
    if (sample_terms) sample_terms[(long long)g * a.n_samples + i] = term;
    acc += term;
  }
  ssum[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) ssum[threadIdx.x] += ssum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) group_means[g] = ssum[0] / (double)a.n_samples;
}
