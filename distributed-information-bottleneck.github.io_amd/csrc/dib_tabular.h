// dib_tabular.h - the tabular front end's quantile transform on the device (include/dib_tabular.h): sklearn's
// QuantileTransformer._transform_col, forward branch, element by element in float64 from the float32 table - the mean of
// np.interp forwards and on the negated, reversed tables, the bounds rule, the clip of u and Wichura's AS 241 PPND16.
//
// Two kernels, one arithmetic (dib_tab_u, dib_tab_ndtri).  The table is row-major, so in both consecutive lanes take consecutive
// columns, then the next row: loads of x and stores of out run along the rows.  The two searches of an element are index
// arithmetic on the one pair of tables: the reversed, negated tables of the second interpolation are q[n - 1 - k] and
// ref[n - 1 - k] with the sign flipped, which is exact.  The interpolation and the rational are compiled with contraction off:
// NumPy rounds slope * (x - xp) before it adds fp, an FMA would not.  An element's result depends on its value and its column's
// table alone; which kernel, workgroup and lane computes it decides nothing.
//   dib_tab_quantile_staged_kernel  a workgroup owns a group of columns whose tables fit DIB_TAB_STAGE_BYTES of LDS (4 columns at
//     2000 quantiles) and a slab of rows; it copies the tables once and searches them in LDS.  Taken from
//     DIB_TAB_STAGE_MIN_ROWS_PER_QUANTILE * n_quantiles rows on, while one column's table fits (n_quantiles <= 8192).
//   dib_tab_quantile_kernel  every lane searches its column's table where it lies, in global memory (the tables of a launch stay in
//     L2): small tables, where copying would cost more than it saves, and tables beyond the LDS budget.
// Measured on 2^20 x 64 at 2000 quantiles: 2.23 ms staged against 7.76 ms unstaged (profiles/tabular_bench.json): unstaged, every
// lane of a wave is in another column's table and each step of a search brings a line from L2 for 8 bytes.
#pragma once
#include "dib_common.h"

#define DIB_TAB_THREADS 256
#define DIB_TAB_MAX_BLOCKS 4096   // 2^20 lanes in flight; tables beyond that many elements take further passes of the loop
#define DIB_TAB_STAGE_BYTES 65536 // LDS of the staged variant: the tables of 4 columns at 2000 quantiles, of 1 up to 8192
#define DIB_TAB_STAGE_MIN_ROWS_PER_QUANTILE 4   // staged from 4 n_quantiles rows on: a slab computes >= 4 elements per staged entry
#define DIB_TAB_BOUNDS_THRESHOLD 1e-7   // sklearn.preprocessing._data.BOUNDS_THRESHOLD

// Wichura (1988), Algorithm AS 241, PPND16: the normal quantile of p in (0, 1), about 1e-16 relative
__device__ __forceinline__ double dib_tab_ndtri(double p) {
#pragma clang fp contract(off)
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                          1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                            2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                          4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  double r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
             4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
             2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
             5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
             5.99832206555887937690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// np.interp(x, xp, fp) of one finite-or-infinite x (the caller keeps NaN out) on n >= 2 knots: REV = false reads xp = q,
// fp = ref; REV = true reads xp = -q[::-1], fp = -ref[::-1] from the same arrays.
template <bool REV>
__device__ __forceinline__ double dib_tab_interp(double x, const double* __restrict__ q, const double* __restrict__ ref, int n) {
#pragma clang fp contract(off)
  auto xp = [&](int k) { return REV ? -q[n - 1 - k] : q[k]; };
  auto fp = [&](int k) { return REV ? -ref[n - 1 - k] : ref[k]; };
  if (x > xp(n - 1)) return fp(n - 1);
  if (x < xp(0)) return fp(0);
  int lo = 0, hi = n - 1;   // xp(lo) <= x; the largest such index is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (xp(mid) <= x) lo = mid; else hi = mid - 1;
  }
  const int j = lo;
  const double xj = xp(j), fj = fp(j);
  if (j == n - 1 || xj == x) return fj;
  const double x1 = xp(j + 1), f1 = fp(j + 1);
  const double slope = (f1 - fj) / (x1 - xj);
  double r = slope * (x - xj) + fj;
  if (r != r) {   // NumPy's two fall-backs (an infinite slope against a zero distance)
    r = slope * (x - x1) + f1;
    if (r != r && fj == f1) r = fj;
  }
  return r;
}

// One element: u as it enters the inverse CDF (NaN stays NaN).  q is the element's column's table, in global memory or in LDS.
__device__ __forceinline__ double dib_tab_u(double xv, const double* __restrict__ q, const double* __restrict__ references, int nq,
                                            int distribution) {
  if (xv != xv) return xv;
  double u = 0.5 * (dib_tab_interp<false>(xv, q, references, nq) - dib_tab_interp<true>(-xv, q, references, nq));
  const double q0 = q[0], q1 = q[nq - 1];
  if (distribution == 0) {
    const double u_lo = DIB_TAB_BOUNDS_THRESHOLD - 2.220446049250313e-16, u_hi = 1.0 - u_lo;   // 1e-7 - np.spacing(1)
    if (xv + DIB_TAB_BOUNDS_THRESHOLD > q1) u = 1.0;
    if (xv - DIB_TAB_BOUNDS_THRESHOLD < q0) u = 0.0;   // the lower bound last, as sklearn assigns it
    u = fmin(fmax(u, u_lo), u_hi);
  } else {
    if (xv == q1) u = 1.0;
    if (xv == q0) u = 0.0;
  }
  return u;
}

// distribution 0: normal, 1: uniform.  u64 (optional) [n_rows][n_cols]: u as it enters the inverse CDF.
// 8 waves per SIMD: 64 VGPRs and still no scratch (left alone the compiler keeps the rational's 48 coefficients in registers: 130
// VGPRs, occupancy 3).  Measured on this kernel, occupancy is not what bounds it: 7.74 ms at 8 against 7.84 ms at 4 on 2^20 x 64
// (profiles/tabular_bench_before_staging.json).
#define DIB_TAB_WAVES_PER_EU 8
__global__ void __launch_bounds__(DIB_TAB_THREADS) __attribute__((amdgpu_waves_per_eu(DIB_TAB_WAVES_PER_EU)))
dib_tab_quantile_kernel(const float* __restrict__ x, long long ldx, long long n_rows, int n_cols,
                        const double* __restrict__ quantiles, const double* __restrict__ references, int nq, int distribution,
                        float* __restrict__ out, long long ldo, double* __restrict__ u64) {
  const long long total = n_rows * n_cols, stride = (long long)gridDim.x * DIB_TAB_THREADS;
  long long e = (long long)blockIdx.x * DIB_TAB_THREADS + threadIdx.x;
  if (e >= total) return;
  long long r = e / n_cols;
  int c = (int)(e - r * n_cols);
  const long long dr = stride / n_cols;
  const int dc = (int)(stride - dr * n_cols);
  for (; e < total; e += stride) {
    const double u = dib_tab_u((double)x[r * ldx + c], quantiles + (long long)c * nq, references, nq, distribution);
    if (u64) u64[e] = u;
    out[r * ldo + c] = (float)(distribution == 0 ? dib_tab_ndtri(u) : u);
    r += dr;
    c += dc;
    if (c >= n_cols) { c -= n_cols; ++r; }
  }
}

// The staged variant: workgroup (blockIdx.x, blockIdx.y) owns the group of G consecutive columns from blockIdx.x * G and the slab of
// rows_per_block rows from blockIdx.y * rows_per_block.  It copies the group's tables - G * nq consecutive doubles of `quantiles`,
// at most DIB_TAB_STAGE_BYTES - into LDS once and runs every search of its slab there; `references` (one table for all columns,
// read twice or four times per element after the searches) stays in global memory.  Consecutive lanes take consecutive columns of
// the group, then the next row: a wave reads 64 / G rows' segments of 4 G bytes.  The arithmetic is dib_tab_u's, the same
// function on the same values: the variant changes where the table is read from and nothing of the result.
__global__ void __launch_bounds__(DIB_TAB_THREADS) __attribute__((amdgpu_waves_per_eu(DIB_TAB_WAVES_PER_EU)))
dib_tab_quantile_staged_kernel(const float* __restrict__ x, long long ldx, long long n_rows, int n_cols,
                               const double* __restrict__ quantiles, const double* __restrict__ references, int nq, int distribution,
                               float* __restrict__ out, long long ldo, double* __restrict__ u64, int G, long long rows_per_block) {
  extern __shared__ double dib_tab_sq[];   // [g][nq]
  const int c0 = blockIdx.x * G, g = min(G, n_cols - c0), tid = threadIdx.x;
  const double* __restrict__ src = quantiles + (long long)c0 * nq;
  for (int i = tid; i < g * nq; i += DIB_TAB_THREADS) dib_tab_sq[i] = src[i];
  __syncthreads();
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  const long long count = (min(n_rows, r0 + rows_per_block) - r0) * g;   // elements of the slab
  long long rr = tid / g;
  int cc = tid - (int)rr * g;
  const int dr = DIB_TAB_THREADS / g, dc = DIB_TAB_THREADS - dr * g;
  for (long long i = tid; i < count; i += DIB_TAB_THREADS) {
    const long long r = r0 + rr;
    const int c = c0 + cc;
    const double u = dib_tab_u((double)x[r * ldx + c], dib_tab_sq + cc * nq, references, nq, distribution);
    if (u64) u64[r * n_cols + c] = u;
    out[r * ldo + c] = (float)(distribution == 0 ? dib_tab_ndtri(u) : u);
    rr += dr;
    cc += dc;
    if (cc >= g) { cc -= g; ++rr; }
  }
}
