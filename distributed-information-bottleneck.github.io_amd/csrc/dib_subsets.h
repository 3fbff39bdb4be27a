// dib_subsets.h - the exhaustive subset informations I(X_S;Y) of a small discrete table on the device (include/dib_subsets.h):
// from the joint counts T[key][class] (int32, key = the features' bit fields concatenated, feature 0 lowest) every subset S of
// the F features gets
//     E[S] = sum_a xlog2(c[a]) - sum_{a,k} xlog2(c[a][k]),   c[a][k] = the sum of T over the keys that agree with a on S's bits
//     bits[S] = E[{}] / N - E[S] / N    (E[{}] / N = H(Y)),   bits[{}] = 0.0
// in float64 with a fixed order of every sum.
//
// One kernel, dib_subset_fold_kernel.  The B key bits are split into L low bits and B - L high bits.  A workgroup owns one mask H
// of high key bits - the 2^L subsets H | S_low - and walks the patterns h of H's bits in ascending order.  Per pattern:
//   build   U[l][k] = the sum of T[(h | d) << L | l][k] over the patterns d of the high bits outside H (ascending; consecutive
//           lanes read consecutive ints: the low bits and the classes are contiguous in T)
//   fold    the 2^L rows of U become the 3^L rows of V: an index is L ternary digits, digit j in {0, 1} = the value of low bit j,
//           2 = low bit j summed out.  Pass j adds the rows with digit j = 0 and 1 into the row with digit j = 2 for every
//           setting of the digits below (already ternary) and above (still binary): 3^L - 2^L row additions in all
//   terms   every row turns, in place, into e = xlog2(sum_k V[k]) - (xlog2(V[0]) + xlog2(V[1]) + ...)  (float64)
//   gather  lane S_low sums e over the rows whose digits are 2 outside S_low, patterns ascending, and adds that sum to its
//           accumulator
// and after the last pattern lane S_low writes bits[H | S_low].  The class totals n_k come out of the same walk (the row with
// every digit 2, summed over h), so the kernel needs no workspace and no second launch.  Integer sums are exact in any order;
// the float64 order above involves neither the grid nor the chunk (mask0, n_masks) nor an address: a chunk only decides which
// workgroups run and which lanes store.  A key mask is a feature subset when it holds every bit field whole or not at all;
// workgroups and lanes whose masks are none (features wider than one bit) or lie outside the chunk leave early / store nothing.
// No atomics, no scratch.  xlog2(c) = c log2(c) in float64, a power of two by its exponent (exact), xlog2(0) = 0.
//
// Work: 2^(2B - L) K reads (L2-resident: T is 2^B K ints) + 3^B K additions + 3^B (K + 1) float64 logarithms.  The workgroup of
// H = all high bits walks 2^(B - L) patterns on its own: at B = 20 it is the tail of the launch (profiles/
// subset_information_bench.json), so the high masks are handed out heaviest first.
#pragma once
#include "dib_common.h"

#define DIB_SUBSET_THREADS 256           // measured against 1024 (profiles/subset_information_bench_1024_threads.json): 1.25 x slower
                                         // up to 18 bits, 1.7 x faster at 20, where the chip is full of workgroups
#define DIB_SUBSET_MAX_LOW_BITS 8        // 2^8 low subsets = one per lane; 3^8 rows of 2 ints = 52 KB of LDS
#define DIB_SUBSET_LDS_BYTES 65536       // dynamic LDS a launch may ask for (no attribute to raise)
#define DIB_SUBSET_LDS_TAIL ((1 << DIB_SUBSET_MAX_LOW_BITS) * 2 + 16 * 8)   // the binary -> ternary index table and the class totals

struct DibSubsetFeatures {   // bit field of feature f in a key: width[f] bits from bit offset[f]
  unsigned char offset[20], width[20];
};

__device__ __forceinline__ double dib_subset_xlog2(long long c) {
  if (c <= 0) return 0.0;
  const double x = (double)c;
  return (c & (c - 1)) == 0 ? x * (double)(63 - __clzll(c)) : x * log2(x);
}

// the feature subset of key mask m, or -1 when m cuts a bit field
__device__ __forceinline__ int dib_subset_features_of(unsigned m, const DibSubsetFeatures& ft, int F) {
  int s = 0;
  for (int f = 0; f < F; ++f) {
    const unsigned field = ((1u << ft.width[f]) - 1u) << ft.offset[f];
    const unsigned part = m & field;
    if (part == field) s |= 1 << f;
    else if (part != 0u) return -1;
  }
  return s;
}

__global__ __launch_bounds__(DIB_SUBSET_THREADS) void dib_subset_fold_kernel(
    const int* __restrict__ counts, int B, int K, int Ks, int L, DibSubsetFeatures ft, int F, int mask0, int n_masks,
    double* __restrict__ out_bits) {
  extern __shared__ __align__(16) unsigned char dib_subset_lds[];
  const int tid = threadIdx.x;
  const int nhigh = B - L;
  const unsigned lowall = (1u << L) - 1u, highall = (1u << nhigh) - 1u;
  const unsigned H = highall - blockIdx.x;   // heaviest (most bits) first
  int P3[DIB_SUBSET_MAX_LOW_BITS + 1];
  P3[0] = 1;
#pragma unroll
  for (int j = 0; j < DIB_SUBSET_MAX_LOW_BITS; ++j) P3[j + 1] = P3[j] * 3;
  int rows = 1;
  for (int j = 0; j < L; ++j) rows *= 3;

  // --- does this workgroup own any subset of the chunk?  (uniform: every lane takes the same way out, before any barrier)
  {
    int lo = 0, hi = 0;   // the smallest / largest feature subset among H | S_low
    for (int f = 0; f < F; ++f) {
      const unsigned field = ((1u << ft.width[f]) - 1u) << ft.offset[f];
      const unsigned fh = field >> L, part = H & fh;
      if (fh == 0u) { hi |= 1 << f; continue; }           // the field lies in the low bits
      if (part == fh) { lo |= 1 << f; hi |= 1 << f; }
      else if (part != 0u) return;                        // H cuts a bit field
    }
    if (hi < mask0 || lo >= mask0 + n_masks) return;
  }

  int* V = reinterpret_cast<int*>(dib_subset_lds);                   // [rows][Ks] ints, then in place a double in the first two ints of every row
  unsigned short* tern = reinterpret_cast<unsigned short*>(dib_subset_lds + (size_t)rows * Ks * 4);   // [2^L]
  long long* n_k = reinterpret_cast<long long*>(dib_subset_lds + (size_t)rows * Ks * 4 + (1 << DIB_SUBSET_MAX_LOW_BITS) * 2);   // [16]
  if (tid <= (int)lowall) {
    int t = 0;
#pragma unroll
    for (int j = 0; j < DIB_SUBSET_MAX_LOW_BITS; ++j) t += ((tid >> j) & 1) * P3[j];
    tern[tid] = (unsigned short)t;
  }
  if (tid < 16) n_k[tid] = 0;

  // this lane's low subset, its feature subset and where it stores
  const int my_subset = tid <= (int)lowall ? dib_subset_features_of((H << L) | (unsigned)tid, ft, F) : -1;
  const bool mine = my_subset >= mask0 && my_subset < mask0 + n_masks;
  double acc = 0.0;
  const unsigned dropped = highall & ~H;
  const int entries = K << L;
  __syncthreads();

  unsigned h = 0;
  do {
    // --- build: U[l][k] over the dropped high bits, into the rows with binary digits
    for (int e = tid; e < entries; e += DIB_SUBSET_THREADS) {
      int sum = 0;
      unsigned d = 0;
      do {
        sum += counts[(size_t)((h | d) << L) * K + e];
        d = (d - dropped) & dropped;
      } while (d != 0u);
      const int l = e / K, k = e - l * K;
      V[(int)tern[l] * Ks + k] = sum;
    }
    __syncthreads();
    // --- fold: digit j of every row from {0, 1} to {0, 1, 2}
#pragma unroll
    for (int j = 0; j < DIB_SUBSET_MAX_LOW_BITS; ++j) {
      if (j < L) {
        const int p = P3[j], items = p << (L - 1 - j);
        for (int w = tid; w < items; w += DIB_SUBSET_THREADS) {
          const int q = w / p, r = w - q * p;
          const int base = (r + 3 * p * (int)tern[q]) * Ks;
          for (int k = 0; k < K; ++k) V[base + 2 * p * Ks + k] = V[base + k] + V[base + p * Ks + k];
        }
        __syncthreads();
      }
    }
    // --- terms: each row becomes its float64 term, in place (a row is read and written by one lane)
    for (int t = tid; t < rows; t += DIB_SUBSET_THREADS) {
      long long tot = 0;
      double parts = 0.0;
      for (int k = 0; k < K; ++k) {
        const int c = V[t * Ks + k];
        tot += c;
        parts += dib_subset_xlog2(c);
        if (t == rows - 1) n_k[k] += c;
      }
      const double term = dib_subset_xlog2(tot) - parts;
      V[t * Ks] = __double2loint(term);
      V[t * Ks + 1] = __double2hiint(term);
    }
    __syncthreads();
    // --- gather: lane S_low sums the rows with digit 2 exactly outside S_low, patterns ascending
    if (mine) {
      const unsigned S = (unsigned)tid;
      const int star = 2 * (int)tern[lowall & ~S];
      double sum = 0.0;
      unsigned a = 0;
      do {
        const int* row = V + (star + (int)tern[a]) * Ks;
        sum += __hiloint2double(row[1], row[0]);
        a = (a - S) & S;
      } while (a != 0u);
      acc += sum;
    }
    __syncthreads();
    h = (h - H) & H;
  } while (h != 0u);

  if (mine) {
    long long n = 0;
    double parts = 0.0;
    for (int k = 0; k < K; ++k) {
      n += n_k[k];
      parts += dib_subset_xlog2(n_k[k]);
    }
    const double e0 = dib_subset_xlog2(n) - parts, dn = (double)n;
    out_bits[my_subset - mask0] = (my_subset == 0 || n <= 0) ? 0.0 : e0 / dn - acc / dn;
  }
}
