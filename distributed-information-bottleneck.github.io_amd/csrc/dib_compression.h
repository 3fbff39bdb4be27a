// dib_compression.h - every feature's compression-scheme matrix of a DistributedIBNet in one evaluation
// (include/dib_compression.h): exp(-Bhattacharyya distance) between the Gaussians of each feature's display sample, for all
// features of a feature-major encoding [F][plane_rows][2E] - the encoder bank's DIB_WS_ENC_OUT - in ONE launch, and the gather
// that builds that forward's input (feature f on its own display rows) in one more.
//
// dib_cmp_matrices_kernel: grid (upper-triangular pairs (I <= J) of 64-row tiles, features), 256 threads; thread (ty, tx) owns the
// 4 x 4 pairs (i0 + ty + 16 a, j0 + tx + 16 b) - a wave reads 4 distinct rows of the I tile (broadcasts) and 16 of the J tile, at an
// odd pitch: no bank conflicts.  The dimensions pass through LDS in chunks of 16: (mu, v = e^logvar, l = ln v) of the 64 + 64 rows,
// the exponential taken ONCE per staged element (dib_bhattacharyya_kernel takes both of every (pair, dimension): 2 n^2 E against
// 2 n E here per tile pair).  l is the logarithm of the ROUNDED variance, not the logvar that was read: the pair term
// ln((v_i + v_j) / 2) - (l_i + l_j) / 2 is then exactly 0 for a row against itself or a duplicate (the same logf of the same
// float; unit diagonal of exp(-D)), and the rounding of expf drops out of every pair to first order - with the raw logvar it
// stayed as an absolute 2^-24 however small the terms were.  Per pair the two sums run over e = 0 .. E-1 in that order in one
// accumulator each, whatever the chunking, with dib_bhattacharyya_kernel's expressions - all of them commutative in (i, j) - so
// the diagonal tiles are bit-symmetric by arithmetic and the off-diagonal tiles by construction: the J x I mirror is the same
// registers, transposed through LDS for coalesced stores.  Rows >= counts[f] are never loaded; their pairs, and whole tiles beyond
// counts[f], are stored as 0.0f.  A pair's bits depend on (E, its two rows) alone.
#pragma once
#include "dib_common.h"

#define DIB_CMP_THREADS 256
#define DIB_CMP_TILE 64
#define DIB_CMP_CHUNK 16
#define DIB_CMP_PITCH (DIB_CMP_CHUNK + 1)

// xg[i][k] = x[clamp(rows[f(k)][i])][k]: one thread per element of xg [n_max][sum_d]; colmap[k].x = the feature of column k
__global__ void __launch_bounds__(256)
dib_cmp_gather_kernel(const float* __restrict__ x, long long ldx, long long n_rows, const int* __restrict__ rows, int n_max,
                      const int4* __restrict__ colmap, int sum_d, float* __restrict__ xg) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)n_max * sum_d) return;
  const int i = (int)(idx / sum_d), k = (int)(idx - (long long)i * sum_d);
  long long r = rows[(long long)colmap[k].x * n_max + i];
  r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
  xg[idx] = x[r * ldx + k];
}

__global__ void __launch_bounds__(DIB_CMP_THREADS)
dib_cmp_matrices_kernel(const float* __restrict__ enc, long long plane_rows, long long row0, int E, const int* __restrict__ counts,
                        int n_max, float* __restrict__ dist, float* __restrict__ comp) {
  constexpr int T = DIB_CMP_TILE, C = DIB_CMP_CHUNK, P = DIB_CMP_PITCH;
  // [side: I / J tile][mu, var, ln var][row][P]; afterwards the [T][T + 1] transpose buffer of the mirror
  __shared__ float sm[2][3][T * P];
  static_assert(sizeof(sm) >= (size_t)T * (T + 1) * sizeof(float), "the mirror's transpose buffer lives in the staging tiles");
  const int f = blockIdx.y, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int nt = (n_max + T - 1) / T;
  int p = blockIdx.x, I = 0;
  while (p >= nt - I) { p -= nt - I; ++I; }   // row I of the upper triangle has nt - I tile pairs
  const int J = I + p, i0 = I * T, j0 = J * T;
  const int cnt = min(max(counts[f], 0), n_max);

  float t1[4][4], t2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) t1[a][b] = t2[a][b] = 0.f;

  if (j0 < cnt) {   // (i0 <= j0) a tile with pairs inside the feature's sample; uniform over the workgroup
    const float* plane = enc + ((long long)f * plane_rows + row0) * 2 * E;
    for (int e0 = 0; e0 < E; e0 += C) {
      const int ec = min(C, E - e0);
      for (int s = tid; s < 2 * T * C; s += DIB_CMP_THREADS) {
        const int side = s / (T * C), r = (s / C) % T, e = s % C;
        const int row = (side ? j0 : i0) + r;
        float mu = 0.f, lv = 0.f;
        if (row < cnt && e < ec) {
          const float* q = plane + (long long)row * 2 * E + e0 + e;
          mu = q[0];
          lv = q[E];
        }
        sm[side][0][r * P + e] = mu;
        const float var = expf(lv);
        sm[side][1][r * P + e] = var;
        sm[side][2][r * P + e] = logf(var);
      }
      __syncthreads();
#pragma unroll 2
      for (int e = 0; e < ec; ++e) {
        float am[4], av[4], al[4], bm[4], bv[4], bl[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          am[a] = sm[0][0][(ty + 16 * a) * P + e]; av[a] = sm[0][1][(ty + 16 * a) * P + e]; al[a] = sm[0][2][(ty + 16 * a) * P + e];
          bm[a] = sm[1][0][(tx + 16 * a) * P + e]; bv[a] = sm[1][1][(tx + 16 * a) * P + e]; bl[a] = sm[1][2][(tx + 16 * a) * P + e];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float sb = 0.5f * (av[a] + bv[b]);
            const float d = am[a] - bm[b];
            t1[a][b] += d * d / sb;
            t2[a][b] += logf(sb) - 0.5f * (al[a] + bl[b]);
          }
      }
      __syncthreads();
    }
  }

  float(*tile)[T + 1] = reinterpret_cast<float(*)[T + 1]>(&sm[0][0][0]);
  const long long fo = (long long)f * n_max * n_max;
  for (int which = 0; which < 2; ++which) {
    float* out = which ? comp : dist;
    if (!out) continue;
    out += fo;
    float v[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
        const float d = 0.125f * t1[a][b] + 0.5f * t2[a][b];
        v[a][b] = (i < cnt && j < cnt) ? (which ? expf(-d) : d) : 0.f;
        if (i < n_max && j < n_max) out[(long long)i * n_max + j] = v[a][b];
      }
    if (I != J) {   // the mirror tile (J, I): rows of it are columns of this one
      __syncthreads();
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) tile[ty + 16 * a][tx + 16 * b] = v[a][b];
      __syncthreads();
      const int c = tid & (T - 1);
      for (int r = tid / T; r < T; r += DIB_CMP_THREADS / T)
        if (j0 + r < n_max && i0 + c < n_max) out[(long long)(j0 + r) * n_max + i0 + c] = tile[c][r];
    }
  }
}
