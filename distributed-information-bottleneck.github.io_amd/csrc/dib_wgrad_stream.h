// dib_wgrad_stream.h - LDS-free weight gradient for 128-row-wide operands: global memory -> registers -> matrix cores.
//
//   C[M,N] = A[Kb,M]^T @ B[Kb,N]  (+ column sums of B), per group and batch slab        (MODE 2's contract of dib_gemm.h)
//
// Both operands of a weight gradient are contracted over the batch, so a row of A and a row of B ARE the operand vectors of
// one contraction index.  In v_mfma_f32_32x32x2_f32 lane (l31, h) supplies the A value of output row l31 and the B value of
// output column l31 for contraction index h, and any consistent permutation of the m / n axis over sub-tiles is legal.  So
// lane (l31, h) loads A[row_h][m0 + 4 l31 .. + 3] with ONE 16-byte load: the four floats are its A operands of four sub-tiles,
// sub-tile t owning m = m0 + 4 i + t (i = the MFMA's row index).  The same for B.  Two loads per lane feed 16 MFMAs: a wave owns
// a full 128 x 128 output tile (16 accumulators = 256 AGPRs) - 128 x 64 with 8-byte B loads for a 64-wide output - of one
// (group, slab); each half-wave reads one whole 512-byte row per load instruction.  No LDS, no barrier, no ds_read; waves
// never talk to each other, a workgroup is four independent waves, one per SIMD (the register budget allows no second).
//
// Contraction order = dib_gemm_kernel<2, ...>'s: 8-row block by 8-row block, MFMA step t = 0..3 contracts rows 8q + t (h = 0)
// and 8q + 4 + t (h = 1).  With the same slab partition every output element sees the same fmaf chain: the slabs are
// bit-identical to the tiled kernel's.
//
// Prefetch: a register ring of kWgsGroups 8-row blocks (4 steps each).  While block g is multiplied, step t of block
// g + kWgsGroups - 1 is loaded into the slot block g - 1 has just left (one block of slack: the bias sums below read a
// block's B values once more at its end).  Loads past the slab's end re-read its last block (no branch in the loop: the
// compiler's s_waitcnt vmcnt counting stays exact).
//
// Bias (column sums of B, tm == 0 only): the tiled kernel sums a column as PARTS chains, chain p = rows p RPP .. + RPP - 1 of
// every K-tile in row order, carried across K-tiles, and adds the chains at the end (PARTS x RPP = 2 x 32 of a 64-deep tile
// for 128-column tiles, 4 x 8 of a 32-deep tile for the 64-column tile).  Here a chain's rows alternate between the half
// waves - h = 0 holds rows 8q .. 8q + 3, h = 1 rows 8q + 4 .. 8q + 7 - so the running sum changes sides twice per block: the
// additions happen in the tiled kernel's order and the bias rows are bit-identical too.
#pragma once
#include "dib_gemm.h"

constexpr int kWgsGroups = 4;               // ring depth in 8-row blocks
constexpr int kWgsRing = 4 * kWgsGroups;    // ... in MFMA steps (row pairs): 16 steps x 2 KB per wave in flight

// both halves of a wave exchange v (lane <-> lane ^ 32)
__device__ __forceinline__ float dib_wgs_swap_halves(float v) { return __shfl_xor(v, 32, 64); }

// NT: output columns per lane (4: 128-column tile, 16-byte B loads; 2: 64-column tile, 8-byte B loads)
// CH: bias chains per column, those of the tiled kernel this launch would otherwise be: 2 (its 128-column tiles: chain p = blocks
//     4p .. 4p + 3 of every 64 rows) or 4 (its 64-column tiles: chain p = block p of every 32 rows)
// NTL: non-temporal operand loads (the host's stream_rows rule)
// grid.x = ceil(waves / 4), wave index = ((slab * count + group) * tiles_m + tm) * tiles_n + tn
template <int NT, int CH, bool NTL>
__global__ void __launch_bounds__(256, 1)
dib_wgrad_stream_kernel(const DibGemmGroup* __restrict__ groups, const float* __restrict__ Abase,
                        const float* __restrict__ Bbase, float* __restrict__ Cbase, float* __restrict__ bias_out, int batch,
                        int count, int tiles_m, int tiles_n, int nsplit, int rows_per_split, long long split_stride) {
  static_assert((NT == 4 && (CH == 2 || CH == 4)) || (NT == 2 && CH == 4), "128- or 64-column tiles; the tiled kernels' bias chains");
  static_assert(kWgsGroups == 4, "the bias chains below are laid out for a ring of four 8-row blocks");
  constexpr int G = kWgsGroups;
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef float fbv __attribute__((ext_vector_type(NT)));
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned wid = blockIdx.x * 4u + (unsigned)wave;   // (the host keeps the wave count below 2^31)
  const unsigned tiles = (unsigned)(tiles_m * tiles_n);
  if (wid >= tiles * (unsigned)count * (unsigned)nsplit) return;   // wave-uniform
  const int tile = (int)(wid % tiles);
  const int grp = (int)((wid / tiles) % (unsigned)count), slab = (int)(wid / (tiles * (unsigned)count));
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const DibGemmGroup g = groups[grp];
  const int M = g.M < 0 ? batch : g.M;
  const int N = g.N < 0 ? batch : g.N;
  const int K = g.K < 0 ? batch : g.K;
  const int m0 = tm * 128, n0 = tn * (32 * NT);
  if (m0 >= M || n0 >= N) return;   // (M % 128 == 0, N % (32 NT) == 0: the host's eligibility rule)
  const int kbeg = slab * rows_per_split;
  const int nblk = max(0, min(K, kbeg + rows_per_split) - kbeg) >> 3;   // whole 64-row K-tiles: a multiple of 8 (and of G)

  // lane (l31, h) of MFMA step t of block q reads row kbeg + 8 q + 4 h + t: a per-lane pointer + a uniform 32-bit byte offset
  // (the host keeps a slab's operand extent below 2^31 bytes)
  const char* pA = reinterpret_cast<const char*>(Abase + g.a_off + g.a_boff * batch + (long long)(kbeg + 4 * h) * g.lda + m0 + 4 * l31);
  const char* pB = reinterpret_cast<const char*>(Bbase + g.b_off + g.b_boff * batch + (long long)(kbeg + 4 * h) * g.ldb + n0 + NT * l31);
  const unsigned rowA = (unsigned)g.lda * 4u, rowB = (unsigned)g.ldb * 4u;

  dib_f32x16 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // bias chains: CH == 2: x[0] = the chain of the four blocks being walked, x[1] the other (they change places every four
  // blocks); CH == 4: block q belongs to chain q % 4
  fbv x[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) x[c] = 0.f;

  f4v ra[G][4];
  fbv rb[G][4];
  auto load_step = [&](int slot, int blk, int t) {
    const f4v* pa = reinterpret_cast<const f4v*>(pA + (size_t)((unsigned)(8 * blk + t) * rowA));
    const fbv* pb = reinterpret_cast<const fbv*>(pB + (size_t)((unsigned)(8 * blk + t) * rowB));
    if (NTL) {
      ra[slot][t] = __builtin_nontemporal_load(pa);
      rb[slot][t] = __builtin_nontemporal_load(pb);
    } else {
      ra[slot][t] = *pa;
      rb[slot][t] = *pb;
    }
  };
  if (nblk > 0) {
#pragma unroll
    for (int j = 0; j < G - 1; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) load_step(j, j, t);   // (nblk >= 8 > G - 1)
  }
#pragma unroll 1
  for (int q0 = 0; q0 < nblk; q0 += G) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int pf = min(q0 + j + G - 1, nblk - 1);   // uniform
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f4v a = ra[j][t];
        const fbv b = rb[j][t];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int u = 0; u < NT; ++u) acc[i][u] = DIB_MFMA(a[i], b[u], acc[i][u]);
        __builtin_amdgcn_sched_barrier(0);   // (without the pair the scheduler sinks every load to its use: no prefetch left)
        load_step((j + G - 1) % G, pf, t);
        __builtin_amdgcn_sched_barrier(0);
      }
      // column sums: rows 8q .. 8q+3 on the h = 0 side, hand over, rows 8q+4 .. 8q+7 on the h = 1 side, hand back
      fbv& xc = x[CH == 2 ? 0 : j];
      fbv y = xc;
#pragma unroll
      for (int t = 0; t < 4; ++t) y += rb[j][t];
#pragma unroll
      for (int u = 0; u < NT; ++u) y[u] = dib_wgs_swap_halves(y[u]);
#pragma unroll
      for (int t = 0; t < 4; ++t) y += rb[j][t];
#pragma unroll
      for (int u = 0; u < NT; ++u) xc[u] = dib_wgs_swap_halves(y[u]);   // meaningful on the h = 0 side only
    }
    if (CH == 2) {
      const fbv s = x[0];
      x[0] = x[1];
      x[1] = s;
    }
  }

  // ---- epilogue.  C/D map of the 32x32 MFMA: column index = lane & 31, row index = (r & 3) + 8 (r >> 2) + 4 (lane >> 5);
  // here row index i means m = m0 + 4 i + (sub-tile), column index j means n = n0 + NT j + u: per (sub-tile, r) one NT-float
  // store per lane, a full row of the tile per half-wave ----
  const long long coff = g.c_off + g.c_boff * batch + (long long)slab * split_stride;
  float* Cg = Cbase + coff;
  const bool vecC = ((coff | (long long)g.ldc) & (NT - 1)) == 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + i;
      float* cp = Cg + (long long)m * g.ldc + n0 + NT * l31;
      fbv v;
#pragma unroll
      for (int u = 0; u < NT; ++u) v[u] = acc[i][u][r];
      if (vecC) {
        *reinterpret_cast<fbv*>(cp) = v;
      } else {
#pragma unroll
        for (int u = 0; u < NT; ++u) cp[u] = v[u];
      }
    }
  }
  if (bias_out != nullptr && g.bias_off >= 0 && tm == 0 && h == 0) {
    // (CH == 2: nblk is a multiple of 8, an even number of 4-block walks: x[0] is chain 0 again)
    fbv s = x[0];
#pragma unroll
    for (int c = 1; c < CH; ++c) s += x[c];
    float* bp = bias_out + g.bias_off + (long long)slab * split_stride + n0 + NT * l31;
#pragma unroll
    for (int u = 0; u < NT; ++u) bp[u] = s[u];
  }
}
