// dib_gemm_stream.h - LDS-free forward / dgrad GEMM for large batches: global memory -> registers -> matrix cores.
//
//   MODE 0 (fwd)   C[M,N] = act( A[M,K] @ B[K,N] + bias[N] )          (MODE 0 / 1's contract of dib_gemm.h, one group)
//   MODE 1 (dgrad) C[M,N] = ( A[M,K] @ B[N,K]^T ) * act'(aux[M,N])
//
// The wave shape of dib_wgrad_stream.h: a wave owns one 128 x 128 output tile (16 accumulators = 256 AGPRs), a workgroup is four
// independent waves, one per SIMD; no LDS, no barrier, no ds_read.  Operand maps - MFMA step t of k-block q contracts
// k = 8q + 4h + t on half-wave h, the tiled kernel's pairing:
//   activation (rows = batch, k contiguous): for m-sub-tile i lane (l31, h) loads A[m0 + 32 i + l31][8q + 4h .. + 3], one 16-byte
//       load whose four floats are its A values of steps t = 0..3;
//   weight, MODE 0 ([K, N], n contiguous): for step t the lane loads B[8q + 4h + t][n0 + 4 l31 .. + 3]: the four floats belong to
//       four n-sub-tiles, sub-tile j owning COLUMN n0 + 4 l31 + j (any consistent permutation of the n axis is legal);
//   weight, MODE 1 ([N, K], k contiguous): sub-tile j again owns column n0 + 4 l31 + j, the lane loads B[n0 + 4 l31 + j][8q + 4h .. + 3].
// 8 loads feed the 64 MFMAs of a k-block.  Accumulator (i, j), register r of lane (l31, h) is
// C[m0 + 32 i + (r & 3) + 8 (r >> 2) + 4h][n0 + 4 l31 + j]: j = 0..3 is ONE 16-byte store (and one 16-byte load of the dgrad's
// mask), a half-wave writes a whole 512-byte row.
//
// Bits: accumulators start at zero, k-blocks ascend, t ascends, one accumulator per output element, the tiled kernel's epilogue
// arithmetic: the outputs are bit-identical to dib_gemm_kernel<MODE, ...>'s.  (Only the order WITHIN an accumulator's chain is
// the contract; the order between accumulators is free - used below.)
//
// Prefetch.  An activation load touches 32 bytes of each of 32 rows: the four k-blocks of one 128-byte line are loaded back to
// back (a "line group": 4 loads), so a line is fetched from L2 once; the same holds for MODE 1's weight rows.  The unit of the
// ring is therefore a SUPER-BLOCK of 32 k (4 k-blocks) = 256 MFMAs in eight phases of 32: phase p multiplies m-sub-tile i = p & 3
// with the n-sub-tile PAIR jp = p >> 2 over all four k-blocks (two accumulators alternate).  Everything is single-buffered,
// 128 registers like dib_wgrad_stream.h's ring:
//   the weights of pair 0 are free after phase 3 and refilled for the next super-block during phases 4 and 5;
//   the weights of pair 1 are free at the super-block's end and refilled for THIS super-block during phases 0 and 1;
//   the line group of sub-tile i is free after phase 4 + i and refilled one phase later (sub-tile 3: in phase 0, for this
//   super-block): every load is at least 64 MFMAs, the line groups 96, ahead of its use.
// MODE 0's weight loads are 8 bytes (one pair's two columns of a row), four rows of a k-block per group.  Loads are pinned with
// sched_barrier pairs as in dib_wgrad_stream.h; none is conditional, so the compiler's s_waitcnt vmcnt counting stays exact.
//
// Several tiles per wave: a wave walks a contiguous range of tiles (n fastest: all n-tiles of an m-tile back to back, the ranges
// of one XCD contiguous), and the ring simply runs on into the next tile's first super-block - its loads are in flight while
// the finished tile is stored.  The last super-block of the last tile re-reads itself.
#pragma once
#include "dib_gemm.h"

typedef float dib_gs_f4 __attribute__((ext_vector_type(4)));
typedef float dib_gs_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ dib_gs_f4 dib_gs_load(const char* p) { return *reinterpret_cast<const dib_gs_f4*>(p); }

// KIND: the epilogue's activation, a template parameter because the epilogue is unrolled over all 1024 elements of a lane and
//   nothing runs beside it on this SIMD - it must be straight-line code (a uniform branch between copies makes the compiler hoist
//   the accumulator reads above it and spill them).  Only activations that are a compare and a multiply run here (linear, relu, the
//   two leaky relus: the host's eligibility rule), with dib_act's / dib_act_grad's arithmetic for them:
//     0: nothing;  1 (MODE 0): fmaxf(z, 0);  2 (MODE 0): z > 0 ? z : slope z;  3 (MODE 1): v *= (y > 0 ? 1 : slope), y = aux
// nts: non-temporal output stores (the host's rule: streamed launches with outputs of 256 MB and more).  The activation loads are
// ALWAYS plain: a non-temporal load bypasses the L1, and the L1 is what serves the second to fourth load of a line group (the
// stand-alone loop at B = 65536: non-temporal loads 5-6 % slower than plain on all four launches, profiles/HISTORY.md section 27)
// grid.x workgroups of four waves; `nwaves` (<= tiles) waves share tiles_m x tiles_n tiles, wave v owning tiles
// [v tiles / nwaves, (v + 1) tiles / nwaves)
template <int MODE, int KIND>
__global__ void __launch_bounds__(256, 1)
dib_gemm_stream_kernel(const DibGemmGroup* __restrict__ groups, const float* __restrict__ Abase, const float* __restrict__ Bbase,
                       float* __restrict__ Cbase, const float* __restrict__ bias, const float* __restrict__ aux, int batch, int act,
                       int tiles_m, int tiles_n, int nwaves, int nts) {
  static_assert((MODE == 0 && KIND >= 0 && KIND <= 2) || (MODE == 1 && (KIND == 0 || KIND == 3)), "forward and dgrad; the weight gradient is dib_wgrad_stream.h");
  typedef dib_gs_f4 f4v;
  typedef dib_gs_f2 f2v;
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // consecutive workgroup ids sit on consecutive XCDs (id % 8): XCD x takes the x-th eighth of the waves, so the n-tiles of
  // an m-tile (and the waves that share one) read the activation rows through one L2
  const unsigned nwg = gridDim.x, wg = blockIdx.x;
  const unsigned v = ((nwg & 7u) == 0u ? (wg & 7u) * (nwg >> 3) + (wg >> 3) : wg) * 4u + wave;
  if (v >= (unsigned)nwaves) return;   // wave-uniform
  const unsigned tiles = (unsigned)tiles_m * (unsigned)tiles_n;
  unsigned tile = (unsigned)((unsigned long long)v * tiles / (unsigned)nwaves);
  const unsigned tend = (unsigned)((unsigned long long)(v + 1u) * tiles / (unsigned)nwaves);
  if (tile >= tend) return;
  const DibGemmGroup g = groups[0];
  const int K = g.K < 0 ? batch : g.K;
  const int nsb = K >> 5;   // super-blocks (K % 32 == 0, M % 128 == 0, N % 128 == 0: the host's eligibility rule)

  // addresses: a per-lane pointer of the tile + a uniform 32-bit byte offset (the host keeps a tile's operand extents below
  // 2^31 bytes), as in dib_wgrad_stream.h
  const char* Ag = reinterpret_cast<const char*>(Abase + g.a_off + g.a_boff * batch);
  const char* Bg = reinterpret_cast<const char*>(Bbase + g.b_off + g.b_boff * batch);
  const unsigned rowA = (unsigned)g.lda * 4u, rowB = (unsigned)g.ldb * 4u, subA = 32u * rowA;
  const unsigned laneA = (unsigned)l31 * rowA + 16u * (unsigned)h;
  const unsigned laneB = MODE == 0 ? 4u * (unsigned)h * rowB + 16u * (unsigned)l31 : 4u * (unsigned)l31 * rowB + 16u * (unsigned)h;
  auto a_base = [&](unsigned t) { return Ag + (size_t)(t / (unsigned)tiles_n) * 128u * (size_t)rowA + (size_t)laneA; };
  auto b_base = [&](unsigned t) {
    const size_t n0 = (size_t)(t % (unsigned)tiles_n) * 128u;
    return Bg + (MODE == 0 ? n0 * 4u : n0 * (size_t)rowB) + (size_t)laneB;
  };

  f4v a[4][4];         // [m-sub-tile i][k-block q]: steps t = 0..3
  f4v bw1[4][4];       // MODE 1: [n-sub-tile j][q]: steps t = 0..3
  f2v bw0[2][4][4];    // MODE 0: [pair jp][q][t]: sub-tiles 2 jp, 2 jp + 1
  auto load_a = [&](int i, const char* p, unsigned sb) {   // the line group of sub-tile i
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a[i][q] = dib_gs_load(p + (size_t)((unsigned)i * subA + 128u * sb) + 32 * q);
  };
  // half hf (0 / 1) of pair jp's weights.  MODE 1: the line group of sub-tile 2 jp + hf; MODE 0: k-blocks 2 hf, 2 hf + 1
  auto load_b = [&](int jp, int hf, const char* p, unsigned sb) {
    if (MODE == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        bw1[2 * jp + hf][q] = dib_gs_load(p + (size_t)((unsigned)(2 * jp + hf) * rowB + 128u * sb) + 32 * q);
    } else {
#pragma unroll
      for (int qq = 0; qq < 2; ++qq)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          bw0[jp][2 * hf + qq][t] = *reinterpret_cast<const f2v*>(p + (size_t)((32u * sb + (unsigned)(8 * (2 * hf + qq) + t)) * rowB) + 8 * jp);
    }
  };

  const char* pA = a_base(tile);
  const char* pB = b_base(tile);
  // (the loop's own order: at the loop's top the compiler waits for the OLDEST loads of either way in; any other order here, the
  // scheduler's included, makes every trip wait for its youngest loads)
  load_b(0, 0, pB, 0u);
  __builtin_amdgcn_sched_barrier(0);
  load_a(0, pA, 0u);
  __builtin_amdgcn_sched_barrier(0);
  load_b(0, 1, pB, 0u);
  __builtin_amdgcn_sched_barrier(0);
  load_a(1, pA, 0u);
  __builtin_amdgcn_sched_barrier(0);
  load_a(2, pA, 0u);
  __builtin_amdgcn_sched_barrier(0);

  char* Cg = reinterpret_cast<char*>(Cbase + g.c_off + g.c_boff * batch);
  const char* auxg = KIND == 3 ? reinterpret_cast<const char*>(aux + g.aux_off + g.aux_boff * batch) : nullptr;
  const unsigned rowC = (unsigned)g.ldc * 4u, rowX = (unsigned)g.ldaux * 4u;
  const float slope = act == 1 ? 0.0f : (act == 2 ? 0.2f : (act == 7 ? 0.1f : 1.0f));   // (KIND 2 / 3)
  const unsigned laneC = 4u * (unsigned)h * rowC + 16u * (unsigned)l31, laneX = 4u * (unsigned)h * rowX + 16u * (unsigned)l31;

#pragma unroll 1
  for (; tile < tend; ++tile) {
    const unsigned tnext = min(tile + 1u, tend - 1u);
    const bool more = tile + 1u < tend;
    const char* pA1 = a_base(tnext);
    const char* pB1 = b_base(tnext);
    dib_f32x16 acc[4][4];   // (a tile's own: carried around the tile loop, the accumulators change registers at its back edge)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int S = 0;
#pragma unroll 1
    do {   // (nsb >= 1: a zero-trip path would hand the epilogue a second, all-zero source of its 256 accumulators)
      // where the ring reads ahead: the next super-block of this tile, the first of the next tile, or (the very end) itself
      const bool last = S + 1 == nsb;
      const char* pAn = last ? pA1 : pA;
      const char* pBn = last ? pB1 : pB;
      const unsigned Sn = last ? (more ? 0u : (unsigned)S) : (unsigned)S + 1u;
#pragma unroll
      for (int ph = 0; ph < 8; ++ph) {
        const int jp = ph >> 2, i = ph & 3;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              const int j = 2 * jp + jj;
              acc[i][j] = DIB_MFMA(a[i][q][t], MODE == 0 ? bw0[jp][q][t][jj] : bw1[j][q][t], acc[i][j]);
            }
            const int step = 4 * q + t;
            const bool la = step == 0 && (ph == 0 || ph >= 5);
            const bool lb = (step == 4 && (ph == 0 || ph == 1 || ph == 4 || ph == 5));
            if (la || lb) {
              __builtin_amdgcn_sched_barrier(0);   // (without the pair the scheduler sinks every load to its use)
              if (la) {
                if (ph == 0) load_a(3, pA, (unsigned)S);   // (its slot was in use until the last phase; for THIS super-block)
                else load_a(ph - 5, pAn, Sn);
              } else {
                if (ph < 2) load_b(1, ph, pB, (unsigned)S);   // (pair 1: for this super-block)
                else load_b(0, ph - 4, pBn, Sn);
              }
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
      }
    } while (++S < nsb);

    // ---- epilogue: per (i, r) one 16-byte store per lane, a full row of the tile per half-wave; the arithmetic of
    // dib_gemm_kernel's LDS epilogue ----
    const size_t m0 = (size_t)(tile / (unsigned)tiles_n) * 128u, n0 = (size_t)(tile % (unsigned)tiles_n) * 128u;
    char* cp = Cg + m0 * rowC + n0 * 4u + (size_t)laneC;
    f4v bv = 0.f;
    if (MODE == 0 && bias != nullptr && g.bias_off >= 0) {
      const float* bp = bias + g.bias_off + n0 + 4 * l31;
      bv = f4v{bp[0], bp[1], bp[2], bp[3]};
    }
    const char* xp = KIND == 3 ? auxg + m0 * rowX + n0 * 4u + (size_t)laneX : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        f4v x[4], o[4];
        if (KIND == 3) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) x[rr] = dib_gs_load(xp + (size_t)((unsigned)(32 * i + 8 * rg + rr) * rowX));
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = 4 * rg + rr;
          o[rr] = f4v{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
          if (MODE == 0) o[rr] += bv;
          // (an untouched value may be stored straight from accumulator registers: the compiler then shuffles accumulators into
          // 4-register store operands, two moves per value and spills; through a vector register it is one read)
          if (MODE == 1 && KIND == 0) asm volatile("" : "+v"(o[rr]));
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (KIND == 1) o[rr][j] = fmaxf(o[rr][j], 0.0f);
            else if (KIND == 2) o[rr][j] = o[rr][j] > 0.0f ? o[rr][j] : slope * o[rr][j];
            else if (KIND == 3) o[rr][j] *= x[rr][j] > 0.0f ? 1.0f : slope;
          }
        }
        if (nts) {   // uniform
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            __builtin_nontemporal_store(o[rr], reinterpret_cast<f4v*>(cp + (size_t)((unsigned)(32 * i + 8 * rg + rr) * rowC)));
        } else {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            *reinterpret_cast<f4v*>(cp + (size_t)((unsigned)(32 * i + 8 * rg + rr) * rowC)) = o[rr];
        }
        __builtin_amdgcn_sched_barrier(0);   // (one group at a time: the scheduler otherwise reads far ahead and spills)
      }
    }
    pA = pA1;
    pB = pB1;
  }
}
