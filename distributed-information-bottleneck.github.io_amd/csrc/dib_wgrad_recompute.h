// dib_wgrad_recompute.h - the encoder layer-2 weight gradient dW2 = h1^T dh2 with h1 RECOMPUTED in registers instead of read.
//
// The sibling of dib_wgrad_stream_kernel<4, CH, NTL> (dib_wgrad_stream.h) with the same contract - a wave = one 128 x 128 tile of
// one (group, slab), the same slab partition and row order (8-row blocks, MFMA step t contracts rows 8q + t | 8q + 4 + t), the
// same bias chains, the same epilogue, the B operand (dh2) streamed through the same register ring - and one difference: the A
// ring is not loaded.  h1 = act(P W1 + b1) has a 5-wide input (in_dim <= 8 here), so a 32 x 32 tile of it costs four
// v_mfma_f32_32x32x2_f32, 1/16 of the 64 MFMAs that consume it, and the fused forward (dib_fused.h) need not write h1 at all:
// 2.15 GB of the headline step's HBM writes and as many of this kernel's reads.
//
// The bits are the forward's.  The forward evaluates the transposed product, A = W1^T, B = p, C = b1, step t contracting
// k = t (h = 0) and k = 4 + t (h = 1), zero-padded to k < 8, then dib_act_tile.  Here, per sub-tile u = 0 .. 3, lane (l31, h)
// supplies A = P[row0 + l31][4 h + t] and B = W1[4 h + t][m0 + 4 l31 + u] with C = b1[m0 + 4 l31 + u] in every register: the same
// products (multiplication commutes) in the same k pairing and order on the same C.  After the four steps register r of lane
// (l31, h) holds h1[row0 + 8 (r >> 2) + 4 h + (r & 3)][m0 + 4 l31 + u] before activation: exactly the A operand of ring block
// q = r >> 2, step t = r & 3, sub-tile u of the stream kernel.  One 32-row tile of h1 is one trip around the ring of four blocks.
//
// Pipeline: while the tile of rows 32 T .. + 31 ("cur", 64 VGPRs) feeds the 256 MFMAs of trip T, the 16 MFMAs of tile T + 1 run in
// "nxt" (64 VGPRs), four after every main step of the trip's first block (four independent chains, a link every 20 MFMAs), from
// P values loaded during trip T - 1; then the activation and the copy nxt -> cur, block by block behind cur's last reader.
#pragma once
#include "dib_fused.h"
#include "dib_wgrad_stream.h"

// per group (= feature) of the launch, what the recompute reads; built by dib_layout_create, uploaded with the layout's tables
struct DibWgradH1Side {
  long long p_boff;    // the group's P block [B][in_dim] (pitch in_dim floats) starts at P + p_boff * batch (dib_fused.h load_p)
  long long w1_off;    // W1 [in_dim][H1] in params
  long long b1_off;    // b1 [H1] in params
  int in_dim;          // <= 8
  int act;             // DIB_ACT_*: the slope is dib_neg_slope(act), as in the forward (relu: the launch picks the forward's RELU
                       // specialisation)
};

// One 8-row block of the bias chains (dib_wgrad_stream_kernel's, as a function): x = the running column sums of this block's chain, rb =
// the block's four B rows of this lane.  Rows 8q .. 8q+3 are summed on the h = 0 side, handed over, rows 8q+4 .. 8q+7 on the
// h = 1 side, handed back (meaningful on the h = 0 side only).
// dib_wgrad_stream_kernel keeps its inline copy (and dib_wgh_epilogue's) on purpose: calling these from it changes the generated code of
// all six instantiations (<4, 2, *>: 142 -> 144 VGPRs, 588 -> 590 loop instructions) - a GPU A/B first, not a clean-up (tools/isa_diff.py).
template <int NT, typename FBV>
__device__ __forceinline__ void dib_wgh_bias_block(FBV& xc, const FBV (&rb)[4]) {
  FBV y = xc;
#pragma unroll
  for (int t = 0; t < 4; ++t) y += rb[t];
#pragma unroll
  for (int u = 0; u < NT; ++u) y[u] = dib_wgs_swap_halves(y[u]);
#pragma unroll
  for (int t = 0; t < 4; ++t) y += rb[t];
#pragma unroll
  for (int u = 0; u < NT; ++u) xc[u] = dib_wgs_swap_halves(y[u]);
}

// Epilogue (dib_wgrad_stream_kernel's, as a function).  C/D map of the 32x32 MFMA: column index = lane & 31, row index = (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5); here row index i means m = m0 + 4 i + (sub-tile), column index j means n = n0 + NT j + u: per
// (sub-tile, r) one NT-float store per lane, a full row of the tile per half-wave.  Then the bias row: the sum of the chains.
template <int NT, int CH, typename FBV>
__device__ __forceinline__ void dib_wgh_epilogue(const DibGemmGroup& g, const dib_f32x16 (&acc)[4][NT], const FBV (&x)[CH],
                                                 float* __restrict__ Cbase, float* __restrict__ bias_out, int batch, int slab,
                                                 long long split_stride, int m0, int n0, int tm, int l31, int h) {
  const long long coff = g.c_off + g.c_boff * batch + (long long)slab * split_stride;
  float* Cg = Cbase + coff;
  const bool vecC = ((coff | (long long)g.ldc) & (NT - 1)) == 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + i;
      float* cp = Cg + (long long)m * g.ldc + n0 + NT * l31;
      FBV v;
#pragma unroll
      for (int u = 0; u < NT; ++u) v[u] = acc[i][u][r];
      if (vecC) {
        *reinterpret_cast<FBV*>(cp) = v;
      } else {
#pragma unroll
        for (int u = 0; u < NT; ++u) cp[u] = v[u];
      }
    }
  }
  if (bias_out != nullptr && g.bias_off >= 0 && tm == 0 && h == 0) {
    // (CH == 2: nblk is a multiple of 8, an even number of 4-block walks: x[0] is chain 0 again)
    FBV s = x[0];
#pragma unroll
    for (int c = 1; c < CH; ++c) s += x[c];
    float* bp = bias_out + g.bias_off + (long long)slab * split_stride + n0 + NT * l31;
#pragma unroll
    for (int u = 0; u < NT; ++u) bp[u] = s[u];
  }
}

// Step t of the recompute: nxt[u] += p * w[u] for the four sub-tiles, accumulators in VGPRs.  Inline assembly because hipcc picks ONE
// form for every MFMA of a function: with the 256 output accumulators in AGPRs it gives these four the AGPR form too, and with no
// AGPR left shuttles their 64 accumulator registers through v_accvgpr_* and scratch (measured: 2501 v_accvgpr_read, 1092 bytes of
// scratch).  The compiler inserts no wait states around instructions it cannot see, so the callers keep the hazards of the ISA
// guide (4.5) away by construction: a chain's links are four MFMAs apart (SrcC = vDst of the previous link), and no VALU touches
// nxt for at least 19 wait states after the last link - in the loop a whole block of 64 MFMAs, in the prologue dib_wgh_settle.
__device__ __forceinline__ void dib_wgh_mfma_step(dib_f32x16 (&nxt)[4], float p, const float (&w)[4]) {
  asm volatile("s_nop 1\n\t"
               "v_mfma_f32_32x32x2_f32 %0, %4, %5, %0\n\t"
               "v_mfma_f32_32x32x2_f32 %1, %4, %6, %1\n\t"
               "v_mfma_f32_32x32x2_f32 %2, %4, %7, %2\n\t"
               "v_mfma_f32_32x32x2_f32 %3, %4, %8, %3"
               : "+v"(nxt[0]), "+v"(nxt[1]), "+v"(nxt[2]), "+v"(nxt[3])
               : "v"(p), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]));
}
// the last link's 16 passes before a VALU may read nxt
__device__ __forceinline__ void dib_wgh_settle(dib_f32x16 (&nxt)[4]) {
  asm volatile("s_nop 15\n\ts_nop 15" : "+v"(nxt[0]), "+v"(nxt[1]), "+v"(nxt[2]), "+v"(nxt[3]));
}

// CH, NTL: dib_wgrad_stream_kernel's; RELU: the fused forward's (act == 1).  grid.x = ceil(waves / 4), wave index = ((slab * count + group) * tiles_m + tm) * tiles_n + tn
template <int CH, bool NTL, bool RELU>
__global__ void __launch_bounds__(256, 1)
dib_wgrad_h1_kernel(const DibGemmGroup* __restrict__ groups, const DibWgradH1Side* __restrict__ side,
                    const float* __restrict__ Pbase, const float* __restrict__ params, const float* __restrict__ Bbase,
                    float* __restrict__ Cbase, float* __restrict__ bias_out, int batch, int count, int tiles_m, int tiles_n,
                    int nsplit, int rows_per_split, long long split_stride) {
  static_assert(CH == 2 || CH == 4, "the tiled kernels' bias chains");
  static_assert(kWgsGroups == 4, "one recomputed 32-row tile = one trip around a ring of four 8-row blocks");
  constexpr int G = kWgsGroups, NT = 4;
  typedef float f4v __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned wid = blockIdx.x * 4u + (unsigned)wave;   // (the host keeps the wave count below 2^31)
  const unsigned tiles = (unsigned)(tiles_m * tiles_n);
  if (wid >= tiles * (unsigned)count * (unsigned)nsplit) return;   // wave-uniform
  const int tile = (int)(wid % tiles);
  const int grp = (int)((wid / tiles) % (unsigned)count), slab = (int)(wid / (tiles * (unsigned)count));
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const DibGemmGroup g = groups[grp];
  const DibWgradH1Side sd = side[grp];
  const int M = g.M < 0 ? batch : g.M;
  const int N = g.N < 0 ? batch : g.N;
  const int K = g.K < 0 ? batch : g.K;
  const int m0 = tm * 128, n0 = tn * 128;
  if (m0 >= M || n0 >= N) return;   // (M % 128 == 0, N % 128 == 0: the host's eligibility rule)
  const int kbeg = slab * rows_per_split;
  const int nblk = max(0, min(K, kbeg + rows_per_split) - kbeg) >> 3;   // whole 64-row K-tiles: a multiple of 8 (and of G)
  const int ntile = nblk >> 2;                                          // 32-row tiles of h1

  // Every address below is a wave-uniform 64-bit base + a 32-bit per-lane offset (the host keeps a slab's operand extent below
  // 2^31 bytes): one VGPR per stream instead of a 64-bit pointer and a 64-bit sum per load - this kernel has no register to spare.
  // lane (l31, h) of MFMA step t of block q reads row kbeg + 8 q + 4 h + t of B
  const char* uB = reinterpret_cast<const char*>(Bbase + g.b_off + g.b_boff * batch + (long long)kbeg * g.ldb + n0);
  const unsigned rowB = (unsigned)g.ldb * 4u;
  // (lh, ll: the lane's h and l31, made opaque once per trip - or every per-lane address is hoisted out of the loop as a loop
  // invariant, two VGPRs each, and spilled)
  int lh = h, ll = l31;

  // ---- the recompute's constants: W1[4 h + t][m0 + 4 l31 .. + 3] (zero from in_dim up, like the forward's staged image), resident
  // - a load inside the loop that is used soon after makes its s_waitcnt drain the B ring's prefetch with it - and b1 ----
  const int in_dim = sd.in_dim;
  float w1[4][4];   // [t][u]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = 4 * h + t;
    const float* W1 = params + sd.w1_off + (long long)min(k, in_dim - 1) * M + m0 + 4 * l31;
#pragma unroll
    for (int u = 0; u < 4; ++u) w1[t][u] = (k < in_dim) ? W1[u] : 0.f;
  }
  const char* ub1 = reinterpret_cast<const char*>(params + sd.b1_off + m0);
  float b1v[4];   // (re-read every trip at the head of block 2, behind the B loads the next trip's start waits for anyway: dead while
                  // blocks 0 and 1 need every register)
  auto load_b1 = [&](int u) { b1v[u] = *reinterpret_cast<const float*>(ub1 + 4 * u + (size_t)((unsigned)(4 * ll) * 4u)); };
#pragma unroll
  for (int u = 0; u < 4; ++u) load_b1(u);
  // lane (l31, h) supplies P[row0 + l31][4 h + t] of tile T: the forward's clamped, masked load (dib_fused.h load_p)
  const char* uP = reinterpret_cast<const char*>(Pbase + sd.p_boff * batch + (long long)kbeg * in_dim);
  const unsigned rowsP = 32u * (unsigned)in_dim * 4u;   // bytes per 32-row tile
  // (the mask is applied where the value is used, a trip later: next to the load its s_waitcnt would drain the B ring's prefetch)
  auto load_p = [&](int T, int t, float (&dst)[4]) {
    const unsigned off = (unsigned)(ll * in_dim + min(4 * lh + t, in_dim - 1)) * 4u;
    dst[t] = *reinterpret_cast<const float*>(uP + (size_t)((unsigned)T * rowsP) + (size_t)off);
  };
  auto mask_p = [&](float (&p)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) p[t] = (4 * lh + t < in_dim) ? p[t] : 0.f;
  };
  const float slope = dib_neg_slope(sd.act);
  auto act_tile = [&](dib_f32x16& v) { dib_act_tile<RELU>(slope, v); };

  dib_f32x16 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // bias chains, as in dib_wgrad_stream_kernel
  f4v x[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) x[c] = 0.f;

  f4v rb[G][4];
  auto load_step = [&](int slot, int blk, int t) {
    const unsigned laneB = (unsigned)(4 * lh) * rowB + (unsigned)(NT * ll) * 4u;
    const f4v* pb = reinterpret_cast<const f4v*>(uB + (size_t)((unsigned)(8 * blk + t) * rowB) + (size_t)laneB);
    if (NTL) rb[slot][t] = __builtin_nontemporal_load(pb);
    else rb[slot][t] = *pb;
  };

  float cur[4][16];    // [u][r]: the h1 tile being multiplied (scalars: each is the A operand of four MFMAs)
  dib_f32x16 nxt[4];   // [u]: the tile being recomputed
  float pn[4];         // P values of the tile recomputed next
  if (nblk > 0) {
    // (the P loads first: were they the youngest loads here, the loop's first s_waitcnt - placed for both ways into the loop -
    // would be vmcnt(0) and drain the ring once per trip)
    float p0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      load_p(0, t, p0);
      load_p(1, t, pn);   // (ntile >= 2)
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < G - 1; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        load_step(j, j, t);   // (nblk >= 8 > G - 1)
        __builtin_amdgcn_sched_barrier(0);   // in the order of use, for the same reason
      }
    mask_p(p0);
    // tile 0 (the only copy of the recompute outside the loop)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) nxt[u][r] = b1v[u];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      dib_wgh_mfma_step(nxt, p0[t], w1[t]);
    }
    dib_wgh_settle(nxt);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      act_tile(nxt[u]);
#pragma unroll
      for (int r = 0; r < 16; ++r) cur[u][r] = nxt[u][r];
    }
  }
#pragma unroll 1
  for (int q0 = 0; q0 < nblk; q0 += G) {
    const int Tnn = min((q0 >> 2) + 2, ntile - 1);   // uniform; past the slab's end the last tile is recomputed again, unused
    asm volatile("" : "+v"(lh), "+v"(ll));
    mask_p(pn);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) nxt[u][r] = b1v[u];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int pf = min(q0 + j + G - 1, nblk - 1);   // uniform
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f4v b = rb[j][t];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int u = 0; u < NT; ++u) acc[i][u] = DIB_MFMA(cur[i][4 * j + t], b[u], acc[i][u]);
        if (j == 0) dib_wgh_mfma_step(nxt, pn[t], w1[t]);   // the next tile: step t of its four sub-tiles
        __builtin_amdgcn_sched_barrier(0);   // (as in dib_wgrad_stream_kernel: keeps the prefetch a prefetch)
        if (j == 2 && t == 0) {
#pragma unroll
          for (int u = 0; u < 4; ++u) load_b1(u);
        }
        load_step((j + G - 1) % G, pf, t);
        if (j == 1) load_p(Tnn, t, pn);   // (block 0 was pn's last reader)
        __builtin_amdgcn_sched_barrier(0);
      }
      dib_wgh_bias_block<NT>(x[CH == 2 ? 0 : j], rb[j]);
      // activation, then the copy nxt -> cur behind the last reader of cur's registers 4 j .. 4 j + 3 (block 0's wait for block
      // 1: the recompute has only just been issued)
      if (j >= 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j == 1) act_tile(nxt[u]);
#pragma unroll
          for (int r = (j == 1 ? 0 : 4 * j); r < 4 * j + 4; ++r) cur[u][r] = nxt[u][r];
        }
      }
    }
    if (CH == 2) {
      const f4v s = x[0];
      x[0] = x[1];
      x[1] = s;
    }
  }

  dib_wgh_epilogue<NT, CH>(g, acc, x, Cbase, bias_out, batch, slab, split_stride, m0, n0, tm, l31, h);
}
