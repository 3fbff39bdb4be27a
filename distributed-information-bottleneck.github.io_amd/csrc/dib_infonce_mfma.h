// dib_infonce_mfma.h - the InfoNCE similarity matrix and its embedding gradients on the gfx950 matrix cores.
//
// reference: train.py:203-215 (eval_batch_infonce: S = similarity(emb_x, emb_y) / T, loss = mean_i CE(i, S[i,:]) +
// mean_j CE(j, S[:,j])), utils.py:131-175 (get_scaled_similarity), utils.py:75-90 (pairwise squared distances as
// |a|^2 + |b|^2 - 2 a.b^T, clamped at 0).  Default similarity of the reference: 'l2' (train.py:57-58).
//
// For the three similarities built on the dot product - l2sq, l2, cosine - everything that is O(B^2 D) is a matrix product:
//   S-tile     ab = X Y^T                                [B, B]   K = D          dib_infonce_sim_mfma_kernel
//   g_x        C Y      with C_ij   = coefficient(S_ij)  [B, D]   K = B          dib_infonce_grad_mfma_kernel (side 0)
//   g_y        C^T X                                     [B, D]   K = B          dib_infonce_grad_mfma_kernel (side 1)
// (round 3 evaluated all three on the VALU: 0.38 ms of the 0.73 ms step at B = 2048, D = 64.)  l1 / linf are not bilinear
// and stay on the VALU kernels of dib_elementwise.h.
//
// With w_ij = dL/d(unscaled similarity)_ij = (softmax_row_i(S)_ij + softmax_col_j(S)_ij - 2 delta_ij) / (B T) the gradient wrt
// the row's own embedding a (partner b) is
//   l2sq   c = -2 w            (0 where the clamp max(d2, 0) is active)       g_a = sum_b c (a - b)  =  a R - C b,   R = sum_b c
//   l2     c = -w / r,  r = sqrt(d2 + 1e-9) = -S T  (0 where d2 = 0)          same form
//   cosine c = w / (|a||b|),  c2 = w sim / |a|^2                               g_a = C b - a R,               R = sum_b c2
// so each side is one product C . Other (MFMA) plus one row sum R (VALU, alongside the coefficient evaluation).
//
// Launches (all deterministic: fixed-order partials, the one atomic is an arrival counter):
//   sim    64 x 64 tile of S per workgroup (4 waves x one 32 x 32 MFMA tile, K chunks of 64 through LDS).  The row norms come
//          out of the staged tiles (sum of squares of what each thread stages, 16-lane DPP reduction); epilogue = norm /
//          -2ab / sqrt / 1/T, S written once; per (row, 32-column block) and per (column, 32-row block) partial
//          (max, sum exp) from the accumulator registers: along a column in-lane + one cross-half swizzle, along a row a
//          16-lane DPP butterfly + one swizzle (the first version's 162 ds_bpermute per tile were most of the kernel)
//   lse    combine the partials: lse_r[i], lse_c[j]; the LAST workgroup to finish (arrival counter) adds up the loss
//   grad   workgroup = 64 "self" rows x a slice of the partner tiles x side; per partner tile: read the S tile (side 1:
//          transposed through LDS), evaluate the coefficients, G += C . Other on the MFMAs, R += row sums.  With one slice
//          (B <= 256) the epilogue writes g = alpha self R + beta G itself; else partial G, R per slice and
//   final  g = alpha self R + beta G, slices summed in a fixed order
// = 3 launches at the reference's default batch of 128 (6 in the first version), 4 from B = 320.
#pragma once
#include "dib_common.h"
#include "dib_gemm.h"   // dib_f32x16, DIB_MFMA
#include "dib_fused.h"  // dib_f32x4, DIB_MFMA16

#define DIB_INCE_TS 64          // tile edge
#define DIB_INCE_KP 68          // LDS pitch of a k-contiguous operand tile (b128 fragment reads: conflict-free at BK + 4)
#define DIB_INCE_CP 65          // LDS pitch of the coefficient tile (odd: conflict-free for row-wise and transposed stores)

// ---- cross-lane helpers: DPP within a row of 16 lanes, ds_swizzle across the two rows of a 32-lane half ----
template <int CTRL>
__device__ __forceinline__ float dib_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float dib_swz_xor16(float v) {   // lane ^ 16 (bit-mask mode: and 0x1f, or 0, xor 0x10)
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));
}
// reductions over the 32 lanes of a half-wave (all 32 get the result): quad_perm xor 1, xor 2, row_half_mirror, row_mirror
// (symmetric reductions: a mirror pairs what an xor would), then the other row of 16
__device__ __forceinline__ float dib_half_max(float v) {
  v = fmaxf(v, dib_dpp<0xB1>(v));
  v = fmaxf(v, dib_dpp<0x4E>(v));
  v = fmaxf(v, dib_dpp<0x141>(v));
  v = fmaxf(v, dib_dpp<0x140>(v));
  return fmaxf(v, dib_swz_xor16(v));
}
__device__ __forceinline__ float dib_half_sum(float v) {
  v += dib_dpp<0xB1>(v);
  v += dib_dpp<0x4E>(v);
  v += dib_dpp<0x141>(v);
  v += dib_dpp<0x140>(v);
  return v + dib_swz_xor16(v);
}
__device__ __forceinline__ float dib_row16_sum(float v) {   // over the 16 lanes of a DPP row
  v += dib_dpp<0xB1>(v);
  v += dib_dpp<0x4E>(v);
  v += dib_dpp<0x141>(v);
  return v + dib_dpp<0x140>(v);
}

// S_ij from the dot product.  KIND: 0 l2sq, 1 l2, 4 cosine.
template <int KIND>
__device__ __forceinline__ float dib_ince_similarity(float ab, float na, float nb, float inv_t) {
  float s;
  if (KIND == 4) {
    s = ab / (sqrtf(na) * sqrtf(nb));
  } else {  // utils.py:85-90: max(|a|^2 + |b|^2 - 2 a.b, 0)
    const float d2 = fmaxf(na + nb - 2.0f * ab, 0.f);
    s = (KIND == 0) ? -d2 : -sqrtf(d2 + 1e-9f);
  }
  return s * inv_t;
}

// grid (ceil(B/64) column tiles, ceil(B/64) row tiles), 256 threads.
// prow: [2][nb32][B] (plane 0 max, plane 1 sum of exp(s - max)) over the 32-column block cb of row i;  pcol: same for columns.
// norms [2B] (|x_i|^2, then |y_j|^2) is an OUTPUT: written by the first tile column / row, read by the gradient kernel.
// arrive: the log-sum-exp kernel's arrival counter, reset here (this launch precedes it on the stream).
template <int KIND>
__global__ void __launch_bounds__(256)
dib_infonce_sim_mfma_kernel(const float* __restrict__ X, const float* __restrict__ Y, int B, int D, float inv_t,
                            float* __restrict__ norms, float* __restrict__ S, float* __restrict__ prow,
                            float* __restrict__ pcol, int nb32, unsigned* __restrict__ arrive) {
#define DIB_INCE_BODY 1
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

// lse[0][i] = LSE_j S[i][j], lse[1][j] = LSE_i S[i][j] from the 32-wide block partials; the workgroup that arrives last (all
// lse values are then in memory) adds up loss = (1/B) sum_i (lse_r[i] + lse_c[i] - 2 S_ii) from one partial per workgroup
// (each workgroup sums lse - S_tt over its own 32 rows or columns).
// grid ceil(2B / 32): a workgroup owns 32 rows (or columns), thread (row = tid & 31, part = tid >> 5) merges every 8th block
// partial online - (m, s) <- (max(m, pm), s e^(m - m') + ps e^(pm - m')) - and the 8 parts of a row are merged in a fixed
// order through LDS.  (One thread per row walking all 2 x 64 partials of B = 2048 in two dependent passes took 47 us on 16
// workgroups - 40 % of the whole InfoNCE sequence, profiles/r04c_infonce_kernel_stats.csv.)
__global__ void __launch_bounds__(256)
dib_infonce_lse_loss_kernel(const float* __restrict__ prow, const float* __restrict__ pcol, const float* __restrict__ S, int B,
                            int nb32, float* __restrict__ lse, unsigned* __restrict__ arrive, float* __restrict__ lpart,
                            float* __restrict__ loss_out) {
#define DIB_INCE_BODY 2
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

// grid (ceil(B/64) self blocks, nsplit partner slices, 2 sides), 256 threads, dynamic LDS (DIB_INCE_TS * (64 NACC + 4)) floats
// for the partner tile.  side 0: self = x rows, partners = y rows, coefficient tile read along rows of S; side 1: self = y
// rows, partners = x rows, the S tile is read along its rows (coalesced) and stored TRANSPOSED into the coefficient tile.
// nsplit == 1: GX / GY written directly; else Gp [2][nsplit][B][D], Rp [2][nsplit][B] for dib_infonce_grad_final_kernel.
template <int NACC, int KIND>
__global__ void __launch_bounds__(256)
dib_infonce_grad_mfma_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ S,
                             const float* __restrict__ lse, const float* __restrict__ norms, int B, int D, float inv_t,
                             float temperature, int nsplit, float* __restrict__ Gp, float* __restrict__ Rp,
                             float* __restrict__ GX, float* __restrict__ GY) {
#define DIB_INCE_BODY 3
#define DIB_INCE_GRAD_SIDE blockIdx.z
#include "dib_infonce_bodies.h"
#undef DIB_INCE_GRAD_SIDE
#undef DIB_INCE_BODY
}

// g = alpha self R + beta G with the slices summed in a fixed order.  One thread per (side, row, coordinate).
__global__ void __launch_bounds__(256)
dib_infonce_grad_final_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Gp,
                              const float* __restrict__ Rp, int B, int D, int kind, int nsplit, float* __restrict__ GX,
                              float* __restrict__ GY) {
#define DIB_INCE_BODY 4
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

// =====================================================================================================================
// One launch for the reference's DEFAULT batch (train.py:34: 128 rows, shared space 64, train.py:60): B <= 128, D <= 64.
// The three launches above spend 39 us on 2 MFLOP at that size (profiles/r05i_config2_loop_kernel_stats_b128.csv: similarity
// 12.3, log-sum-exp + loss 6.4, gradients 19.9 us - each a dependent launch of a handful of workgroups).  Here every
// workgroup keeps BOTH embedding sets and the whole [128][128] similarity matrix in its CU's LDS (136 KB of the 160) and
// recomputes S and the 2 B log-sum-exps itself - 8192 MFMA cycles per SIMD, cheaper than any exchange between workgroups -
// then evaluates the gradient of ITS 64 self rows of one side: grid (ceil(B/64) self blocks, 2 sides); without gradients (the
// validation pass) one workgroup.  512 threads = 2 waves per SIMD: the square roots / exponentials of one wave run under the
// MFMAs of the other (with 4 waves the phases ran back to back: S 11.6 us of which 3.7 are MFMAs, profiles/r05r_*).  The
// coefficient matrix overwrites S in place (side 1 reads it transposed: the LDS pitch is odd, so row-wise and column-wise
// accesses are both conflict-free).  Same expressions as the kernels above except v_sqrt_f32 / v_rsq_f32 (1 ulp) for the
// IEEE sqrtf / division sequences; every sum in a fixed order.  Workgroup (0, 0) writes the loss.
// =====================================================================================================================
#define DIB_INCE1_MAXB 128
#define DIB_INCE1_THREADS 512
#define DIB_INCE1_SP 129          // pitch of the similarity / coefficient matrix
#define DIB_INCE1_LDS_FLOATS (2 * DIB_INCE1_MAXB * DIB_INCE_KP + DIB_INCE1_MAXB * DIB_INCE1_SP + 4 * DIB_INCE1_MAXB + 4 * 256 + 8 * 64 + 64 + 8)

template <int KIND>
__device__ __forceinline__ float dib_ince1_similarity(float ab, float na, float nb, float inv_t) {
  if (KIND == 4) return ab * __builtin_amdgcn_rsqf(na) * __builtin_amdgcn_rsqf(nb) * inv_t;
  const float d2 = fmaxf(na + nb - 2.0f * ab, 0.f);   // utils.py:85-90
  return ((KIND == 0) ? -d2 : -__builtin_amdgcn_sqrtf(d2 + 1e-9f)) * inv_t;
}

template <int KIND>
__global__ void __launch_bounds__(DIB_INCE1_THREADS)
dib_infonce_small_kernel(const float* __restrict__ X, const float* __restrict__ Y, int B, int D, float inv_t, float temperature,
                         float* __restrict__ GX, float* __restrict__ GY, float* __restrict__ loss_out) {
#define DIB_INCE_BODY 5
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

// =====================================================================================================================
// R independent problems [R][B][D] in the launches of one (dib_infonce_fwd_bwd_batched).  The replica is the grid index the
// single kernels leave free - z for the similarity and the one-launch kernel, y for the log-sum-exp and the final kernel, the
// upper bits of z (z = 2 r + side) for the gradient kernel.  A workgroup moves every pointer to its replica's slice -
// embeddings and gradients r B D floats on, the workspace (S, partials, lse, norms, arrival counter, slice partials)
// `ws_stride` floats on, the loss one float on - and runs the single kernel's body (csrc/dib_infonce_bodies.h): the same tiles,
// the same fixed-order sums, one arrival counter per replica, no workgroup waiting on another.
// =====================================================================================================================
template <int KIND>
__global__ void __launch_bounds__(256)
dib_infonce_batched_sim_kernel(const float* __restrict__ X_, const float* __restrict__ Y_, int B, int D, float inv_t,
                               float* __restrict__ norms_, float* __restrict__ S_, float* __restrict__ prow_,
                               float* __restrict__ pcol_, int nb32, unsigned* __restrict__ arrive_, long long ws_stride) {
  const long long e_ = (long long)blockIdx.z * B * D, w_ = (long long)blockIdx.z * ws_stride;
  const float* __restrict__ X = X_ + e_;
  const float* __restrict__ Y = Y_ + e_;
  float* __restrict__ norms = norms_ + w_;
  float* __restrict__ S = S_ + w_;
  float* __restrict__ prow = prow_ + w_;
  float* __restrict__ pcol = pcol_ + w_;
  unsigned* __restrict__ arrive = arrive_ + w_;
#define DIB_INCE_BODY 1
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

__global__ void __launch_bounds__(256)
dib_infonce_batched_lse_loss_kernel(const float* __restrict__ prow_, const float* __restrict__ pcol_,
                                    const float* __restrict__ S_, int B, int nb32, float* __restrict__ lse_,
                                    unsigned* __restrict__ arrive_, float* __restrict__ lpart_, float* __restrict__ loss_out_,
                                    long long ws_stride) {
  const long long w_ = (long long)blockIdx.y * ws_stride;
  const float* __restrict__ prow = prow_ + w_;
  const float* __restrict__ pcol = pcol_ + w_;
  const float* __restrict__ S = S_ + w_;
  float* __restrict__ lse = lse_ + w_;
  unsigned* __restrict__ arrive = arrive_ + w_;
  float* __restrict__ lpart = lpart_ + w_;
  float* __restrict__ loss_out = loss_out_ + blockIdx.y;
#define DIB_INCE_BODY 2
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

template <int NACC, int KIND>
__global__ void __launch_bounds__(256)
dib_infonce_batched_grad_kernel(const float* __restrict__ X_, const float* __restrict__ Y_, const float* __restrict__ S_,
                                const float* __restrict__ lse_, const float* __restrict__ norms_, int B, int D, float inv_t,
                                float temperature, int nsplit, float* __restrict__ Gp_, float* __restrict__ Rp_,
                                float* __restrict__ GX_, float* __restrict__ GY_, long long ws_stride) {
  const long long e_ = (long long)(blockIdx.z >> 1) * B * D, w_ = (long long)(blockIdx.z >> 1) * ws_stride;
  const float* __restrict__ X = X_ + e_;
  const float* __restrict__ Y = Y_ + e_;
  const float* __restrict__ S = S_ + w_;
  const float* __restrict__ lse = lse_ + w_;
  const float* __restrict__ norms = norms_ + w_;
  float* __restrict__ Gp = Gp_ + w_;
  float* __restrict__ Rp = Rp_ + w_;
  float* __restrict__ GX = GX_ + e_;
  float* __restrict__ GY = GY_ + e_;
#define DIB_INCE_BODY 3
#define DIB_INCE_GRAD_SIDE (blockIdx.z & 1)
#include "dib_infonce_bodies.h"
#undef DIB_INCE_GRAD_SIDE
#undef DIB_INCE_BODY
}

__global__ void __launch_bounds__(256)
dib_infonce_batched_grad_final_kernel(const float* __restrict__ X_, const float* __restrict__ Y_, const float* __restrict__ Gp_,
                                      const float* __restrict__ Rp_, int B, int D, int kind, int nsplit,
                                      float* __restrict__ GX_, float* __restrict__ GY_, long long ws_stride) {
  const long long e_ = (long long)blockIdx.y * B * D, w_ = (long long)blockIdx.y * ws_stride;
  const float* __restrict__ X = X_ + e_;
  const float* __restrict__ Y = Y_ + e_;
  const float* __restrict__ Gp = Gp_ + w_;
  const float* __restrict__ Rp = Rp_ + w_;
  float* __restrict__ GX = GX_ + e_;
  float* __restrict__ GY = GY_ + e_;
#define DIB_INCE_BODY 4
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}

template <int KIND>
__global__ void __launch_bounds__(DIB_INCE1_THREADS)
dib_infonce_batched_small_kernel(const float* __restrict__ X_, const float* __restrict__ Y_, int B, int D, float inv_t,
                                 float temperature, float* __restrict__ GX_, float* __restrict__ GY_,
                                 float* __restrict__ loss_out_) {
  const long long e_ = (long long)blockIdx.z * B * D;
  const float* __restrict__ X = X_ + e_;
  const float* __restrict__ Y = Y_ + e_;
  float* __restrict__ GX = GX_ ? GX_ + e_ : nullptr;   // both NULL: the losses only
  float* __restrict__ GY = GY_ ? GY_ + e_ : nullptr;
  float* __restrict__ loss_out = loss_out_ + blockIdx.z;
#define DIB_INCE_BODY 5
#include "dib_infonce_bodies.h"
#undef DIB_INCE_BODY
}
