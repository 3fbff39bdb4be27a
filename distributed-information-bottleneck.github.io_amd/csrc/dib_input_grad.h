// dib_input_grad.h - dL/dx of the encoder bank (include/dib_hip.h dib_encoder_bank_input_grad): the first encoder layer's
// gradient toward its inputs and the backward of the positional encoding (reference models.py:22-23), in one launch over
// (row tiles, features).
//
//   G_f  [B, H]            dL/d(pre-activation of encoder layer 0) of feature f (feature-major, like every encoder activation)
//   dP_f = G_f W1_f^T      [B, n_blocks d_f]: the gradient of P_f = [x_f, sin(2 x_f), ..., sin(2^(n_blocks-1) x_f)] (blockwise)
//   dx[b, c0_f + q] = dP_f[b, q] + sum_{j >= 1} 2^j cos(2^j x[b, c0_f + q]) dP_f[b, j d_f + q]
//
// Layout of dib_measure.h: the product runs TRANSPOSED on v_mfma_f32_16x16x4_f32, a wave owns 16 rows (lane & 15) and an output
// tile holds 16 outputs, 4 (lane >> 4) + reg of them in each lane.  The output tiles are cut BY POSITIONAL-ENCODING BLOCK: tile j
// of the column chunk q0 holds dP_f[row, j d_f + q0 + m], m < 16, so a lane ends up with every block of its four x columns
// q0 + 4 (lane >> 4) + reg in registers and the cosine chain needs no exchange.  Rows m >= d_f - q0 of a tile are zero weights.
// W1^T is packed into LDS per workgroup, one float4 per lane and MFMA group: [k tile][block][g][m][e] =
// W1[(j0 + block) d_f + q0 + m][16 k + 4 g + e], zero-padded; a first layer too wide for the LDS budget is walked in chunks of
// k tiles, more than DIB_IG_NB blocks in groups, more than 16 columns of x in chunks - the packing is then redone per step (the
// weights come from L2), otherwise once per workgroup, which walks its row tiles with a grid stride.
// Every dx element has one owner lane: no atomics, a fixed summation order.  Exact fp32 operands; the forward takes the accurate
// sinf of the fp32 product 2^j x, so this takes the accurate cosf of the same product (|2^j x| reaches 100 and beyond).
#pragma once
#include "dib_measure.h"

#define DIB_IG_THREADS 256   // 4 waves, 16 rows each
#define DIB_IG_WAVES (DIB_IG_THREADS / 64)
#define DIB_IG_NB 8          // positional-encoding blocks held as accumulators at once (32 VGPRs)
#define DIB_IG_LDS_FLOATS 16384   // 64 KB: the packed weights of one (block group, k chunk)

struct DibInputGradArgs {
  const float* G;            // [F][batch][H]
  const float* params;
  const long long* w_off;    // [F] offset of W1_f [n_blocks d_f][H] in params
  const int4* featmap;       // [F] {d_f, in_dim_f, first column in x, .}
  const float* X;            // the forward's inputs: row b of the batch is X[row_idx ? row_idx[b] : row0 + b]
  long long ldx;
  const int* row_idx;
  long long row0;
  int batch, H, n_blocks;
  int kc;                    // k tiles (of 16 columns of G) per LDS chunk
  float* dx;                 // [batch][lddx]
  long long lddx;
};

// k tiles per chunk / dynamic LDS bytes for a first layer of H outputs and n_blocks positional-encoding blocks
__host__ __device__ inline int dib_input_grad_kc(int H, int n_blocks) {
  const int nb = n_blocks < DIB_IG_NB ? n_blocks : DIB_IG_NB, tk = dib_measure_tiles(H), fit = DIB_IG_LDS_FLOATS / (256 * nb);
  return tk < fit ? tk : fit;
}
__host__ __device__ inline long long dib_input_grad_lds_bytes(int H, int n_blocks) {
  const int nb = n_blocks < DIB_IG_NB ? n_blocks : DIB_IG_NB;
  return 256ll * nb * dib_input_grad_kc(H, n_blocks) * (long long)sizeof(float);
}

// G[row][16 kt + 4 g .. + 3] of this lane's row (zero outside the batch and the layer's width)
__device__ __forceinline__ dib_f4 dib_input_grad_load_g(const float* __restrict__ Grow, int h, int H, bool valid, bool vec) {
  dib_f4 gv = dib_f4{0.f, 0.f, 0.f, 0.f};
  if (valid) {
    if (vec) {
      if (h < H) gv = *reinterpret_cast<const dib_f4*>(Grow + h);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (h + e < H) gv[e] = Grow[h + e];
    }
  }
  return gv;
}

template <int NB>   // positional-encoding blocks per group: min(n_blocks, DIB_IG_NB)
__global__ void __launch_bounds__(DIB_IG_THREADS) dib_input_grad_kernel(DibInputGradArgs a) {
  extern __shared__ float lds[];
  const int f = blockIdx.y;
  const int4 fm = a.featmap[f];
  const int d = fm.x, c0 = fm.z, H = a.H, tk = dib_measure_tiles(H);
  const float* __restrict__ W = a.params + a.w_off[f];
  const float* __restrict__ G = a.G + (long long)f * H * a.batch;
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wave = threadIdx.x >> 6;
  const int nq = (d + 15) / 16, njg = (a.n_blocks + NB - 1) / NB, nch = (tk + a.kc - 1) / a.kc;
  const bool restage = nq * njg * nch > 1;   // more than one packing: redone at every step of the loops below
  const bool vec = (H & 3) == 0;             // rows of G are 16-byte aligned
  const int ntiles = (a.batch + 15) / 16, per_round = gridDim.x * DIB_IG_WAVES, rounds = (ntiles + per_round - 1) / per_round;
  const dib_f4* w4 = reinterpret_cast<const dib_f4*>(lds);
  bool staged = false;
  for (int it = 0; it < rounds; ++it) {   // (uniform trip counts: every wave reaches every barrier)
    const int tile = (it * gridDim.x + blockIdx.x) * DIB_IG_WAVES + wave;
    const int b = tile * 16 + m;
    const bool valid = b < a.batch;
    const long long xrow = !valid ? 0ll : a.row_idx ? (long long)a.row_idx[b] : a.row0 + b;
    const float* __restrict__ Grow = G + (long long)(valid ? b : 0) * H;
    for (int qc = 0; qc < nq; ++qc) {
      const int q0 = 16 * qc + 4 * g;   // this lane's four columns of x_f: q0 .. q0 + 3
      float xv[4], dxa[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[r] = (valid && q0 + r < d) ? a.X[xrow * a.ldx + c0 + q0 + r] : 0.f;
        dxa[r] = 0.f;
      }
      for (int jg = 0; jg < njg; ++jg) {
        const int j0 = jg * NB;   // (blocks past n_blocks in the last group: zero weights)
        dib_f4 acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = dib_f4{0.f, 0.f, 0.f, 0.f};
        for (int ch = 0; ch < nch; ++ch) {
          const int k0 = ch * a.kc, nk = min(a.kc, tk - k0);
          if (restage || !staged) {
            __syncthreads();   // (the previous packing's readers are done)
            for (int idx = threadIdx.x; idx < nk * NB * 256; idx += DIB_IG_THREADS) {
              const int e = idx & 3, sm = (idx >> 2) & 15, sg = (idx >> 6) & 3, t = idx >> 8, kt = t / NB, j = t - kt * NB;
              const int q = 16 * qc + sm, h = 16 * (k0 + kt) + 4 * sg + e;
              lds[idx] = (q < d && h < H && j0 + j < a.n_blocks) ? W[((long long)(j0 + j) * d + q) * H + h] : 0.f;
            }
            __syncthreads();
            staged = true;
          }
          if (tile < ntiles) {
            dib_f4 gv = dib_input_grad_load_g(Grow, 16 * k0 + 4 * g, H, valid, vec);
            for (int kt = 0; kt < nk; ++kt) {
              const dib_f4 gn = kt + 1 < nk ? dib_input_grad_load_g(Grow, 16 * (k0 + kt + 1) + 4 * g, H, valid, vec) : gv;
              dib_f4 wv[NB];
#pragma unroll
              for (int j = 0; j < NB; ++j) wv[j] = w4[((kt * NB + j) * 4 + g) * 16 + m];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[j] = DIB_MEASURE_MFMA(wv[j][e], gv[e], acc[j]);
              }
              gv = gn;
            }
          }
        }
        // the positional encoding's derivative for blocks j0 .. j0 + NB of this lane's columns
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!valid || q0 + r >= d) continue;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            if (j0 + j >= a.n_blocks) break;
            float coef = 1.f;
            if (j0 + j > 0) {
              const float fr = ldexpf(1.f, j0 + j);
              coef = fr * cosf(fr * xv[r]);
            }
            dxa[r] = fmaf(coef, acc[j][r], dxa[r]);
          }
        }
      }
      if (valid) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (q0 + r < d) a.dx[(long long)b * a.lddx + c0 + q0 + r] = dxa[r];
      }
    }
  }
}
