// dib_partition.h - random-MLP partitions of the chaos notebook (include/dib_partition.h; Chaos_experiments.ipynb cell 7, the
// paper's Fig. 1): every point of a trajectory through an MLP [d] -> N x Dense(H, act) -> Dense(A), its symbol the index of the
// output of largest magnitude, in one launch that keeps only the byte per point (plus optional logits and a symbol histogram).
//
// Layout of dib_measure.h: every layer runs TRANSPOSED on v_mfma_f32_16x16x4_f32, a wave owns 16 points (lane & 15) and a
// layer's output tile t holds features 16 t + 4 (lane >> 4) + reg of its point, which is directly the B operand of the next
// layer; hidden and output weights are packed into LDS once per workgroup by dib_measure_stage.  The first layer (in_dim <= 4)
// is ONE k-step: lane group g holds input feature g of its point (one load per lane), and the packing of W1 is
// [out tile][g][m] = W1[g][16 ot + m] (zero for g >= in_dim), so an output tile of layer 1 is one MFMA.  Exact fp32 operands.
#pragma once
#include "dib_measure.h"

#define DIB_PARTITION_THREADS 256   // 4 waves, 16 points each: one wave per SIMD, up to 3 workgroups per CU (~145 VGPRs)
#define DIB_PARTITION_WAVES (DIB_PARTITION_THREADS / 64)
#define DIB_PARTITION_MT 8          // hidden widths up to 128: 8 tiles of 16 features in registers

struct DibPartitionArgs {
  const float *w[4], *b[4];   // Keras layout [in][out], layer n_hidden = the output layer
  const void* x;              // [n][ldx] fp32 or fp64
  int x_f64;
  long long ldx, n;
  int in_dim, n_hidden, width[4];   // width[n_hidden] = A
  uint8_t* sym;
  float* logits;                    // [n][A] or NULL
  unsigned long long* counts;       // [A] or NULL, added into
};

// floats of LDS: W1 (64 per output tile) + biases, hidden layers 2 .. N, the output layer (one tile of A <= 16 outputs)
__host__ __device__ inline long long dib_partition_lds_floats(int n_hidden, const int* width) {
  long long f = 64 * dib_measure_tiles(width[0]);
  for (int l = 1; l < n_hidden; ++l) f += 256ll * dib_measure_tiles(width[l - 1]) * dib_measure_tiles(width[l]);
  f += 256ll * dib_measure_tiles(width[n_hidden - 1]);
  for (int l = 0; l <= n_hidden; ++l) f += 16 * dib_measure_tiles(width[l]);
  return f;
}

// ACT: DIB_ACT_LINEAR / RELU / LEAKY_RELU (0.2) / TANH (accurate tanhf)
template <int ACT>
__device__ __forceinline__ float dib_partition_act(float v) {
  if (ACT == 1) return fmaxf(v, 0.f);
  if (ACT == 2) return v > 0.f ? v : 0.2f * v;
  if (ACT == 3) return tanhf(v);
  return v;
}

// y[o] = act(sum_i W[i][o] x[i] + b[o]) for output tiles o < to, input tiles i < ti (dib_measure_layer's packing)
template <int MI, int MO, int ACT>
__device__ __forceinline__ void dib_partition_layer(const float* wp, const float* bias, int ti, int to, const dib_f4 (&x)[MI],
                                                    dib_f4 (&y)[MO]) {
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
  const dib_f4* w4 = reinterpret_cast<const dib_f4*>(wp);
#pragma unroll
  for (int o = 0; o < MO; ++o) y[o] = dib_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    if (i >= ti) break;
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      if (o >= to) break;
      const dib_f4 a = w4[((i * to + o) * 4 + g) * 16 + m];
      y[o] = DIB_MEASURE_MFMA(a[0], x[i][0], y[o]);
      y[o] = DIB_MEASURE_MFMA(a[1], x[i][1], y[o]);
      y[o] = DIB_MEASURE_MFMA(a[2], x[i][2], y[o]);
      y[o] = DIB_MEASURE_MFMA(a[3], x[i][3], y[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    if (o >= to) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[o][j] = dib_partition_act<ACT>(y[o][j] + bias[16 * o + 4 * g + j]);
  }
}

// Argmax of |logit| over the A logits of a point (features 4 g .. 4 g + 3 in lane group g); the first index wins exact ties.
// A NaN logit never wins (its key is -1, below every magnitude); a point whose logits are all NaN gets symbol 0.
__device__ __forceinline__ int dib_partition_argmax_abs(const dib_f4& lg, int A) {
  const int g = (threadIdx.x & 63) >> 4;
  float bv = -1.f;
  int bi = 4 * g;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = fabsf(lg[j]);
    const float key = v == v ? v : -1.f;
    if (4 * g + j < A && key > bv) { bv = key; bi = 4 * g + j; }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  return bi;
}

template <int ACT>
__global__ void __launch_bounds__(DIB_PARTITION_THREADS, 3) dib_partition_symbolize_kernel(DibPartitionArgs a) {
  extern __shared__ float lds[];
  __shared__ int hist[16];
  const int NH = a.n_hidden, A = NH == 1 ? a.width[1] : NH == 2 ? a.width[2] : a.width[3];
  // ---- weights -> LDS (layer loops over constant bounds: no dynamically indexed arrays) ----
  int tl[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) tl[l] = l <= NH ? dib_measure_tiles(a.width[l]) : 0;
  float* wl[4];
  float* bl[4];
  wl[0] = lds;
  float* p = lds + 64 * tl[0];
#pragma unroll
  for (int l = 1; l < 4; ++l) {
    wl[l] = p;
    if (l <= NH) p += 256 * tl[l - 1] * tl[l];
  }
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    bl[l] = p;
    p += 16 * tl[l];
  }
  for (int idx = threadIdx.x; idx < 64 * tl[0]; idx += blockDim.x) {
    const int m = idx & 15, g = (idx >> 4) & 3, ot = idx >> 6, out = 16 * ot + m;
    wl[0][idx] = (g < a.in_dim && out < a.width[0]) ? a.w[0][(long long)g * a.width[0] + out] : 0.f;
  }
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (l > NH) break;
    if (l > 0) dib_measure_stage(wl[l], a.w[l], a.width[l - 1], a.width[l], false);
    dib_measure_stage_bias(bl[l], a.b[l], a.width[l]);
  }
  if (threadIdx.x < 16) hist[threadIdx.x] = 0;
  __syncthreads();
  // the output layer's weights and bias
  const float* wout = NH == 1 ? wl[1] : NH == 2 ? wl[2] : wl[3];
  const float* bout = NH == 1 ? bl[1] : NH == 2 ? bl[2] : bl[3];
  const int tlast = NH == 1 ? tl[0] : NH == 2 ? tl[1] : tl[2];

  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wave = threadIdx.x >> 6;
  const float* xf = static_cast<const float*>(a.x);
  const double* xd = static_cast<const double*>(a.x);
  const long long ntiles = (a.n + 15) / 16;
  for (long long t = (long long)blockIdx.x * DIB_PARTITION_WAVES + wave; t < ntiles; t += (long long)gridDim.x * DIB_PARTITION_WAVES) {
    const long long pt = t * 16 + m;
    const bool valid = pt < a.n;
    float x0 = 0.f;
    if (valid && g < a.in_dim) x0 = a.x_f64 ? (float)xd[pt * a.ldx + g] : xf[pt * a.ldx + g];
    // layer 1: one MFMA per output tile
    dib_f4 h[DIB_PARTITION_MT], u[DIB_PARTITION_MT];
#pragma unroll
    for (int o = 0; o < DIB_PARTITION_MT; ++o) {
      if (o >= tl[0]) break;
      h[o] = DIB_MEASURE_MFMA(wl[0][(o * 4 + g) * 16 + m], x0, (dib_f4{0.f, 0.f, 0.f, 0.f}));
#pragma unroll
      for (int j = 0; j < 4; ++j) h[o][j] = dib_partition_act<ACT>(h[o][j] + bl[0][16 * o + 4 * g + j]);
    }
    // hidden layers 2 .. N
#pragma unroll
    for (int l = 1; l < 3; ++l) {
      if (l >= NH) break;
      dib_partition_layer<DIB_PARTITION_MT, DIB_PARTITION_MT, ACT>(wl[l], bl[l], tl[l - 1], tl[l], h, u);
#pragma unroll
      for (int o = 0; o < DIB_PARTITION_MT; ++o) if (o < tl[l]) h[o] = u[o];
    }
    dib_f4 lg[1];
    dib_partition_layer<DIB_PARTITION_MT, 1, 0>(wout, bout, tlast, 1, h, lg);
    const int s = dib_partition_argmax_abs(lg[0], A);
    if (valid) {
      if (g == 0) a.sym[pt] = (uint8_t)s;
      if (a.logits) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * g + j < A) a.logits[pt * A + 4 * g + j] = lg[0][j];
      }
      if (a.counts && g == 0) atomicAdd(&hist[s], 1);
    }
  }
  if (a.counts) {
    __syncthreads();
    if ((int)threadIdx.x < A && hist[threadIdx.x] != 0) atomicAdd(a.counts + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
  }
}
