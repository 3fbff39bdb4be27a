// dib_measure.h - measurement-partition kernels of the chaos notebook (include/dib_measure.h; Chaos_experiments.ipynb cell 10):
// the VQ network between the IB encoder's (mu | logvar) and the measurement aggregator, for training (forward / backward row
// tiles over the B * L sequence states) and for symbolisation (K fixed noise draws per evaluation point, argmax, majority).
//
// Layout.  Every layer runs TRANSPOSED on v_mfma_f32_16x16x4_f32: a wave owns 16 rows (the MFMA's column index, lane & 15)
// and a layer's output tile t holds features 16 t + 4 (lane >> 4) + reg of its row - the C/D map of the instruction.  That
// tile is directly the B operand of the next layer when k-step j of lane group g contracts feature 16 t + 4 g + j, so the
// whole chain stays in registers; the weights are staged once per workgroup into LDS in the matching order, one float4 per
// lane and MFMA group ("packed": [in tile][out tile][g][m][j] = W[16 it + 4 g + j][16 ot + m], zero-padded).  The backward's
// dgrad products contract over the OUTPUT features and read the transposed packing [out tile][in tile][g][m][j] =
// W[16 it + m][16 ot + 4 g + j].  Exact fp32 (no narrowed operands), like the rest of the library.
#pragma once
#include "dib_common.h"

#define DIB_MEASURE_THREADS 512   // 8 waves, 16 rows each; one workgroup per CU at the notebook's widths (83 KB of LDS)
#define DIB_MEASURE_WAVES (DIB_MEASURE_THREADS / 64)
#define DIB_MEASURE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

typedef float dib_f4 __attribute__((ext_vector_type(4)));

struct DibMeasureArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;   // VQ network, Keras layout [in][out]
  const float* enc;                          // [rows][2E] mu | logvar
  long long rows;
  int E, H1, H2, A, L;
  float slope;                               // hidden activation: max(v, 0) + slope * min(v, 0)
  uint64_t seed;
  uint32_t step;
  // forward
  float beta, kl_exp;
  float *z, *h1s, *h2s, *soft, *out3;
  double* kl_part;
  unsigned* counter;
  // backward
  const float *h1c, *h2c, *softc, *g_agg, *w_agg0, *out3c;
  int agg_width;
  float *g3, *g2, *g1, *g_enc;
  // symbolisation
  const float* noise;
  int K;
  uint8_t* sym;
  int* counts;
};

__host__ __device__ inline int dib_measure_tiles(int w) { return (w + 15) / 16; }

// floats of LDS: the packed weights of the three layers (+ biases for the forward kernels)
__host__ __device__ inline long long dib_measure_lds_floats(int E, int H1, int H2, bool bias) {
  const long long te = dib_measure_tiles(E), t1 = dib_measure_tiles(H1), t2 = dib_measure_tiles(H2);
  long long f = 256 * (te * t1 + t1 * t2 + t2);
  if (bias) f += 16 * (t1 + t2 + 1);
  return f;
}

// W [K][N] (Keras) -> LDS, packed for the forward (T = false) or for the dgrad (T = true)
__device__ __forceinline__ void dib_measure_stage(float* dst, const float* __restrict__ W, int K, int N, bool T) {
  const int tk = dib_measure_tiles(K), tn = dib_measure_tiles(N), total = tk * tn * 256;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int j = idx & 3, m = (idx >> 2) & 15, g = (idx >> 6) & 3, t = idx >> 8;
    int in, out;
    if (!T) { in = 16 * (t / tn) + 4 * g + j; out = 16 * (t % tn) + m; }
    else { in = 16 * (t % tk) + m; out = 16 * (t / tk) + 4 * g + j; }
    dst[idx] = (in < K && out < N) ? W[(long long)in * N + out] : 0.f;
  }
}

__device__ __forceinline__ void dib_measure_stage_bias(float* dst, const float* __restrict__ b, int N) {
  const int total = dib_measure_tiles(N) * 16;
  for (int i = threadIdx.x; i < total; i += blockDim.x) dst[i] = i < N ? b[i] : 0.f;
}

// y[o] = sum_i W[i][o] x[i] (+ bias, activation) for output tiles o < to, input tiles i < ti
template <int MI, int MO>
__device__ __forceinline__ void dib_measure_layer(const float* wp, const float* bias, int ti, int to, const dib_f4 (&x)[MI],
                                                  dib_f4 (&y)[MO], float slope, bool act) {
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
    for (int j = 0; j < 4; ++j) {
      float v = y[o][j] + bias[16 * o + 4 * g + j];
      if (act) v = fmaxf(v, 0.f) + slope * fminf(v, 0.f);
      y[o][j] = v;
    }
  }
}

// dgrad: y[i] = sum_o W[i][o] x[o] for input tiles i < ti, contracting output tiles o < to (transposed packing)
template <int MO, int MI>
__device__ __forceinline__ void dib_measure_layer_t(const float* wpt, int ti, int to, const dib_f4 (&x)[MO], dib_f4 (&y)[MI]) {
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
  const dib_f4* w4 = reinterpret_cast<const dib_f4*>(wpt);
#pragma unroll
  for (int i = 0; i < MI; ++i) y[i] = dib_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    if (o >= to) break;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (i >= ti) break;
      const dib_f4 a = w4[((o * ti + i) * 4 + g) * 16 + m];
      y[i] = DIB_MEASURE_MFMA(a[0], x[o][0], y[i]);
      y[i] = DIB_MEASURE_MFMA(a[1], x[o][1], y[i]);
      y[i] = DIB_MEASURE_MFMA(a[2], x[o][2], y[i]);
      y[i] = DIB_MEASURE_MFMA(a[3], x[o][3], y[i]);
    }
  }
}

// the forward weights of all three layers; returns the pointers into LDS
struct DibMeasureLds { float *w1, *w2, *w3, *b1, *b2, *b3; };
__device__ __forceinline__ DibMeasureLds dib_measure_stage_fwd(float* lds, const DibMeasureArgs& a) {
  const int te = dib_measure_tiles(a.E), t1 = dib_measure_tiles(a.H1), t2 = dib_measure_tiles(a.H2);
  DibMeasureLds s;
  s.w1 = lds; s.w2 = s.w1 + 256 * te * t1; s.w3 = s.w2 + 256 * t1 * t2;
  s.b1 = s.w3 + 256 * t2; s.b2 = s.b1 + 16 * t1; s.b3 = s.b2 + 16 * t2;
  dib_measure_stage(s.w1, a.w1, a.E, a.H1, false);
  dib_measure_stage(s.w2, a.w2, a.H1, a.H2, false);
  dib_measure_stage(s.w3, a.w3, a.H2, a.A, false);
  dib_measure_stage_bias(s.b1, a.b1, a.H1);
  dib_measure_stage_bias(s.b2, a.b2, a.H2);
  dib_measure_stage_bias(s.b3, a.b3, a.A);
  __syncthreads();
  return s;
}

// VQ chain of one 16-row tile: z -> h1 -> h2 -> logits
template <int MT>
__device__ __forceinline__ void dib_measure_chain(const DibMeasureLds& s, const DibMeasureArgs& a, const dib_f4 (&z)[2],
                                                  dib_f4 (&h1)[MT], dib_f4 (&h2)[MT], dib_f4 (&lg)[1]) {
  const int te = dib_measure_tiles(a.E), t1 = dib_measure_tiles(a.H1), t2 = dib_measure_tiles(a.H2);
  dib_measure_layer<2, MT>(s.w1, s.b1, te, t1, z, h1, a.slope, true);
  dib_measure_layer<MT, MT>(s.w2, s.b2, t1, t2, h1, h2, a.slope, true);
  dib_measure_layer<MT, 1>(s.w3, s.b3, t2, 1, h2, lg, a.slope, false);
}

// ---- training forward: KL, reparameterisation, VQ chain, softmax -> aggregator input; stashes for the weight gradients ----
template <int MT>
__global__ void __launch_bounds__(DIB_MEASURE_THREADS) dib_measure_fwd_kernel(DibMeasureArgs a) {
#define DIB_MEASURE_BODY 1
#include "dib_measure_bodies.h"
#undef DIB_MEASURE_BODY
}

// ---- training backward: aggregator input gradient, softmax backward, VQ dgrad chain, d(mu | logvar) with the KL term ----
template <int MT>
__global__ void __launch_bounds__(DIB_MEASURE_THREADS) dib_measure_bwd_kernel(DibMeasureArgs a) {
#define DIB_MEASURE_BODY 2
#include "dib_measure_bodies.h"
#undef DIB_MEASURE_BODY
}

// ---- R replicas of the training forward / backward in one launch each (dib_measure_fwd_batched / _bwd_batched) ----
// grid (one replica's workgroups - the forward's as in the single launch, the backward's a share of the CUs -, replicas): a
// workgroup belongs to replica blockIdx.y, moves every pointer to
// that replica's slice and runs the single kernel's body on it - the same staging, the same tile walk over blockIdx.x, the same
// Philox rows (local to the replica) and, in the forward, the same workgroup-order KL sum behind the replica's own counter.
// No workgroup waits on another.  The seeds travel in the kernel arguments (a host array at the entry point): at most
// DIB_MEASURE_BATCH_SEEDS replicas per launch, the host splits a larger ensemble.
#define DIB_MEASURE_BATCH_SEEDS 64
struct DibMeasureBatchArgs {
  DibMeasureArgs a;                  // replica 0
  long long param_stride;            // floats between the replicas' packed VQ parameters
  long long w_agg0_stride;           // floats between the replicas' aggregator kernels
  long long counter_stride;          // unsigned words between the replicas' arrival counters
  uint64_t seeds[DIB_MEASURE_BATCH_SEEDS];
};

__device__ __forceinline__ DibMeasureArgs dib_measure_replica_args(const DibMeasureBatchArgs& ba, bool fwd) {
  DibMeasureArgs a = ba.a;
  const long long r = blockIdx.y, rows = a.rows, ps = r * ba.param_stride;
  a.w1 += ps; a.b1 += ps; a.w2 += ps; a.b2 += ps; a.w3 += ps; a.b3 += ps;
  a.enc += r * rows * 2 * a.E;
  a.seed = ba.seeds[r];
  if (fwd) {
    a.z += r * rows * a.E; a.h1s += r * rows * a.H1; a.h2s += r * rows * a.H2; a.soft += r * rows * a.A;
    a.out3 += r * 3;
    a.kl_part += r * (long long)gridDim.x;
    a.counter += r * ba.counter_stride;
  } else {
    a.h1c += r * rows * a.H1; a.h2c += r * rows * a.H2; a.softc += r * rows * a.A;
    a.g_agg += r * (rows / a.L) * a.agg_width;
    a.w_agg0 += r * ba.w_agg0_stride;
    a.out3c += r * 3;
    a.g3 += r * rows * a.A; a.g2 += r * rows * a.H2; a.g1 += r * rows * a.H1; a.g_enc += r * rows * 2 * a.E;
  }
  return a;
}

template <int MT>
__global__ void __launch_bounds__(DIB_MEASURE_THREADS) dib_measure_batched_fwd_kernel(DibMeasureBatchArgs ba) {
  const DibMeasureArgs a = dib_measure_replica_args(ba, true);
#define DIB_MEASURE_BODY 1
#include "dib_measure_bodies.h"
#undef DIB_MEASURE_BODY
}

template <int MT>
__global__ void __launch_bounds__(DIB_MEASURE_THREADS) dib_measure_batched_bwd_kernel(DibMeasureBatchArgs ba) {
  const DibMeasureArgs a = dib_measure_replica_args(ba, false);
#define DIB_MEASURE_BODY 2
#include "dib_measure_bodies.h"
#undef DIB_MEASURE_BODY
}

// ---- symbolisation: 16 points per wave, K draws each; one lane group per point keeps its argmax counts in registers ----
template <int MT>
__global__ void __launch_bounds__(DIB_MEASURE_THREADS) dib_measure_symbolize_kernel(DibMeasureArgs a) {
  extern __shared__ float lds[];
  const DibMeasureLds s = dib_measure_stage_fwd(lds, a);
  const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, wave = threadIdx.x >> 6;
  const int E = a.E, A = a.A;
  const long long ntiles = (a.rows + 15) / 16;
  for (long long t = (long long)blockIdx.x * DIB_MEASURE_WAVES + wave; t < ntiles; t += (long long)gridDim.x * DIB_MEASURE_WAVES) {
    const long long pt = t * 16 + m;
    const bool valid = pt < a.rows;
    float mu[8], sg[8];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 16 * it + 4 * g + j;
        const bool ok = valid && e < E;
        mu[4 * it + j] = ok ? a.enc[pt * 2 * E + e] : 0.f;
        sg[4 * it + j] = ok ? expf(0.5f * a.enc[pt * 2 * E + E + e]) : 0.f;
      }
    int cnt[4] = {0, 0, 0, 0};
    for (int k = 0; k < a.K; ++k) {
      const float* nz = a.noise + (long long)k * E;
      dib_f4 z[2];
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 16 * it + 4 * g + j;
          z[it][j] = e < E ? mu[4 * it + j] + nz[e] * sg[4 * it + j] : 0.f;
        }
      dib_f4 h1[MT], h2[MT], lg[1];
      dib_measure_chain<MT>(s, a, z, h1, h2, lg);
      // argmax over the row's A logits, the first maximum winning (NumPy)
      float bv = -INFINITY;
      int bi = 1 << 20;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * g + j < A && (lg[0][j] > bv || bi == (1 << 20))) { bv = lg[0][j]; bi = 4 * g + j; }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != (1 << 20) && (bi == (1 << 20) || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[j] += bi == 4 * g + j ? 1 : 0;
    }
    int wsum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) wsum += (4 * g + j) * cnt[j];
    wsum += __shfl_xor(wsum, 16, 64);
    wsum += __shfl_xor(wsum, 32, 64);
    if (valid) {
      if (g == 0) a.sym[pt] = (uint8_t)(2ll * wsum > (long long)a.K ? 1 : 0);
      if (a.counts) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * g + j < A) a.counts[pt * A + 4 * g + j] = cnt[j];
      }
    }
  }
}

// PositionalEncoding with frequencies 2^f0, 2^(f0+1), ... of gathered rows (the reference-state encoder: f0 = 0)
__global__ void __launch_bounds__(256)
dib_measure_posenc_rows_kernel(const float* __restrict__ X, long long ldx, const int* __restrict__ row_idx, int n, int d,
                               int n_blocks, float f0, float* __restrict__ P) {
  const long long total = (long long)n * d;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / d), c = (int)(i - (long long)r * d);
    const float x = X[(long long)row_idx[r] * ldx + c];
    float* dst = P + (long long)r * d * n_blocks + c;
    dst[0] = x;
    float fr = f0;
    for (int j = 1; j < n_blocks; ++j) { dst[(long long)j * d] = sinf(fr * x); fr *= 2.0f; }
  }
}
