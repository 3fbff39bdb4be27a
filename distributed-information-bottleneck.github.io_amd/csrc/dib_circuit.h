// dib_circuit.h - the Boolean-circuit notebook's scalar-channel distributed IB (include/dib_circuit.h;
// complex_systems/InfoDecomp_Boolean_circuits.ipynb cells 4 and 6): everything of a training step in front of the predictor
// (row draw, gather, reparameterisation, KL), the gradient of the 2G encoder scalars behind it, and the sandwich bounds of
// every gate's channel for all evaluation batches in one launch.  The predictor itself runs on the row-tile head kernel
// (dib_mlp_small_head_step) and the grouped weight-gradient GEMM.
//
// Gate g's encoder (SimpleEncoder) holds two scalars, s_g and lv_g (params + sc_off: s[0..G) then lv[0..G)):
//   x in {-1, +1} -> N(x s_g, exp(lv_g)),  u = x s_g + exp(lv_g / 2) eps,  KL_g = 0.5 (s_g^2 + exp(lv_g) - lv_g - 1)
// (mu^2 = s^2 for x = +-1, so the notebook's batch mean of the per-row KL is this value).
//
// Row draw: r_b = x0 >> (32 - G), x0 the first output of Philox4x32-10 at counter (b, 0xFFFFFFFF, 0, step), key = seed.  The
// table has 2^G rows, so the top G bits of a uniform 32-bit word are an exactly uniform row (tf.random.categorical over zero
// logits: uniform, with replacement).  The counter's second word never equals a gate index, so the draw is independent of the
// eps draws, which keep the library's key (seed, step, row b, feature g, dim 0).
#pragma once
#include "dib_common.h"
#include "dib_gauss_lse.h"

#define DIB_CIRCUIT_MAX_GATES 16
#define DIB_CIRCUIT_MAX_BATCH 2048
#define DIB_CIRCUIT_LD 16          // u's row pitch: 16 * ceil(G / 16) with G <= 16

__device__ __forceinline__ uint32_t dib_circuit_draw_row(uint64_t seed, uint32_t step, uint32_t b, int G) {
  const dib_u4 c = {b, 0xFFFFFFFFu, 0u, step};
  const dib_u4 r = dib_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return r.x >> (32 - G);
}

__device__ __forceinline__ float dib_circuit_eps(uint64_t seed, uint32_t step, uint32_t b, uint32_t g) {
  float e[4];
  dib_eps4(seed, step, b, g, 0u, e);
  return e[0];
}

// one thread per (row b, column k < 16): u [B][16] (pad columns 0), y [B], drawn rows [B]; workgroup 0 also writes
// kl[0..G) and kl[G] = beta * sum_g kl[g] (summed in gate order)
__global__ void __launch_bounds__(256)
dib_circuit_fwd_kernel(const uint32_t* __restrict__ table, int G, int B, const float* __restrict__ sc, uint64_t seed, uint32_t step,
                       float beta, const int32_t* __restrict__ row_in, int32_t* __restrict__ row_out, float* __restrict__ u,
                       float* __restrict__ y, float* __restrict__ kl) {
#define DIB_CIRCUIT_BODY 1
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}

// one workgroup per gate: ds_g = sum_b g_u[b][g] x[b][g] + beta s_g, dlv_g = sum_b g_u[b][g] eps[b][g] exp(lv_g / 2) / 2 +
// beta (exp(lv_g) - 1) / 2 - float64 partials, strided over the batch, then a fixed tree: the same bits on any device
__global__ void __launch_bounds__(256)
dib_circuit_bwd_kernel(const uint32_t* __restrict__ table, int G, int B, const float* __restrict__ sc, uint64_t seed, uint32_t step,
                       float beta, const int32_t* __restrict__ rows, const float* __restrict__ g_u, float* __restrict__ g_sc) {
  const int g = blockIdx.x;
#define DIB_CIRCUIT_BODY 2
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}

// Sandwich bounds of every gate's channel for nb evaluation batches of n points (x [nb][n] = +-1), eps of point i of batch b
// keyed (seed, b, i, g).  Per point the arithmetic of dib_mi_prep_kernel + dib_mi_rows_kernel on the encoder output
// (x s_g, lv_g): u_i = mu_i + sigma eps_i, l_ij = c - ((u_i - mu_j) / sigma)^2 / 2 (every point of a gate shares sigma and c),
// lower_i = l_ii - (LSE_j l_ij - log n), upper_i = l_ii - (LSE_{j != i} l_ij - log n), in float64 with a log-sum-exp.
// A workgroup takes 64 points of one (gate, batch), four lanes per point (every fourth j, merged by two shuffles); it sums its
// 64 rows in order into a partial, and the last of the (gate, batch)'s ceil(n / 64) workgroups to arrive sums the partials in
// order: out[g][b] = {lower, upper} (nats), the same bits every call.
#define DIB_CIRCUIT_MI_ROWS 64

__global__ void __launch_bounds__(256)
dib_circuit_mi_kernel(const float* __restrict__ sc, int G, const float* __restrict__ xs, int n, int nb, uint64_t seed,
                      double* __restrict__ part_ws, unsigned* __restrict__ counters, double* __restrict__ out) {
  const int g = blockIdx.z;
#define DIB_CIRCUIT_BODY 3
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}

// ---- R replicas per launch (dib_circuit_fwd_batched / _bwd_batched / _mi_bounds_batched) ----
// The model's architecture does not depend on the circuit (u is 16 columns wide for every G), so replicas may differ in
// circuit, truth table, G, seed and beta and still share a launch.  A workgroup belongs to one replica (a grid index), moves its
// pointers to that replica's slices and runs the single kernel's body text on them (dib_circuit_bodies.h): the same Philox rows
// (local to the replica), the same fixed-order sums, the replica's own arrival counters.  No workgroup waits on a workgroup of
// another replica.  The per-replica scalars travel in the kernel arguments (host arrays at the entry points; uniform index: scalar
// loads): at most DIB_CIRCUIT_BATCH replicas per launch, the host splits a larger ensemble.
#define DIB_CIRCUIT_BATCH 64
struct DibCircuitBatchArgs {
  const uint32_t* tables;            // the replicas' truth tables, concatenated
  const float* params;               // replica 0's flat parameters; sc = params + r * param_stride + sc_off
  long long param_stride, sc_off;
  int B; uint32_t step;
  const int32_t* row_in; int32_t* rows; float* u; float* y; float* kl;   // forward: [R][B], [R][B], [R][B][16], [R][B], [R][17]
  const float* g_u; float* grads; long long grad_stride;                 // backward: [R][B][16]; g_sc = grads + r * grad_stride + sc_off
  uint64_t seeds[DIB_CIRCUIT_BATCH];
  float beta[DIB_CIRCUIT_BATCH];
  int table_off[DIB_CIRCUIT_BATCH];  // words
  int G[DIB_CIRCUIT_BATCH];
};

// grid (the single forward's workgroups, replicas)
__global__ void __launch_bounds__(256) dib_circuit_batched_fwd_kernel(DibCircuitBatchArgs ba) {
  const long long rep = blockIdx.y;
  const int G = ba.G[rep], B = ba.B;
  const uint32_t* __restrict__ const table = ba.tables + ba.table_off[rep];
  const float* __restrict__ const sc = ba.params + rep * ba.param_stride + ba.sc_off;
  const uint64_t seed = ba.seeds[rep];
  const uint32_t step = ba.step;
  const float beta = ba.beta[rep];
  const int32_t* __restrict__ const row_in = ba.row_in ? ba.row_in + rep * B : nullptr;
  int32_t* __restrict__ const row_out = ba.rows + rep * B;
  float* __restrict__ const u = ba.u + rep * B * DIB_CIRCUIT_LD;
  float* __restrict__ const y = ba.y + rep * B;
  float* __restrict__ const kl = ba.kl + rep * (DIB_CIRCUIT_MAX_GATES + 1);
#define DIB_CIRCUIT_BODY 1
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}

// grid (gates, replicas): the workgroups of gates a replica does not have exit
__global__ void __launch_bounds__(256) dib_circuit_batched_bwd_kernel(DibCircuitBatchArgs ba) {
  const long long rep = blockIdx.y;
  const int g = blockIdx.x;
  const int G = ba.G[rep], B = ba.B;
  if (g >= G) return;
  const uint32_t* __restrict__ const table = ba.tables + ba.table_off[rep];
  const float* __restrict__ const sc = ba.params + rep * ba.param_stride + ba.sc_off;
  const uint64_t seed = ba.seeds[rep];
  const uint32_t step = ba.step;
  const float beta = ba.beta[rep];
  const int32_t* __restrict__ const rows = ba.rows + rep * B;
  const float* __restrict__ const g_u = ba.g_u + rep * B * DIB_CIRCUIT_LD;
  float* __restrict__ const g_sc = ba.grads + rep * ba.grad_stride + ba.sc_off;
#define DIB_CIRCUIT_BODY 2
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}

// grid (chunks of 64 points, batches, 16 x replicas): z = 16 r + g runs over the (replica, gate) pairs, those with g >= G_r exit.
// Every replica has a workspace slice of the single kernel's layout at G = 16 (partials, then arrival counters) and writes
// out [R][16][nb][2]; rows g >= G_r are not touched.
struct DibCircuitMiBatchArgs {
  const float* params; long long param_stride, sc_off;
  const float* xs; int n, nb;        // [R][nb][n]
  char* ws; long long ws_stride;     // bytes between the replicas' slices
  double* out;
  uint64_t seeds[DIB_CIRCUIT_BATCH];
  int G[DIB_CIRCUIT_BATCH];
};

__global__ void __launch_bounds__(256) dib_circuit_batched_mi_kernel(DibCircuitMiBatchArgs ba) {
  const long long rep = blockIdx.z >> 4;
  const int g = blockIdx.z & 15;
  const int G = ba.G[rep], n = ba.n, nb = ba.nb;
  if (g >= G) return;
  const float* __restrict__ const sc = ba.params + rep * ba.param_stride + ba.sc_off;
  const float* __restrict__ const xs = ba.xs + rep * nb * n;
  const uint64_t seed = ba.seeds[rep];
  double* __restrict__ const part_ws = (double*)(ba.ws + rep * ba.ws_stride);
  unsigned* __restrict__ const counters = (unsigned*)(part_ws + (long long)DIB_CIRCUIT_MAX_GATES * nb * gridDim.x * 2);
  double* __restrict__ const out = ba.out + rep * DIB_CIRCUIT_MAX_GATES * nb * 2;
#define DIB_CIRCUIT_BODY 3
#include "dib_circuit_bodies.h"
#undef DIB_CIRCUIT_BODY
}
