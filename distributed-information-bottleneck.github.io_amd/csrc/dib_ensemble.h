// dib_ensemble.h - what a lockstep step of R DistributedIBNet replicas (include/dib_ensemble.h, ensemble.py) needs besides the
// grouped GEMMs: the batch gather + positional encoding of every (replica, feature), the reparameterisation + KL forward and
// backward, and the task loss with the History sums.  The replica is a grid index: a workgroup belongs to one replica, moves its
// pointers to that replica's slices and runs the single kernel's body text on them (dib_elementwise_bodies.h) - the same Philox
// key (seed_r, step, dataset row, feature, dim), the same arithmetic, sums in a fixed order.  No workgroup waits on another:
// where a second stage is needed the LAST workgroup of a (replica, feature) / replica to arrive runs it (an integer arrival
// counter, self-cleaning; the pattern of dib_circuit_mi_kernel), so the sums have the same bits every call.
#pragma once
#include "dib_common.h"

#define DIB_ENS_POSENC_ROWS 16   // batch rows per workgroup tile of the gather (the small-batch tiling of dib_posenc_kernel)

// x [N][ldx] sample-major, F features of d columns each; rows [R][batch] dataset rows.  P [R F][batch][n_blocks d]:
// P[r F + f][b][j d + c] = (j == 0 ? v : sin(2^j v)), v = x[rows[r][b]][f d + c] - dib_posenc_kernel's arithmetic.  One workgroup
// = 16 rows x 64 input columns of one replica: the tile is read along the x rows (coalesced), transposed through LDS and written
// with lanes <-> consecutive rows of one column.  grid (ceil(F d / 64), ceil(batch / 16), R).
__global__ void __launch_bounds__(256)
dib_ens_posenc_rows_kernel(const float* __restrict__ X, long long ldx, const int* __restrict__ rows, int batch, int F, int d,
                           int n_blocks, float* __restrict__ P) {
  __shared__ float T[DIB_ENS_POSENC_ROWS][65];
  const long long rep = blockIdx.z;
  const int* __restrict__ const row_idx = rows + rep * batch;
  const int ncols = F * d, c0 = blockIdx.x * 64, b0 = blockIdx.y * DIB_ENS_POSENC_ROWS;
#pragma unroll
  for (int i = 0; i < DIB_ENS_POSENC_ROWS / 4; ++i) {
    const int idx = threadIdx.x + 256 * i, r = idx >> 6, c = idx & 63;
    float v = 0.f;
    if (b0 + r < batch && c0 + c < ncols) v = X[(long long)row_idx[b0 + r] * ldx + c0 + c];
    T[r][c] = v;
  }
  __syncthreads();
  const int r = threadIdx.x & (DIB_ENS_POSENC_ROWS - 1), b = b0 + r;
  if (b >= batch) return;
  const long long pw = (long long)n_blocks * d;
  for (int c = threadIdx.x / DIB_ENS_POSENC_ROWS; c < 64 && c0 + c < ncols; c += 256 / DIB_ENS_POSENC_ROWS) {
    const int f = (c0 + c) / d, cl = (c0 + c) - f * d;
    const float x = T[r][c];
    float* dst = P + ((rep * F + f) * batch + b) * pw + cl;
    dst[0] = x;
    float fr = 2.0f;
    for (int j = 1; j < n_blocks; ++j) {
      dst[(long long)j * d] = sinf(fr * x);
      fr *= 2.0f;
    }
  }
}

// enc [R][F][batch][2E] (the encoder plan's last activation), rows [R][batch], seeds [R] -> u [R][batch][F E] (the integration
// plan's input) and kl [R][F] = sum over the batch rows of KL_f.  grid (row tiles of dib_reparam_kl_fwd_kernel, F, R).
// parts [R][gridDim.x][F] workgroup partials, counters [R F] zero before the first launch.
__global__ void __launch_bounds__(256)
dib_ens_reparam_kl_fwd_kernel(const float* __restrict__ enc, float* __restrict__ u_all, float* __restrict__ parts,
                              unsigned* __restrict__ counters, float* __restrict__ kl, const int* __restrict__ rows, int batch, int F,
                              int E, const unsigned long long* __restrict__ seeds, unsigned step_arg, int deterministic) {
  const long long rep = blockIdx.z;
  const float* __restrict__ const enc_out = enc + rep * F * batch * 2ll * E;
  float* __restrict__ const U = u_all + rep * batch * (long long)F * E;
  float* __restrict__ const kl_partial = parts + rep * gridDim.x * F;
  const int* __restrict__ const row_idx = rows + rep * batch;
  const long long row0 = 0;
  const unsigned long long seed = seeds[rep];
  unsigned step = step_arg;
  const unsigned* const step_dev = nullptr;
  const float lv_off = 0.f;
#define DIB_ELEMENTWISE_BODY 1
#include "dib_elementwise_bodies.h"
#undef DIB_ELEMENTWISE_BODY
  // second stage by the last workgroup of (replica, feature) to arrive: the partials in workgroup order
  if (threadIdx.x == 0) {   // (the thread that wrote this workgroup's partial `tot`)
    __threadfence();
    if (atomicAdd(counters + rep * F + f, 1u) == gridDim.x - 1u) {
      __threadfence();
      float s = 0.f;
      for (unsigned k = 0; k < gridDim.x; ++k)
        s += __hip_atomic_load(kl_partial + (long long)k * F + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      kl[rep * F + f] = s;
      counters[rep * F + f] = 0u;
    }
  }
}

// enc, g_u [R][batch][F E], u, beta [R] -> d_enc [R][F][batch][2E] (the encoder plan's last gradient region).  The noise term is
// u - mu.  grid as the forward.
__global__ void __launch_bounds__(256)
dib_ens_reparam_kl_bwd_kernel(const float* __restrict__ enc, const float* __restrict__ g_u, const float* __restrict__ u_all,
                              float* __restrict__ d_enc, const float* __restrict__ beta, float inv_bg, int batch, int F, int E) {
  const long long rep = blockIdx.z;
  const float* __restrict__ const enc_out = enc + rep * F * batch * 2ll * E;
  const float* __restrict__ const GU = g_u + rep * batch * (long long)F * E;
  const float* __restrict__ const U = u_all + rep * batch * (long long)F * E;
  float* __restrict__ const dout = d_enc + rep * F * batch * 2ll * E;
  const float* __restrict__ const beta_dev = beta + rep;
  const float lv_off = 0.f;
#define DIB_ELEMENTWISE_BODY 2
#include "dib_elementwise_bodies.h"
#undef DIB_ELEMENTWISE_BODY
}

// pred [R][batch][out_dim], labels Y[rows[r][b]], beta [R], kl [R][F] (the forward's sums) -> g_pred [R][batch][out_dim] and the
// History sums of the step added to acc [R][F + 3] in dib_metrics_accumulate_kernel's layout per replica:
//   acc[f] += kl[f] inv_bg ;  acc[F] += task sum + beta_r sum_f kl[f] ;  acc[F + 1] += #correct ;  acc[F + 2] += batch
// grid (ceil(batch / 256), R): one thread per row; the last workgroup of a replica to arrive sums the workgroup partials in order.
// parts [R][gridDim.x][2], counters [R] zero before the first launch.
__global__ void __launch_bounds__(256)
dib_ens_loss_kernel(int kind, const float* __restrict__ pred_all, int out_dim, const float* __restrict__ Y, long long ldy,
                    const int* __restrict__ rows, int batch, float inv_bg, int out_act, float* __restrict__ g_all,
                    float* __restrict__ parts, unsigned* __restrict__ counters, const float* __restrict__ kl, int F,
                    const float* __restrict__ beta, float* __restrict__ acc_all) {
  const long long rep = blockIdx.y;
  const float* __restrict__ const pred = pred_all + rep * batch * out_dim;
  float* __restrict__ const g_pred = g_all + rep * batch * out_dim;
  const int* __restrict__ const row_idx = rows + rep * batch;
  const long long row0 = 0;
  float* __restrict__ const partial = parts + rep * gridDim.x * 2;
#define DIB_ELEMENTWISE_BODY 3
#include "dib_elementwise_bodies.h"
#undef DIB_ELEMENTWISE_BODY
  __shared__ int last;
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(counters + rep, 1u) == gridDim.x - 1u;
  }
  __syncthreads();
  if (!last) return;
  float* __restrict__ const acc = acc_all + rep * (F + 3);
  const float* __restrict__ const klr = kl + rep * F;
  for (int i = threadIdx.x; i < F; i += 256) acc[i] += klr[i] * inv_bg;
  if (threadIdx.x == 0) {
    __threadfence();
    float task = 0.f, right = 0.f, s = 0.f;
    for (unsigned k = 0; k < gridDim.x; ++k) {
      task += __hip_atomic_load(partial + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      right += __hip_atomic_load(partial + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int i = 0; i < F; ++i) s += klr[i];
    acc[F] += task + beta[rep] * s;
    acc[F + 1] += right;
    acc[F + 2] += (float)batch;
    counters[rep] = 0u;
  }
}
