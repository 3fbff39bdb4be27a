// dib_grad_transform.h - what Keras optimizer_v2 does to the gradient and the learning rate before the update rule: clipvalue,
// clipnorm, global_clipnorm over the variables of a flat buffer, and the learning rate of a step as a function of the device
// step count.  include/dib_grad_transform.h states the semantics and the variable table.
//
// HBM-streaming kernels over a tile work-list (DibGradTile = dib_grad_tile: start, count, segment), one 256-thread workgroup per
// tile of at most 4096 elements: a tile never crosses a segment and the alignment gaps of the buffer are in no tile, so a gap is
// neither read nor written.  A tile starts wherever its segment does (biases of feature f start at o + f * width): a scalar head
// of (4 - start % 4) % 4 elements brings the body to a 16-byte boundary, the body is float4 loads (thread t takes float4 t,
// t + 256, ...), a scalar tail takes the rest.  Which element a lane sees depends on the tile alone.
//
// Determinism.  dib_grad_sumsq_tile_kernel: each lane adds its squares in float64 in element order, the 64 lanes of a wave are
// combined by a fixed xor butterfly, the four waves in wave order - no atomics; dib_grad_sumsq_finish_kernel adds a segment's
// tile partials in tile order.  A square of a float32 is exact in float64 and contraction is off, so body and head / tail lanes
// round alike.  The apply kernel's float32 expressions are contraction-off too (the operation order of the header is the bits).
#pragma once
#include "dib_common.h"

struct DibGradTile { long long start; int count; int segment; };

constexpr int kGradTile = 4096;   // DIB_GRAD_TILE

__device__ __forceinline__ float dib_grad_scaled(float g, float gscale, float clipvalue) {
#pragma clang fp contract(off)
  float v = g * gscale;
  if (clipvalue > 0.f) v = fminf(fmaxf(v, -clipvalue), clipvalue);
  return v;
}

__device__ __forceinline__ double dib_grad_sq(float g, float gscale, float clipvalue) {
#pragma clang fp contract(off)
  const double d = (double)dib_grad_scaled(g, gscale, clipvalue);
  return d * d;
}

// partials[tile] = sum over the tile of (clip(g * gscale))^2, for the tiles [tile_first, tile_first + gridDim.x)
__global__ void __launch_bounds__(256)
dib_grad_sumsq_tile_kernel(const DibGradTile* __restrict__ tiles, int tile_first, const float* __restrict__ grads, float gscale,
                           float clipvalue, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double wave_sum[4];
  const int tile = tile_first + blockIdx.x;
  const DibGradTile t = tiles[tile];
  const float* g = grads + t.start;
  const int tid = threadIdx.x;
  const int head = min(t.count, (int)((4 - (t.start & 3)) & 3));
  const int body4 = (t.count - head) >> 2;
  const int tail = (t.count - head) & 3;
  double acc = 0.0;
  if (tid < head) acc = acc + dib_grad_sq(g[tid], gscale, clipvalue);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  for (int i = tid; i < body4; i += 256) {
    const float4 v = g4[i];
    acc = acc + dib_grad_sq(v.x, gscale, clipvalue);
    acc = acc + dib_grad_sq(v.y, gscale, clipvalue);
    acc = acc + dib_grad_sq(v.z, gscale, clipvalue);
    acc = acc + dib_grad_sq(v.w, gscale, clipvalue);
  }
  if (tid < tail) acc = acc + dib_grad_sq(g[head + (body4 << 2) + tid], gscale, clipvalue);
  for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[tile] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// ss[s] = sum of the partials of segment s's tiles, in tile order, for the segments [seg_first, seg_first + seg_count)
__global__ void __launch_bounds__(256)
dib_grad_sumsq_finish_kernel(const int* __restrict__ seg_tile0, int seg_first, int seg_count, const double* __restrict__ partials,
                             double* __restrict__ ss) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= seg_count) return;
  const int s = seg_first + k;
  double acc = 0.0;
  for (int i = seg_tile0[s]; i < seg_tile0[s + 1]; ++i) acc = acc + partials[i];
  ss[s] = acc;
}

struct DibGradClip { float gscale, clipvalue, norm; int mode; };   // mode: DIB_CLIP_*

// one element: the value clip, then the norm clip with the workgroup's coefficient (den = max(n, c) | scale)
__device__ __forceinline__ float dib_grad_clip_one(float g, const DibGradClip& c, float coef) {
#pragma clang fp contract(off)
  const float v = dib_grad_scaled(g, c.gscale, c.clipvalue);
  if (c.mode == 1) return (v * c.norm) / coef;
  if (c.mode == 2) return v * coef;
  return v;
}

// grads <- transformed g, for the tiles [tile_first, tile_first + gridDim.x)
__global__ void __launch_bounds__(256)
dib_grad_clip_apply_kernel(const DibGradTile* __restrict__ tiles, int tile_first, float* __restrict__ grads, DibGradClip c,
                           const double* __restrict__ ss, const double* __restrict__ ss_all, int n_ss) {
#pragma clang fp contract(off)
  __shared__ float coef_s;
  const DibGradTile t = tiles[tile_first + blockIdx.x];
  const int tid = threadIdx.x;
  if (tid == 0) {
    float coef = 1.f;
    if (c.mode == 1) {   // per variable: n = sqrt(ss), 0 for a zero gradient; den = max(n, c)
      const double s = ss[t.segment];
      const float n = s > 0.0 ? (float)sqrt(s) : 0.f;
      coef = fmaxf(n, c.norm);
    } else if (c.mode == 2) {   // over every ss given, in index order; (N - N): a non-finite norm poisons every gradient
      double s = 0.0;
      for (int i = 0; i < n_ss; ++i) s = s + ss_all[i];
      const float N = (float)sqrt(s);
      coef = c.norm * fminf(1.0f / N, 1.0f / c.norm) + (N - N);
    }
    coef_s = coef;
  }
  __syncthreads();
  const float coef = coef_s;
  float* g = grads + t.start;
  const int head = min(t.count, (int)((4 - (t.start & 3)) & 3));
  const int body4 = (t.count - head) >> 2;
  const int tail = (t.count - head) & 3;
  if (tid < head) g[tid] = dib_grad_clip_one(g[tid], c, coef);
  float4* g4 = reinterpret_cast<float4*>(g + head);
  for (int i = tid; i < body4; i += 256) {
    float4 v = g4[i];
    v.x = dib_grad_clip_one(v.x, c, coef);
    v.y = dib_grad_clip_one(v.y, c, coef);
    v.z = dib_grad_clip_one(v.z, c, coef);
    v.w = dib_grad_clip_one(v.w, c, coef);
    g4[i] = v;
  }
  if (tid < tail) {
    const int i = head + (body4 << 2) + tid;
    g[i] = dib_grad_clip_one(g[i], c, coef);
  }
}

// ---- the learning rate of a step: lr_dev[0] = schedule(t_dev[0]) in float32, one thread -------------------------------------
struct DibLrSchedule {   // = dib_lr_schedule
  int kind, flags;
  float initial, decay_steps, rate, end, power, alpha;
  int n_boundaries, reserved;
  long long boundaries[8];
  float values[9];
  float reserved2;
};

__global__ void dib_lr_schedule_kernel(DibLrSchedule s, const long long* __restrict__ t_dev, float* __restrict__ lr_dev) {
#pragma clang fp contract(off)
  const long long t = t_dev[0];
  float step = (float)t;
  float lr = s.initial;
  switch (s.kind) {
    case 1: lr = s.initial / (1.0f + s.rate * step); break;
    case 2: case 3: {
      float p = step / s.decay_steps;
      if (s.flags & 1) p = floorf(p);
      lr = s.kind == 2 ? s.initial * powf(s.rate, p) : s.initial / (1.0f + s.rate * p);
      break;
    }
    case 4: {
      float ds = s.decay_steps;
      if (s.flags & 2) ds = ds * fmaxf(1.0f, ceilf(step / ds));
      else step = fminf(step, ds);
      lr = (s.initial - s.end) * powf(1.0f - step / ds, s.power) + s.end;
      break;
    }
    case 5: {
      lr = s.values[s.n_boundaries];
      for (int i = s.n_boundaries - 1; i >= 0; --i)
        if (t <= s.boundaries[i]) lr = s.values[i];
      break;
    }
    case 6: {
      step = fminf(step, s.decay_steps);
      lr = s.initial * (((1.0f - s.alpha) * 0.5f) * (1.0f + cosf((3.14159265358979323846f * step) / s.decay_steps)) + s.alpha);
      break;
    }
  }
  lr_dev[0] = lr;
}
