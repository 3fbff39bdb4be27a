// dib_losses.h - the Keras loss and metric family of compile(loss=, metrics=) beyond dib_loss_kernel's four kinds
// (include/dib_losses.h has the formulas).  One kernel template, dib_loss_ex_kernel<KIND, LANES>:
//   * a workgroup of 256 threads owns the 256 rows of a block of dib_loss_kernel and writes the same partial pair
//     {sum loss, sum metric}, so m.loss_blocks, dib_loss_finalize_kernel and dib_step_tail(DIB_TAIL_LOSS) read it unchanged;
//   * LANES in {1, 4, 16, 64} consecutive lanes share a row (the host picks LANES from out_dim) and walk its class axis with a
//     stride of LANES: a wave's loads of pred / y and its stores of g_pred are runs of LANES consecutive floats per row, one
//     contiguous run per wave at LANES = 64 - dib_loss_kernel's lanes are out_dim floats apart;
//   * the 256 / LANES rows of a pass are handled together, LANES passes cover the block;
//   * a lane's sums run over k = lane, lane + LANES, ... in that order, the lanes of a row combine by an xor butterfly, the
//     rows of a block by the lane-0 accumulators in pass order and dib_block_sum_256: no atomics, the bits of a row depend on
//     (out_dim, LANES) alone and those of a block on its rows alone, never on the grid or the address.
// The class-axis kinds read a row two or three times (statistics, then the gradient); the re-reads hit the cache the first
// pass filled (a row is at most a few KB).
#pragma once
#include "dib_common.h"
#include "../../include/dib_losses.h"

#define DIB_LOSS_EPS 1e-7f

template <int LANES> __device__ __forceinline__ float dib_grp_sum(float v) {
#pragma unroll
  for (int o = LANES >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int LANES> __device__ __forceinline__ float dib_grp_max(float v) {
#pragma unroll
  for (int o = LANES >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// arg-max over the lanes of a row, the first of equal maxima (numpy.argmax)
template <int LANES> __device__ __forceinline__ int dib_grp_argmax(float v, int i) {
#pragma unroll
  for (int o = LANES >> 1; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  return i;
}

__device__ __forceinline__ float dib_sign(float e) { return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float dib_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

constexpr bool dib_loss_is_elementwise(int kind) {
  return kind == DIB_LOSS_BCE_LOGITS || kind == DIB_LOSS_BCE || kind == DIB_LOSS_MSE || (kind >= DIB_LOSS_MAE && kind <= DIB_LOSS_KLD);
}

// value l and derivative g of one element of an element-wise kind (prm: delta / label smoothing)
template <int KIND> __device__ __forceinline__ void dib_loss_elem(float p, float y, float prm, float& l, float& g) {
  const float e = p - y;
  if constexpr (KIND == DIB_LOSS_BCE_LOGITS) {
    const float ys = y * (1.f - prm) + 0.5f * prm;
    l = fmaxf(p, 0.f) - p * ys + log1pf(expf(-fabsf(p)));
    g = 1.0f / (1.0f + expf(-p)) - ys;
  } else if constexpr (KIND == DIB_LOSS_BCE) {
    const float ys = y * (1.f - prm) + 0.5f * prm;
    const float pc = fminf(fmaxf(p, DIB_LOSS_EPS), 1.0f - DIB_LOSS_EPS);
    l = -(ys * logf(pc) + (1.f - ys) * logf(1.f - pc));
    g = (p < DIB_LOSS_EPS || p > 1.0f - DIB_LOSS_EPS) ? 0.f : (-(ys / pc) + (1.f - ys) / (1.f - pc));
  } else if constexpr (KIND == DIB_LOSS_MSE) {
    l = e * e;
    g = 2.f * e;
  } else if constexpr (KIND == DIB_LOSS_MAE) {
    l = fabsf(e);
    g = dib_sign(e);
  } else if constexpr (KIND == DIB_LOSS_MAPE) {
    const float r = 100.f / fmaxf(fabsf(y), DIB_LOSS_EPS);
    l = fabsf(e) * r;
    g = dib_sign(e) * r;
  } else if constexpr (KIND == DIB_LOSS_MSLE) {
    const float a = log1pf(fmaxf(p, DIB_LOSS_EPS)) - log1pf(fmaxf(y, DIB_LOSS_EPS));
    l = a * a;
    g = p < DIB_LOSS_EPS ? 0.f : 2.f * a / (p + 1.f);
  } else if constexpr (KIND == DIB_LOSS_HUBER) {
    const float ae = fabsf(e);
    l = ae <= prm ? 0.5f * e * e : prm * ae - 0.5f * prm * prm;
    g = ae <= prm ? e : prm * dib_sign(e);
  } else if constexpr (KIND == DIB_LOSS_LOGCOSH) {
    l = e + dib_softplus(-2.f * e) - 0.6931471805599453f;
    g = tanhf(e);
  } else if constexpr (KIND == DIB_LOSS_POISSON) {
    l = p - y * logf(p + DIB_LOSS_EPS);
    g = 1.f - y / (p + DIB_LOSS_EPS);
  } else {  // DIB_LOSS_KLD
    const float yc = fminf(fmaxf(y, DIB_LOSS_EPS), 1.f), pc = fminf(fmaxf(p, DIB_LOSS_EPS), 1.f);
    l = yc * logf(yc / pc);
    g = (p < DIB_LOSS_EPS || p > 1.f) ? 0.f : -yc / pc;
  }
}

template <int KIND, int LANES>
__global__ void __launch_bounds__(256)
dib_loss_ex_kernel(int metric, float prm, const float* __restrict__ pred, int C, const float* __restrict__ Y, long long ldy,
                   const int* __restrict__ row_idx, long long row0, int batch, float inv_bg, int out_act,
                   float* __restrict__ g_pred, float* __restrict__ partial /*[gridDim.x][2]*/) {
  __shared__ float red[4];
  constexpr int RPP = 256 / LANES;   // rows of a pass
  const int lane = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const float invC = 1.f / (float)C;
  float lsum = 0.f, msum = 0.f;
  for (int pass = 0; pass < LANES; ++pass) {
    if (blockIdx.x * 256 + pass * RPP >= batch) break;   // (uniform over the workgroup)
    const int b = blockIdx.x * 256 + pass * RPP + grp;
    const bool valid = b < batch;
    const int n = valid ? C : 0;                         // a lane without a row loops zero times and still joins the butterflies
    const int bb = valid ? b : 0;
    const long long row = row_idx ? (long long)row_idx[bb] : row0 + bb;
    const float* p = pred + (long long)bb * C;
    float* g = g_pred + (long long)bb * C;
    const float* y = Y + row * ldy;
    const int lab = KIND == DIB_LOSS_SPARSE_CCE || metric == DIB_METRIC_SPARSE_CATEGORICAL_ACCURACY
                        ? min(max((int)y[0], 0), C - 1) : 0;
    // ---- the metric: the labels as given ----
    float mrow = 0.f;
    if (metric == DIB_METRIC_BINARY_ACCURACY || metric == DIB_METRIC_MAE || metric == DIB_METRIC_MSE) {
      float s = 0.f;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k], yk = y[k], e = pk - yk;
        s += metric == DIB_METRIC_MAE ? fabsf(e) : metric == DIB_METRIC_MSE ? e * e : (((pk > 0.5f ? 1.f : 0.f) == yk) ? 1.f : 0.f);
      }
      mrow = dib_grp_sum<LANES>(s) * invC;
    } else if (metric == DIB_METRIC_CATEGORICAL_ACCURACY || metric == DIB_METRIC_SPARSE_CATEGORICAL_ACCURACY) {
      float pm = -INFINITY, ym = -INFINITY;
      int pi = 0x7fffffff, yi = 0x7fffffff;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k];
        if (pk > pm) { pm = pk; pi = k; }
        if (metric == DIB_METRIC_CATEGORICAL_ACCURACY) {
          const float yk = y[k];
          if (yk > ym) { ym = yk; yi = k; }
        }
      }
      pi = dib_grp_argmax<LANES>(pm, pi);
      if (metric == DIB_METRIC_CATEGORICAL_ACCURACY) yi = dib_grp_argmax<LANES>(ym, yi); else yi = lab;
      mrow = pi == yi ? 1.f : 0.f;
    }
    // ---- the loss and its gradient ----
    float lrow;
    if constexpr (dib_loss_is_elementwise(KIND)) {
      const float sc = KIND == DIB_LOSS_KLD ? 1.f : invC;
      float s = 0.f;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k];
        float l, gg;
        dib_loss_elem<KIND>(pk, y[k], prm, l, gg);
        s += l;
        g[k] = gg * sc * inv_bg * dib_act_grad(out_act, pk);
      }
      lrow = dib_grp_sum<LANES>(s) * sc;
    } else if constexpr (KIND == DIB_LOSS_COSINE) {
      float syy = 0.f, spp = 0.f, syp = 0.f;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k], yk = y[k];
        syy += yk * yk; spp += pk * pk; syp += yk * pk;
      }
      syy = dib_grp_sum<LANES>(syy); spp = dib_grp_sum<LANES>(spp); syp = dib_grp_sum<LANES>(syp);
      const float ry = rsqrtf(fmaxf(syy, 1e-12f)), rp = rsqrtf(fmaxf(spp, 1e-12f));
      lrow = -(syp * ry * rp);
      const float c3 = spp >= 1e-12f ? syp * rp * rp * rp : 0.f;   // the clamp's own derivative is zero
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k];
        g[k] = -ry * (y[k] * rp - c3 * pk) * inv_bg * dib_act_grad(out_act, pk);
      }
    } else if constexpr (KIND == DIB_LOSS_CCE_LOGITS) {
      const float ya = 1.f - prm, yb = prm * invC;
      float m = -INFINITY, sy = 0.f, syz = 0.f;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k], ys = y[k] * ya + yb;
        m = fmaxf(m, pk); sy += ys; syz += ys * pk;
      }
      m = dib_grp_max<LANES>(m); sy = dib_grp_sum<LANES>(sy); syz = dib_grp_sum<LANES>(syz);
      float se = 0.f;
      for (int k = lane; k < n; k += LANES) se += expf(p[k] - m);
      se = dib_grp_sum<LANES>(se);
      const float lse = m + logf(se);
      lrow = lse * sy - syz;
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k];
        g[k] = (expf(pk - lse) * sy - (y[k] * ya + yb)) * inv_bg * dib_act_grad(out_act, pk);
      }
    } else if constexpr (KIND == DIB_LOSS_CCE) {
      const float ya = 1.f - prm, yb = prm * invC;
      float S = 0.f;
      for (int k = lane; k < n; k += LANES) S += p[k];
      S = dib_grp_sum<LANES>(S);
      const float rS = 1.f / S;
      float v = 0.f, aq = 0.f;
      for (int k = lane; k < n; k += LANES) {
        const float q = p[k] * rS, ys = y[k] * ya + yb;
        const float c = fminf(fmaxf(q, DIB_LOSS_EPS), 1.f - DIB_LOSS_EPS);
        v -= ys * logf(c);
        if (q >= DIB_LOSS_EPS && q <= 1.f - DIB_LOSS_EPS) aq -= ys;   // a_k q_k = -(y_k / q_k) q_k
      }
      lrow = dib_grp_sum<LANES>(v);
      aq = dib_grp_sum<LANES>(aq);
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k], q = pk * rS, ys = y[k] * ya + yb;
        const float a = (q >= DIB_LOSS_EPS && q <= 1.f - DIB_LOSS_EPS) ? -ys / q : 0.f;
        g[k] = (a - aq) * rS * inv_bg * dib_act_grad(out_act, pk);
      }
    } else {  // DIB_LOSS_SPARSE_CCE on probabilities
      float sc = 0.f;
      for (int k = lane; k < n; k += LANES) sc += fminf(fmaxf(p[k], DIB_LOSS_EPS), 1.f - DIB_LOSS_EPS);
      sc = dib_grp_sum<LANES>(sc);
      const float plab = valid ? p[lab] : 1.f;
      const float rsc = 1.f / sc;
      lrow = logf(sc) - logf(fminf(fmaxf(plab, DIB_LOSS_EPS), 1.f - DIB_LOSS_EPS));
      for (int k = lane; k < n; k += LANES) {
        const float pk = p[k];
        const float gg = (pk < DIB_LOSS_EPS || pk > 1.f - DIB_LOSS_EPS) ? 0.f : rsc - (k == lab ? 1.f / pk : 0.f);
        g[k] = gg * inv_bg * dib_act_grad(out_act, pk);
      }
    }
    if (lane == 0 && valid) { lsum += lrow; msum += mrow; }
  }
  const float tl = dib_block_sum_256(lsum, red);
  const float tm = dib_block_sum_256(msum, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = tl;
    partial[2 * blockIdx.x + 1] = tm;
  }
}
