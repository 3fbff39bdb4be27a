// dib_optimizers.h - the Keras optimizer_v2 family beyond Adam and plain SGD on the flat parameter buffer (reference train.py:41,
// 128-129: tf.keras.optimizers.get(name) accepts any Keras name): SGD with momentum / Nesterov, RMSprop (centered and momentum
// variants), Adagrad, Adadelta, Adamax, Nadam and AMSGrad-Adam.  include/dib_optimizers.h states the update rules.
//
// One kernel template, one instantiation per rule (RMSprop: one per (centered, momentum) pair): a float4 grid-stride pass over
// the range with a scalar tail for n & 3, the shape of dib_adam_kernel.  Everything that depends on the step alone - b^t, Nadam's
// momentum schedule and its running product P, the bias corrections - is computed once per thread into registers (Rule::coef),
// like dib_adam_coef.  The kernel only READS the step count and P: dib_opt_advance_kernel, one thread, launched after the last
// range of a step, bumps t and advances P - every workgroup and every bucket's launch of a data-parallel step must see the same
// (t, P), the hazard DIB_TAIL_BUMP documents.  Floating-point contraction is OFF in every rule (as in dib_adam_update): an
// element gets the same bits from the float4 body and from the scalar tail, so stepping a buffer in ranges equals stepping it whole.
#pragma once
#include "dib_common.h"

struct DibOptHyper { float b1, b2, eps, momentum, init_acc; int nesterov; };   // b1: beta_1, or rho of RMSprop / Adadelta

// Nadam's momentum schedule u_t = beta_1 (1 - 0.5 * 0.96^(0.004 t)): ONE definition for the step and the advance kernel
__device__ __forceinline__ float dib_nadam_mu(float b1, long long t) {
#pragma clang fp contract(off)
  return b1 * (1.0f - 0.5f * powf(0.96f, 0.004f * (float)t));
}

// ---- rules: kSlots state arrays (x0, x1, x2 in slot order), Coef = the per-step registers, update = one element -------------
struct DibOptSgdMomentum {   // a = momentum a - lr g; w += a   |   nesterov: w += momentum a - lr g
  static constexpr int kSlots = 1;
  struct Coef { float lr, mom, gscale; int nesterov; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long, const double*, float gs) {
    return Coef{lr, h.momentum, gs, h.nesterov};
  }
  static __device__ __forceinline__ void update(float& p, float& a, float&, float&, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float step = c.lr * (g * c.gscale);
    a = c.mom * a - step;
    p = c.nesterov ? p + (c.mom * a - step) : p + a;
  }
};

// r = rho r + (1 - rho) g^2; den = r, centered: mg = rho mg + (1 - rho) g, den = r - mg^2
// momentum == 0: w -= lr g / (sqrt(den) + eps)   |   momentum > 0: mom = momentum mom + lr g / sqrt(den + eps); w -= mom
// (Keras optimizer_v2 places epsilon differently in its two branches).  Slots in order: r, [mg], [mom].
template <bool CENTERED, bool MOMENTUM>
struct DibOptRmsprop {
  static constexpr int kSlots = 1 + (CENTERED ? 1 : 0) + (MOMENTUM ? 1 : 0);
  struct Coef { float lr, rho, one_rho, mom, eps, gscale; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long, const double*, float gs) {
    return Coef{lr, h.b1, 1.f - h.b1, h.momentum, h.eps, gs};
  }
  static __device__ __forceinline__ void update(float& p, float& r, float& x1, float& x2, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    r = c.rho * r + c.one_rho * (gg * gg);
    float den = r;
    if (CENTERED) {
      x1 = c.rho * x1 + c.one_rho * gg;
      den = r - x1 * x1;
    }
    if (MOMENTUM) {
      float& mom = CENTERED ? x2 : x1;
      mom = c.mom * mom + (c.lr * gg) / sqrtf(den + c.eps);
      p = p - mom;
    } else {
      p = p - (c.lr * gg) / (sqrtf(den) + c.eps);
    }
  }
};

struct DibOptAdagrad {   // a += g^2; w -= lr g / (sqrt(a) + eps)
  static constexpr int kSlots = 1;
  struct Coef { float lr, eps, gscale; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long, const double*, float gs) {
    return Coef{lr, h.eps, gs};
  }
  static __device__ __forceinline__ void update(float& p, float& a, float&, float&, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    a = a + gg * gg;
    p = p - (c.lr * gg) / (sqrtf(a) + c.eps);
  }
};

struct DibOptAdadelta {   // a = rho a + (1 - rho) g^2; u = g sqrt(d + eps) / sqrt(a + eps); d = rho d + (1 - rho) u^2; w -= lr u
  static constexpr int kSlots = 2;
  struct Coef { float lr, rho, one_rho, eps, gscale; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long, const double*, float gs) {
    return Coef{lr, h.b1, 1.f - h.b1, h.eps, gs};
  }
  static __device__ __forceinline__ void update(float& p, float& a, float& d, float&, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    a = c.rho * a + c.one_rho * (gg * gg);
    const float u = gg * sqrtf(d + c.eps) / sqrtf(a + c.eps);
    d = c.rho * d + c.one_rho * (u * u);
    p = p - c.lr * u;
  }
};

struct DibOptAdamax {   // m = b1 m + (1 - b1) g; u = max(b2 u, |g|); w -= lr / (1 - b1^t) m / (u + eps)
  static constexpr int kSlots = 2;
  struct Coef { float lr_t, b1, one_b1, b2, eps, gscale; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long t, const double*, float gs) {
#pragma clang fp contract(off)
    return Coef{lr / (1.0f - powf(h.b1, (float)t)), h.b1, 1.f - h.b1, h.b2, h.eps, gs};
  }
  static __device__ __forceinline__ void update(float& p, float& m, float& u, float&, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    m = c.b1 * m + c.one_b1 * gg;
    u = fmaxf(c.b2 * u, fabsf(gg));
    p = p - (c.lr_t * m) / (u + c.eps);
  }
};

// u_t = b1 (1 - 0.5 0.96^(0.004 t)); P_t = P u_t; P_next = P_t u_{t+1} (P: device float64, the product of u_1 .. u_{t-1});
// m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2
// w -= lr ((1 - u_t) g / (1 - P_t) + u_{t+1} m / (1 - P_next)) / (sqrt(v / (1 - b2^t)) + eps)
struct DibOptNadam {
  static constexpr int kSlots = 2;
  struct Coef { float lr, cg, cm, bc2, b1, one_b1, b2, one_b2, eps, gscale; };
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long t, const double* P, float gs) {
#pragma clang fp contract(off)
    const float u_t = dib_nadam_mu(h.b1, t), u_n = dib_nadam_mu(h.b1, t + 1);
    const double p_t = P[0] * (double)u_t;
    const double p_n = p_t * (double)u_n;
    Coef c;
    c.lr = lr;
    c.cg = (1.0f - u_t) / (float)(1.0 - p_t);
    c.cm = u_n / (float)(1.0 - p_n);
    c.bc2 = 1.0f - powf(h.b2, (float)t);
    c.b1 = h.b1; c.one_b1 = 1.f - h.b1; c.b2 = h.b2; c.one_b2 = 1.f - h.b2; c.eps = h.eps; c.gscale = gs;
    return c;
  }
  static __device__ __forceinline__ void update(float& p, float& m, float& v, float&, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    m = c.b1 * m + c.one_b1 * gg;
    v = c.b2 * v + c.one_b2 * (gg * gg);
    const float num = c.cg * gg + c.cm * m;
    p = p - (c.lr * num) / (sqrtf(v / c.bc2) + c.eps);
  }
};

struct DibOptAmsgrad {   // Adam's m, v (dib_adam_update's expressions); vhat = max(vhat, v); w -= lr_t m / (sqrt(vhat) + eps)
  static constexpr int kSlots = 3;
  typedef DibAdamCoef Coef;
  static __device__ __forceinline__ Coef coef(const DibOptHyper& h, float lr, long long t, const double*, float gs) {
    return dib_adam_coef(lr, t - 1, h.b1, h.b2, h.eps, gs);
  }
  static __device__ __forceinline__ void update(float& p, float& m, float& v, float& vhat, float g, const Coef& c) {
#pragma clang fp contract(off)
    const float gg = g * c.gscale;
    m = m + c.c1 * (gg - m);
    v = v + c.c2 * (gg * gg - v);
    vhat = fmaxf(vhat, v);
    p = p - (c.lr_t * m) / (sqrtf(vhat) + c.eps);
  }
};

// one rule on one contiguous range; t = *t_dev + 1 and *scalar_state (Nadam's P) are read, never written
template <class Rule>
__global__ void __launch_bounds__(256)
dib_opt_kernel(DibOptHyper h, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
               float* __restrict__ s2, long long n, const float* __restrict__ lr_dev, const long long* __restrict__ t_dev,
               const double* __restrict__ scalar_state, float gscale) {
  const typename Rule::Coef c = Rule::coef(h, lr_dev[0], t_dev[0] + 1, scalar_state, gscale);
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, d = a;
    a = reinterpret_cast<float4*>(s0)[i];
    if (Rule::kSlots > 1) b = reinterpret_cast<float4*>(s1)[i];
    if (Rule::kSlots > 2) d = reinterpret_cast<float4*>(s2)[i];
    Rule::update(pp.x, a.x, b.x, d.x, gg.x, c);
    Rule::update(pp.y, a.y, b.y, d.y, gg.y, c);
    Rule::update(pp.z, a.z, b.z, d.z, gg.z, c);
    Rule::update(pp.w, a.w, b.w, d.w, gg.w, c);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(s0)[i] = a;
    if (Rule::kSlots > 1) reinterpret_cast<float4*>(s1)[i] = b;
    if (Rule::kSlots > 2) reinterpret_cast<float4*>(s2)[i] = d;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    float b = 0.f, d = 0.f;
    if (Rule::kSlots > 1) b = s1[i];
    if (Rule::kSlots > 2) d = s2[i];
    Rule::update(p[i], s0[i], b, d, g[i], c);
    if (Rule::kSlots > 1) s1[i] = b;
    if (Rule::kSlots > 2) s2[i] = d;
  }
}

// state fill: slot 0 = v0 (Adagrad's initial accumulator, else 0), slots 1 / 2 = 0 where given, P = 1
__global__ void __launch_bounds__(256)
dib_opt_init_kernel(float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2, long long n, float v0,
                    double* __restrict__ scalar_state) {
  const long long n4 = n >> 2;
  const float4 f0 = make_float4(v0, v0, v0, v0), z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    if (s0) reinterpret_cast<float4*>(s0)[i] = f0;
    if (s1) reinterpret_cast<float4*>(s1)[i] = z;
    if (s2) reinterpret_cast<float4*>(s2)[i] = z;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    if (s0) s0[i] = v0;
    if (s1) s1[i] = 0.f;
    if (s2) s2[i] = 0.f;
  }
  if (scalar_state && blockIdx.x == 0 && threadIdx.x == 0) scalar_state[0] = 1.0;
}

// after the last range of a step: P *= u_t (Nadam, scalar_state != nullptr), then t += 1.  One thread.
__global__ void dib_opt_advance_kernel(float b1, long long* __restrict__ t_dev, double* __restrict__ scalar_state) {
  const long long t = t_dev[0] + 1;
  if (scalar_state) scalar_state[0] = scalar_state[0] * (double)dib_nadam_mu(b1, t);
  t_dev[0] = t;
}
