/* dib_optimizers.h - C ABI of the Keras optimizer family on a flat fp32 parameter buffer, beyond dib_adam_step / dib_sgd_step
 * (dib_hip.h): the names tf.keras.optimizers.get() accepts in the reference (train.py:41, 128-129), with the update rules of
 * Keras optimizer_v2 (TF 2.x before 2.11, the generation SURVEY.md App. B pins Adam to).
 *
 * g = grads[i] * grad_scale, lr = lr_dev[0], t = *t_dev + 1; all state is fp32 and starts at 0 unless stated.  State slots are
 * passed in the order listed (s0, s1, s2); dib_optimizer_slots says how many a (kind, hyper) needs.
 *   DIB_OPT_SGD_MOMENTUM (momentum > 0)  slots a          a = momentum a - lr g;  w += a;  nesterov: w += momentum a - lr g
 *                                                         (momentum == 0 is dib_sgd_step: DIB_E_ARG here)
 *   DIB_OPT_RMSPROP   slots r, [mg if centered], [mom if momentum > 0]
 *                                                         r = rho r + (1 - rho) g^2;  den = r;
 *                                                         centered: mg = rho mg + (1 - rho) g, den = r - mg^2
 *                                                         momentum == 0: w -= lr g / (sqrt(den) + eps)
 *                                                         momentum  > 0: mom = momentum mom + lr g / sqrt(den + eps);  w -= mom
 *   DIB_OPT_ADAGRAD   slots a (starts at initial_accumulator)   a += g^2;  w -= lr g / (sqrt(a) + eps)
 *   DIB_OPT_ADADELTA  slots a, d                          a = rho a + (1 - rho) g^2;  u = g sqrt(d + eps) / sqrt(a + eps);
 *                                                         d = rho d + (1 - rho) u^2;  w -= lr u
 *   DIB_OPT_ADAMAX    slots m, u                          m = b1 m + (1 - b1) g;  u = max(b2 u, |g|);
 *                                                         w -= lr / (1 - b1^t) m / (u + eps)
 *   DIB_OPT_NADAM     slots m, v; scalar_state P (one device float64, starts at 1)
 *                                                         u_t = b1 (1 - 0.5 0.96^(0.004 t)), u_{t+1} likewise;  P_t = P u_t;
 *                                                         P_next = P_t u_{t+1};  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 *                                                         w -= lr ((1 - u_t) g / (1 - P_t) + u_{t+1} m / (1 - P_next))
 *                                                                 / (sqrt(v / (1 - b2^t)) + eps);  the advance sets P = P_t
 *   DIB_OPT_AMSGRAD   slots m, v, vhat                    Adam's m, v;  vhat = max(vhat, v);
 *                                                         w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(vhat) + eps)
 * hyper->rho carries rho (RMSprop, Adadelta) or beta_1 (Adamax, Nadam, AMSGrad).
 *
 * dib_optimizer_slots is host-only (callable without a GPU): 0..3, DIB_E_ARG for an unknown kind or a NULL hyper.
 * dib_optimizer_init fills the state of n elements (one launch): s0 with the rule's start value, s1 / s2 with 0, *scalar_state
 * with 1.  dib_optimizer_step applies the rule to ONE contiguous range of n elements (one launch); it reads *t_dev and
 * *scalar_state and writes neither, so the ranges (gradient buckets) of one step can be stepped in any order, by separate launches,
 * and all see the same t and P.  dib_optimizer_advance (one thread, one launch) ends the step: P = P u_t for Nadam, *t_dev += 1.
 * Stepping a buffer in ranges and advancing once gives the bits of stepping it whole.
 *
 * Every entry returns int (DIB_OK or an error), never allocates, never synchronises, reads nothing from the environment and can
 * be captured into a hipGraph; the caller owns every buffer.  DIB_E_ARG: unknown kind, NULL hyper / params / grads / lr_dev / t_dev,
 * a slot the rule needs that is NULL (scalar_state for Nadam), n < 0, a parameter / gradient / slot pointer that is not 16-byte
 * aligned or a scalar_state that is not 8-byte aligned.  A refused call launches nothing; a step with n == 0 is DIB_OK without a launch.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_OPTIMIZERS_H
#define DIB_OPTIMIZERS_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_OPT_SGD_MOMENTUM 1
#define DIB_OPT_RMSPROP 2
#define DIB_OPT_ADAGRAD 3
#define DIB_OPT_ADADELTA 4
#define DIB_OPT_ADAMAX 5
#define DIB_OPT_NADAM 6
#define DIB_OPT_AMSGRAD 7

typedef struct dib_optimizer_hyper {
  float rho;                 /* rho (RMSprop, Adadelta) / beta_1 (Adamax, Nadam, AMSGrad) */
  float beta_2;              /* Adamax, Nadam, AMSGrad */
  float epsilon;
  float momentum;            /* SGD, RMSprop */
  float initial_accumulator; /* Adagrad */
  int32_t nesterov;          /* SGD */
  int32_t centered;          /* RMSprop */
  int32_t reserved;          /* 0 */
} dib_optimizer_hyper;

int dib_optimizer_slots(int kind, const dib_optimizer_hyper* hyper);
int dib_optimizer_init(int kind, const dib_optimizer_hyper* hyper, float* s0, float* s1, float* s2, int64_t n,
                       double* scalar_state, dib_stream_t stream);
int dib_optimizer_step(int kind, const dib_optimizer_hyper* hyper, float* params, const float* grads, float* s0, float* s1,
                       float* s2, int64_t n, const float* lr_dev, const int64_t* t_dev, const double* scalar_state,
                       float grad_scale, dib_stream_t stream);
int dib_optimizer_advance(int kind, const dib_optimizer_hyper* hyper, int64_t* t_dev, double* scalar_state, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_OPTIMIZERS_H */
