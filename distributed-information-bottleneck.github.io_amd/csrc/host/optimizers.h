// host/optimizers.h - the Keras optimizer family on a flat buffer (include/dib_optimizers.h, csrc/dib_optimizers.h): argument
// checks, the slot count of a rule, and the three launches (state fill, one range of a step, the advance).

namespace {

int opt_slots(int kind, const dib_optimizer_hyper* h) {
  if (!h) return DIB_E_ARG;
  switch (kind) {
    case DIB_OPT_SGD_MOMENTUM: return h->momentum > 0.f ? 1 : 0;
    case DIB_OPT_RMSPROP: return 1 + (h->centered ? 1 : 0) + (h->momentum > 0.f ? 1 : 0);
    case DIB_OPT_ADAGRAD: return 1;
    case DIB_OPT_ADADELTA: case DIB_OPT_ADAMAX: case DIB_OPT_NADAM: return 2;
    case DIB_OPT_AMSGRAD: return 3;
    default: return DIB_E_ARG;
  }
}

inline bool opt_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the slots the rule needs are there and aligned; Nadam has its P
int opt_check_state(int kind, const dib_optimizer_hyper* h, const float* s0, const float* s1, const float* s2, int64_t n,
                    const double* scalar_state) {
  const int slots = opt_slots(kind, h);
  if (slots < 0 || n < 0) return DIB_E_ARG;
  if (kind == DIB_OPT_SGD_MOMENTUM && slots == 0) return DIB_E_ARG;   // momentum == 0: dib_sgd_step
  const float* s[3] = {s0, s1, s2};
  for (int k = 0; k < slots; ++k)
    if (!s[k] || !opt_aligned(s[k], 16)) return DIB_E_ARG;
  if (kind == DIB_OPT_NADAM && (!scalar_state || !opt_aligned(scalar_state, 8))) return DIB_E_ARG;
  return DIB_OK;
}

DibOptHyper opt_device_hyper(const dib_optimizer_hyper* h) {
  return DibOptHyper{h->rho, h->beta_2, h->epsilon, h->momentum, h->initial_accumulator, h->nesterov ? 1 : 0};
}

}  // namespace

extern "C" {

int dib_optimizer_slots(int kind, const dib_optimizer_hyper* hyper) { return opt_slots(kind, hyper); }

int dib_optimizer_init(int kind, const dib_optimizer_hyper* hyper, float* s0, float* s1, float* s2, int64_t n,
                       double* scalar_state, dib_stream_t stream) {
  if (int rc = opt_check_state(kind, hyper, s0, s1, s2, n, scalar_state)) return rc;
  const int slots = opt_slots(kind, hyper);
  if (n == 0 && kind != DIB_OPT_NADAM) return DIB_OK;
  ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_opt_init_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, s0, slots > 1 ? s1 : (float*)nullptr,
             slots > 2 ? s2 : (float*)nullptr, (long long)n, kind == DIB_OPT_ADAGRAD ? hyper->initial_accumulator : 0.f,
             kind == DIB_OPT_NADAM ? scalar_state : (double*)nullptr);
  return (int)hipGetLastError();
}

int dib_optimizer_step(int kind, const dib_optimizer_hyper* hyper, float* params, const float* grads, float* s0, float* s1,
                       float* s2, int64_t n, const float* lr_dev, const int64_t* t_dev, const double* scalar_state,
                       float grad_scale, dib_stream_t stream) {
  if (int rc = opt_check_state(kind, hyper, s0, s1, s2, n, scalar_state)) return rc;
  if (!params || !grads || !lr_dev || !t_dev || !opt_aligned(params, 16) || !opt_aligned(grads, 16)) return DIB_E_ARG;
  if (n == 0) return DIB_OK;
  hipStream_t st = (hipStream_t)stream;
  const DibOptHyper h = opt_device_hyper(hyper);
  const dim3 grid(grid_for(n / 4));
  ProfScope ps(kProfOther, st);
  typedef DibOptRmsprop<false, false> Rms;
  typedef DibOptRmsprop<false, true> RmsM;
  typedef DibOptRmsprop<true, false> RmsC;
  typedef DibOptRmsprop<true, true> RmsCM;
#define DIB_OPT_STEP(RULE) DIB_LAUNCH(dib_opt_kernel<RULE>, grid, dim3(256), 0, st, h, params, grads, s0, s1, s2, (long long)n, \
                                      lr_dev, (const long long*)t_dev, scalar_state, grad_scale)
  switch (kind) {
    case DIB_OPT_SGD_MOMENTUM: DIB_OPT_STEP(DibOptSgdMomentum); break;
    case DIB_OPT_RMSPROP:
      if (hyper->centered) { if (hyper->momentum > 0.f) DIB_OPT_STEP(RmsCM); else DIB_OPT_STEP(RmsC); }
      else { if (hyper->momentum > 0.f) DIB_OPT_STEP(RmsM); else DIB_OPT_STEP(Rms); }
      break;
    case DIB_OPT_ADAGRAD: DIB_OPT_STEP(DibOptAdagrad); break;
    case DIB_OPT_ADADELTA: DIB_OPT_STEP(DibOptAdadelta); break;
    case DIB_OPT_ADAMAX: DIB_OPT_STEP(DibOptAdamax); break;
    case DIB_OPT_NADAM: DIB_OPT_STEP(DibOptNadam); break;
    case DIB_OPT_AMSGRAD: DIB_OPT_STEP(DibOptAmsgrad); break;
    default: return DIB_E_ARG;
  }
#undef DIB_OPT_STEP
  return (int)hipGetLastError();
}

int dib_optimizer_advance(int kind, const dib_optimizer_hyper* hyper, int64_t* t_dev, double* scalar_state, dib_stream_t stream) {
  if (opt_slots(kind, hyper) < 0 || !t_dev) return DIB_E_ARG;
  if (kind == DIB_OPT_NADAM && (!scalar_state || !opt_aligned(scalar_state, 8))) return DIB_E_ARG;
  ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_opt_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper->rho, (long long*)t_dev,
             kind == DIB_OPT_NADAM ? scalar_state : (double*)nullptr);
  return (int)hipGetLastError();
}

}  // extern "C"
