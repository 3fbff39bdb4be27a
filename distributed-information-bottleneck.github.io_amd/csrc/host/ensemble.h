// host/ensemble.h - the lockstep DistributedIBNet ensemble's entry points (include/dib_ensemble.h, csrc/dib_ensemble.h).

namespace {

constexpr int kEnsMaxGroups = 65535, kEnsMaxE = 1024, kEnsMaxRows = 2048, kEnsMaxOut = 16;

inline int ens_kl_blocks(int E, int n) { return cdiv(n, 256 / ((E + 3) / 4)); }   // dib_reparam_kl_fwd_kernel's row tiles
inline int ens_loss_blocks(int n) { return cdiv(n, 256); }
inline bool ens_shape_ok(int R, int F, int n) {
  return R >= 1 && F >= 1 && (int64_t)R * F <= kEnsMaxGroups && n >= 1 && n <= kEnsMaxRows;
}

// the workspace, in 4-byte words: loss partials [R][loss_blocks][2] | loss counters [R] | KL counters [R F] | KL partials
// [R][kl_blocks][F] - only the last region's size depends on E, so the loss entry finds its regions without knowing it
struct EnsWs { float* loss_parts; unsigned* loss_counters; unsigned* kl_counters; float* kl_parts; };
inline EnsWs ens_ws(void* ws, int R, int F, int n) {
  float* p = (float*)ws;
  const int64_t a = (int64_t)R * ens_loss_blocks(n) * 2, b = R, c = (int64_t)R * F;
  return {p, (unsigned*)(p + a), (unsigned*)(p + a + b), p + a + b + c};
}

}  // namespace

extern "C" {

int dib_ens_supported(int R, int F, int E, int n, int out_dim, int kind) {
  return ens_shape_ok(R, F, n) && E >= 1 && E <= kEnsMaxE && out_dim >= 1 && out_dim <= kEnsMaxOut
         && (kind == 0 || kind == 2 || kind == 3) ? 1 : 0;
}

int64_t dib_ens_workspace_bytes(int R, int F, int E, int n) {
  if (!dib_ens_supported(R, F, E, n, 1, 0)) return DIB_E_UNSUPPORTED;
  const int64_t words = (int64_t)R * ens_loss_blocks(n) * 2 + R + (int64_t)R * F + (int64_t)R * ens_kl_blocks(E, n) * F;
  return align_up(words) * (int64_t)sizeof(float);
}

int dib_ens_posenc_rows(const float* x, int64_t ldx, const int32_t* rows, int R, int F, int d, int n_blocks, int n, float* out,
                        dib_stream_t stream) {
  if (!ens_shape_ok(R, F, n) || d < 1 || n_blocks < 1 || n_blocks > 32 || (int64_t)F * d > INT32_MAX / 2) return DIB_E_UNSUPPORTED;
  if (!x || !rows || !out || ldx < (int64_t)F * d) return DIB_E_ARG;
  DIB_LAUNCH(dib_ens_posenc_rows_kernel, dim3(cdiv((int64_t)F * d, 64), cdiv(n, DIB_ENS_POSENC_ROWS), R), dim3(256), 0,
             (hipStream_t)stream, x, (long long)ldx, rows, n, F, d, n_blocks, out);
  return (int)hipGetLastError();
}

int dib_ens_reparam_kl_fwd(const float* enc, const int32_t* rows, const uint64_t* seeds, uint32_t step, int deterministic, int R,
                           int F, int E, int n, float* u, float* kl, void* ws, dib_stream_t stream) {
  if (!dib_ens_supported(R, F, E, n, 1, 0)) return DIB_E_UNSUPPORTED;
  if (!enc || !rows || !seeds || !u || !kl || !ws) return DIB_E_ARG;
  const EnsWs w = ens_ws(ws, R, F, n);
  DIB_LAUNCH(dib_ens_reparam_kl_fwd_kernel, dim3(ens_kl_blocks(E, n), F, R), dim3(256), 0, (hipStream_t)stream, enc, u, w.kl_parts,
             w.kl_counters, kl, rows, n, F, E, (const unsigned long long*)seeds, (unsigned)step, deterministic);
  return (int)hipGetLastError();
}

int dib_ens_loss(int kind, const float* pred, int out_dim, const float* y, int64_t ldy, const int32_t* rows, int R, int F, int n,
                 float inv_b, int out_act, const float* beta, const float* kl, float* g_pred, float* metrics_acc, void* ws,
                 dib_stream_t stream) {
  if (!dib_ens_supported(R, F, 1, n, out_dim, kind)) return DIB_E_UNSUPPORTED;
  if (!pred || !y || !rows || !beta || !kl || !g_pred || !metrics_acc || !ws || ldy < (kind == 2 ? 1 : out_dim) || !act_ok(out_act))
    return DIB_E_ARG;
  const EnsWs w = ens_ws(ws, R, F, n);
  DIB_LAUNCH(dib_ens_loss_kernel, dim3(ens_loss_blocks(n), R), dim3(256), 0, (hipStream_t)stream, kind, pred, out_dim, y,
             (long long)ldy, rows, n, inv_b, out_act, g_pred, w.loss_parts, w.loss_counters, kl, F, beta, metrics_acc);
  return (int)hipGetLastError();
}

int dib_ens_reparam_kl_bwd(const float* enc, const float* g_u, const float* u, const float* beta, float inv_b, int R, int F, int E,
                           int n, float* d_enc, dib_stream_t stream) {
  if (!dib_ens_supported(R, F, E, n, 1, 0)) return DIB_E_UNSUPPORTED;
  if (!enc || !g_u || !u || !beta || !d_enc) return DIB_E_ARG;
  DIB_LAUNCH(dib_ens_reparam_kl_bwd_kernel, dim3(ens_kl_blocks(E, n), F, R), dim3(256), 0, (hipStream_t)stream, enc, g_u, u, d_enc,
             beta, inv_b, n, F, E);
  return (int)hipGetLastError();
}

}  // extern "C"
