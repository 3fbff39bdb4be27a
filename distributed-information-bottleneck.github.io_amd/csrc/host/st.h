// host/st.h - set-transformer building blocks (include/dib_st.h): softmax, Add + LayerNorm, the token chain, pooling, attention,
// token KL and loss rows.  (The probe bounds and the information maps are in host/mi.h.)

static int ln_grid(int64_t T, int D) { return grid_for(T, D <= 32 ? 8 : 4, 512); }

// ---- the token-wise half of a set-transformer block in one launch per direction (csrc/dib_st_chain.h) ----------------
static_assert(sizeof(dib_st_block_desc) == sizeof(DibStChainDesc), "public block descriptor must mirror the kernel's");
// dynamic LDS bytes of the two kernels, from the LDS maps they carve from (dib_st_chain.h)
static size_t st_chain_fwd_lds(const DibStChainDesc& d) { return (size_t)dib_st_chain_fwd_lds<DibLdsFloats>(0, d).end * sizeof(float); }
static size_t st_chain_bwd_lds(const DibStChainDesc& d) { return (size_t)dib_st_chain_bwd_lds<DibLdsFloats>(0, d).end * sizeof(float); }

extern "C" {

int dib_softmax_rows_fwd(float* S, int64_t rows, int P, int ld, float scale, dib_stream_t stream) {
  if (!S || rows <= 0 || P <= 0 || ld < P) return DIB_E_ARG;
  const dim3 grid(grid_for(rows, 4, 8192));
  hipStream_t st = (hipStream_t)stream;
#define DIB_SM(R) DIB_LAUNCH(dib_softmax_rows_fwd_kernel<R>, grid, dim3(256), 0, st, S, (long long)rows, P, ld, scale)
  if (P <= 64) DIB_SM(1); else if (P <= 256) DIB_SM(4); else if (P <= 1024) DIB_SM(16); else if (P <= 4096) DIB_SM(64); else DIB_SM(0);
#undef DIB_SM
  return (int)hipGetLastError();
}

int dib_softmax_rows_bwd(const float* Pm, float* dP, int64_t rows, int P, int ld, float scale, dib_stream_t stream) {
  if (!Pm || !dP || rows <= 0 || P <= 0 || ld < P) return DIB_E_ARG;
  const dim3 grid(grid_for(rows, 4, 8192));
  hipStream_t st = (hipStream_t)stream;
#define DIB_SM(R) DIB_LAUNCH(dib_softmax_rows_bwd_kernel<R>, grid, dim3(256), 0, st, Pm, dP, (long long)rows, P, ld, scale)
  if (P <= 64) DIB_SM(1); else if (P <= 256) DIB_SM(4); else if (P <= 1024) DIB_SM(16); else if (P <= 4096) DIB_SM(64); else DIB_SM(0);
#undef DIB_SM
  return (int)hipGetLastError();
}

int dib_add_layernorm_fwd(const float* a, const float* b, int b_slabs, int64_t b_stride, int64_t T, int D, const float* gamma,
                          const float* beta, float eps, float* y, float* xhat, float* rstd, dib_stream_t stream) {
  if (!a || !b || !gamma || !beta || !y || !xhat || !rstd || T <= 0 || D <= 0 || b_slabs < 1) return DIB_E_ARG;
  if (D > 256) return DIB_E_UNSUPPORTED;
  if (D <= 32)
    DIB_LAUNCH(dib_add_layernorm_fwd_kernel<32>, dim3(ln_grid(T, D)), dim3(256), 0, (hipStream_t)stream, a, b, b_slabs,
                       (long long)b_stride, (long long)T, D, gamma, beta, eps, y, xhat, rstd);
  else
    DIB_LAUNCH(dib_add_layernorm_fwd_kernel<64>, dim3(ln_grid(T, D)), dim3(256), 0, (hipStream_t)stream, a, b, b_slabs,
                       (long long)b_stride, (long long)T, D, gamma, beta, eps, y, xhat, rstd);
  return (int)hipGetLastError();
}

int64_t dib_add_layernorm_bwd_workspace_bytes(int64_t T, int D) {
  if (T <= 0 || D <= 0 || D > 256) return DIB_E_ARG;
  return (int64_t)ln_grid(T, D) * 4 * (D <= 32 ? 2 : 1) * 2 * D * (int64_t)sizeof(float);
}

int dib_add_layernorm_bwd_fused(const float* dy, const float* dy2, const float* xhat, const float* rstd, const float* gamma,
                                int64_t T, int D, float* ds, const float* act_src, int act, float* dz, float* dgamma_dbeta,
                                void* ws, dib_stream_t stream) {
  if (!dy || !xhat || !rstd || !gamma || !ds || !dgamma_dbeta || !ws || T <= 0 || D <= 0) return DIB_E_ARG;
  if ((dz != nullptr) != (act_src != nullptr) || (dz && !act_ok(act))) return DIB_E_ARG;
  if (D > 256) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int grid = ln_grid(T, D);
  float* partial = (float*)ws;
  if (D <= 32)
    DIB_LAUNCH(dib_add_layernorm_bwd_kernel<32>, dim3(grid), dim3(256), 0, st, dy, dy2, xhat, rstd, gamma, (long long)T, D,
                       ds, act_src, act, dz, partial);
  else
    DIB_LAUNCH(dib_add_layernorm_bwd_kernel<64>, dim3(grid), dim3(256), 0, st, dy, dy2, xhat, rstd, gamma, (long long)T, D,
                       ds, act_src, act, dz, partial);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  // [gamma gradient (D) | beta gradient (D)] = fixed-order column sums of the per-slot partials
  DIB_LAUNCH(dib_colsum_partials_kernel, dim3(2 * D), dim3(256), 0, st, (const float*)partial,
                     grid * 4 * (D <= 32 ? 2 : 1), 2 * D, dgamma_dbeta);
  return (int)hipGetLastError();
}

int dib_add_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, int64_t T, int D,
                          float* ds, float* dgamma_dbeta, void* ws, dib_stream_t stream) {
  return dib_add_layernorm_bwd_fused(dy, nullptr, xhat, rstd, gamma, T, D, ds, nullptr, 0, nullptr, dgamma_dbeta, ws, stream);
}

int dib_st_chain_supported(const dib_st_block_desc* d, int64_t T) {
  if (!d || T <= 0 || !knobs().small_batch) return 0;
  if (d->D <= 0 || d->D % 32 || d->D > 256 || d->HK <= 0 || d->HK % 16 || d->n_ff < 1 || d->n_ff > DIB_ST_CHAIN_MAX_FF) return 0;
  if (d->act < 0 || d->act > 2) return 0;
  for (int l = 0; l < d->n_ff; ++l)
    if (d->ff_width[l] <= 0 || d->ff_width[l] % 16 || d->ff_width[l] > 1024) return 0;
  if (d->ff_width[d->n_ff - 1] != d->D) return 0;
  if (T > 4096) return 0;   // above: one tiled GEMM per layer reads each weight once per 64-128 rows instead of once per 16
  DibStChainDesc k;
  std::memcpy(&k, d, sizeof(k));
  return st_chain_fwd_lds(k) <= kSmallAdmitLds && st_chain_bwd_lds(k) <= kSmallAdmitLds;
}

int64_t dib_st_chain_workspace_bytes(int64_t T, int D) {
  if (T <= 0 || D <= 0) return DIB_E_ARG;
  return ((T + DIB_SMALL_ROWS - 1) / DIB_SMALL_ROWS * 4 * D + 64) * (int64_t)sizeof(float);
}

int dib_st_chain_fwd(const dib_st_block_desc* d, int64_t T, const float* params, const float* ctx, const float* x_in, float* h,
                     float* xhat1, float* rstd1, float* const* ff, float* x_out, float* xhat2, float* rstd2, dib_stream_t stream) {
  if (!d || !params || !ctx || !x_in || !h || !xhat1 || !rstd1 || !ff || !x_out || !xhat2 || !rstd2) return DIB_E_ARG;
  if (!dib_st_chain_supported(d, T)) return DIB_E_UNSUPPORTED;
  DibStChainFwdArgs a;
  std::memset(&a, 0, sizeof(a));
  std::memcpy(&a.d, d, sizeof(a.d));
  a.T = T; a.params = params; a.ctx = ctx; a.x_in = x_in; a.h = h; a.xhat1 = xhat1; a.rstd1 = rstd1;
  for (int l = 0; l < d->n_ff; ++l) { if (!ff[l]) return DIB_E_ARG; a.ff[l] = ff[l]; }
  a.x_out = x_out; a.xhat2 = xhat2; a.rstd2 = rstd2;
  const size_t lds = st_chain_fwd_lds(a.d);
  return launch_lds<&dib_st_chain_fwd_kernel>(dim3((unsigned)((T + DIB_SMALL_ROWS - 1) / DIB_SMALL_ROWS)), dim3(DIB_SMALL_THREADS), lds,
                                              (hipStream_t)stream, a);
}

int dib_st_chain_bwd(const dib_st_block_desc* d, int64_t T, const float* params, const float* g_out, int g_out_slabs,
                     int64_t g_out_stride, const float* xhat2, const float* rstd2, const float* const* ff, const float* xhat1,
                     const float* rstd1, float* const* g_ff, float* g_in, float* g_ctx, float* grads, void* ws, dib_stream_t stream) {
  if (!d || !params || !g_out || !xhat2 || !rstd2 || !ff || !xhat1 || !rstd1 || !g_ff || !g_in || !g_ctx || !grads || !ws)
    return DIB_E_ARG;
  if (g_out_slabs < 1 || (g_out_slabs > 1 && (g_out_stride < T * d->D || (g_out_stride & 3))) || ((uintptr_t)g_out & 15)) return DIB_E_ARG;
  if (!dib_st_chain_supported(d, T)) return DIB_E_UNSUPPORTED;
  DibStChainBwdArgs a;
  std::memset(&a, 0, sizeof(a));
  std::memcpy(&a.d, d, sizeof(a.d));
  a.T = T; a.params = params; a.g_out = g_out; a.g_slabs = g_out_slabs; a.g_stride = g_out_stride;
  a.xhat2 = xhat2; a.rstd2 = rstd2; a.xhat1 = xhat1; a.rstd1 = rstd1;
  for (int l = 0; l < d->n_ff; ++l) { if (!ff[l] || !g_ff[l]) return DIB_E_ARG; a.ff[l] = ff[l]; a.g_ff[l] = g_ff[l]; }
  a.g_in = g_in; a.g_ctx = g_ctx; a.grads = grads;
  const long long tiles = (T + DIB_SMALL_ROWS - 1) / DIB_SMALL_ROWS;
  a.ln_partial = (float*)ws;
  a.sync = (unsigned*)((float*)ws + tiles * 4 * d->D);   // zero at first use (the caller zero-fills the workspace once)
  const size_t lds = st_chain_bwd_lds(a.d);
  return launch_lds<&dib_st_chain_bwd_kernel>(dim3((unsigned)tiles), dim3(DIB_SMALL_THREADS), lds, (hipStream_t)stream, a);
}

int dib_mean_pool_fwd(const float* x, int B, int P, int D, float* out, dib_stream_t stream) {
  if (!x || !out || B <= 0 || P <= 0 || D <= 0) return DIB_E_ARG;
  DIB_LAUNCH(dib_mean_pool_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, B, P, D, out);
  return (int)hipGetLastError();
}

int dib_mean_pool_bwd(const float* g, int B, int P, int D, float* dx, dib_stream_t stream) {
  if (!g || !dx || B <= 0 || P <= 0 || D <= 0) return DIB_E_ARG;
  DIB_LAUNCH(dib_mean_pool_bwd_kernel, dim3(grid_for((int64_t)B * P * D)), dim3(256), 0, (hipStream_t)stream, g, B, P,
                     D, dx);
  return (int)hipGetLastError();
}

int dib_add_inplace(float* dst, const float* src, int64_t n, dib_stream_t stream) {
  if (!dst || !src || n <= 0) return DIB_E_ARG;
  DIB_LAUNCH(dib_add_inplace_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dst, src, (long long)n);
  return (int)hipGetLastError();
}

int64_t dib_attention_stash_bytes(int B, int P, int H) {
  if (B <= 0 || P <= 0 || H <= 0) return DIB_E_ARG;
  if (P <= kAttnSmallP) return 0;   // the single-workgroup path keeps the scores in LDS: nothing to stash
  const int64_t nt = cdiv(P, kAttnTile);
  return (int64_t)sizeof(float) * B * H * nt * nt * kAttnTile * kAttnTile;
}

int dib_attention_fwd(const float* q, const float* k, const float* v, int B, int P, int H, int key_dim, int64_t ld,
                      float scale, float* o, float* lse, float* s_stash, dib_stream_t stream) {
  if (!q || !k || !v || !o || !lse || B <= 0 || P <= 0 || H <= 0 || ld < (int64_t)H * key_dim || (ld & 3)) return DIB_E_ARG;
  if (key_dim != kAttnD || (int64_t)P * ld >= (1ll << 30)) return DIB_E_UNSUPPORTED;   // 32-bit row offsets inside one neighbourhood
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)s_stash) & 15) != 0) return DIB_E_ARG;
  DibAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.o = o; a.lse = lse; a.s_stash = s_stash; a.P = P; a.H = H; a.ld = ld; a.scale = scale;
  ProfScope ps(kProfAttnFwd, (hipStream_t)stream);
  if (P <= kAttnSmallP) {   // the whole head in LDS, one workgroup per (neighbourhood, head): csrc/dib_attn_small.h (no stash)
    const size_t lds = (size_t)DibAttnSmallFwdLds * sizeof(float);
    return launch_lds<&dib_attn_small_fwd_kernel<false>>(dim3(H, B), dim3(256), lds, (hipStream_t)stream, a);
  }
  if (knobs().attn_fwd_waves == 8 && P >= 256) DIB_LAUNCH(dib_attn_fwd8_kernel, dim3(cdiv(P, 256), H, B), dim3(512), 0, (hipStream_t)stream, a);
  else DIB_LAUNCH(dib_attn_fwd_kernel, dim3(cdiv(P, 128), H, B), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int dib_attention_fwd_proj_supported(int P, int key_dim, int model_dim) {
  return P >= 1 && P <= kAttnSmallP && key_dim == kAttnD && model_dim == 32;
}

int dib_attention_fwd_proj(const float* x, int64_t ldx, const float* params, const int64_t* w_off, const int64_t* b_off, int B, int P,
                           int H, int key_dim, int model_dim, int64_t ld, float scale, float* q, float* k, float* v, float* o,
                           float* lse, dib_stream_t stream) {
  if (!x || !params || !w_off || !b_off || !q || !k || !v || !o || !lse || B <= 0 || P <= 0 || H <= 0 || ldx < model_dim || (ldx & 3))
    return DIB_E_ARG;
  if (!dib_attention_fwd_proj_supported(P, key_dim, model_dim)) return DIB_E_UNSUPPORTED;
  if (ld != (int64_t)H * key_dim) return DIB_E_ARG;   // the projection kernels [model_dim][H * key_dim] share the outputs' leading dimension
  if ((((uintptr_t)x | (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) != 0) return DIB_E_ARG;
  DibAttnArgs a{};
  a.o = o; a.lse = lse; a.P = P; a.H = H; a.ld = ld; a.scale = scale;
  a.px = x; a.pldx = ldx; a.pparams = params; a.pq = q; a.pk = k; a.pv = v;
  for (int i = 0; i < 3; ++i) { a.pw[i] = w_off[i]; a.pb[i] = b_off[i]; }
  ProfScope ps(kProfAttnFwd, (hipStream_t)stream);
  const size_t lds = (size_t)DibAttnSmallFwdLds * sizeof(float);
  return launch_lds<&dib_attn_small_fwd_kernel<true>>(dim3(H, B), dim3(256), lds, (hipStream_t)stream, a);
}

int dib_attention_bwd_proj(const float* q, const float* k, const float* v, const float* d_o, const float* lse, int B, int P, int H,
                           int key_dim, int model_dim, int64_t ld, float scale, float* dq, float* dk, float* dv, const float* params,
                           const int64_t* w_off, float* dx_slabs, int64_t slab_stride, dib_stream_t stream) {
  if (!q || !k || !v || !d_o || !lse || !dq || !dk || !dv || !params || !w_off || !dx_slabs || B <= 0 || P <= 0 || H <= 0)
    return DIB_E_ARG;
  if (!dib_attention_fwd_proj_supported(P, key_dim, model_dim)) return DIB_E_UNSUPPORTED;
  if (ld != (int64_t)H * key_dim || slab_stride < (int64_t)B * P * model_dim || (slab_stride & 3)) return DIB_E_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)d_o | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv |
        (uintptr_t)dx_slabs) & 15) != 0)
    return DIB_E_ARG;
  DibAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.lse = const_cast<float*>(lse); a.d_o = d_o; a.dq = dq; a.dk = dk; a.dv = dv;
  a.P = P; a.H = H; a.ld = ld; a.scale = scale;
  a.pparams = params; a.pdx = dx_slabs; a.pdx_stride = slab_stride;
  for (int i = 0; i < 3; ++i) { if (w_off[i] & 3) return DIB_E_ARG; a.pw[i] = w_off[i]; }
  const size_t lds = (size_t)DibAttnSmallBwdLds * sizeof(float);
  ProfScope ps(kProfAttnBwd, (hipStream_t)stream);
  return launch_lds<&dib_attn_small_bwd8_kernel<true>>(dim3(H, B), dim3(512), lds, (hipStream_t)stream, a);
}

int64_t dib_attention_bwd_workspace_bytes(int B, int P, int H) {
  if (B <= 0 || P <= 0 || H <= 0) return DIB_E_ARG;
  const int64_t nkb = cdiv(P, 128);
  return (int64_t)sizeof(float) * ((int64_t)B * H * P + (nkb > 1 ? (int64_t)B * H * nkb * P * kAttnD : 0) + 64);
}

int dib_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse,
                      const float* s_stash, int B, int P, int H, int key_dim, int64_t ld, float scale, float* dq, float* dk,
                      float* dv, void* ws, dib_stream_t stream) {
  if (!q || !k || !v || !o || !d_o || !lse || !dq || !dk || !dv || !ws || B <= 0 || P <= 0 || H <= 0 ||
      ld < (int64_t)H * key_dim || (ld & 3))
    return DIB_E_ARG;
  if (key_dim != kAttnD || (int64_t)P * ld >= (1ll << 30)) return DIB_E_UNSUPPORTED;   // 32-bit row offsets inside one neighbourhood
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv |
        (uintptr_t)ws | (uintptr_t)s_stash) & 15) != 0)
    return DIB_E_ARG;   // every one of them is accessed with 16-byte loads / stores
  hipStream_t st = (hipStream_t)stream;
  if (P <= kAttnSmallP) {   // csrc/dib_attn_small.h: one launch - delta, the score recompute and dQ/dK/dV inside one workgroup per head
    DibAttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.lse = const_cast<float*>(lse); a.d_o = d_o; a.dq = dq; a.dk = dk; a.dv = dv;
    a.P = P; a.H = H; a.ld = ld; a.scale = scale;
    const size_t lds = (size_t)DibAttnSmallBwdLds * sizeof(float);
    ProfScope ps(kProfAttnBwd, st);
    if (knobs().attn_small_bwd_waves >= 8) return launch_lds<&dib_attn_small_bwd8_kernel<false>>(dim3(H, B), dim3(512), lds, st, a);
    return launch_lds<&dib_attn_small_bwd_kernel>(dim3(H, B), dim3(256), lds, st, a);
  }
  float* delta = (float*)ws;
  float* part = delta + (((int64_t)B * H * P + 63) / 64) * 64;
  const int nkb = cdiv(P, 128);
  DIB_LAUNCH(dib_attn_delta_kernel, dim3(cdiv((int64_t)B * P * H, 4)), dim3(256), 0, st, o, d_o, (long long)ld, B, P, H,
                     delta);
  DibAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.lse = const_cast<float*>(lse); a.d_o = d_o; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
  a.s_stash = const_cast<float*>(s_stash);
  a.P = P; a.H = H; a.ld = ld; a.scale = scale;
  const size_t lds = (size_t)DibAttnBwdLds * sizeof(float);
  int rc;
  { ProfScope ps(kProfAttnBwd, st);
    rc = s_stash ? launch_lds<&dib_attn_bwd_kernel<true>>(dim3(nkb, H, B), dim3(256), lds, st, a, part, nkb)
                 : launch_lds<&dib_attn_bwd_kernel<false>>(dim3(nkb, H, B), dim3(256), lds, st, a, part, nkb); }
  if (rc) return rc;
  if (nkb > 1) {
    DIB_LAUNCH(dib_attn_dq_reduce_kernel, dim3(grid_for((int64_t)B * H * P * (kAttnD / 4))), dim3(256), 0, st,
                       (const float*)part, B, P, H, nkb, (long long)ld, scale, dq);
    rc = (int)hipGetLastError();
  }
  return rc;
}

#ifdef DIB_ATTN_TIMING
// diagnostic build only (not declared in include/): copy the phase timers of the last dib_attention_bwd to the host
int dib_attn_debug_read(long long* out16) {
  if (hipDeviceSynchronize() != hipSuccess) return DIB_E_ARG;
  return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(dib_attn_dbg), 16 * sizeof(long long));
}
#endif

int dib_act_grad_mul(const float* g, const float* y, int act, int64_t n, float* out, dib_stream_t stream) {
  if (!g || !y || !out || n <= 0 || !act_ok(act)) return DIB_E_ARG;
  DIB_LAUNCH(dib_act_grad_mul_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, y, act, (long long)n, out);
  return (int)hipGetLastError();
}

int64_t dib_token_kl_workspace_bytes(int64_t T, int E) {
  if (T <= 0 || T > 0x7fffffff || E <= 0 || (E + 3) / 4 > 256) return DIB_E_ARG;   // same limit as the fwd / bwd entries
  return (int64_t)cdiv(T, std::max(1, 256 / ((E + 3) / 4))) * (int64_t)sizeof(float);
}

int dib_token_reparam_kl_fwd(const float* enc_out, int64_t T, int E, float logvar_offset, uint64_t seed, uint32_t step,
                             const uint32_t* step_dev, int64_t row0, int deterministic, float* u, float* kl_sum, void* ws,
                             dib_stream_t stream) {
  if (!enc_out || !u || !kl_sum || !ws || T <= 0 || T > 0x7fffffff || E <= 0 || (E + 3) / 4 > 256) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = cdiv(T, std::max(1, 256 / ((E + 3) / 4)));
  DIB_LAUNCH(dib_reparam_kl_fwd_kernel, dim3(blocks, 1), dim3(256), 0, st, enc_out, u, (float*)ws, (const int*)nullptr,
                     (long long)row0, (int)T, 1, E, (unsigned long long)seed, (unsigned)step, deterministic ? 1 : 0,
                     (const unsigned*)step_dev, logvar_offset);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  DIB_LAUNCH(dib_colsum_partials_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, blocks, 1, kl_sum);
  return (int)hipGetLastError();
}

int dib_token_reparam_kl_bwd(const float* enc_out, const float* g_u, const float* u, int64_t T, int E, float logvar_offset,
                             const float* beta_dev, float inv_batch, float* d_enc_out, dib_stream_t stream) {
  if (!enc_out || !g_u || !u || !beta_dev || !d_enc_out || T <= 0 || T > 0x7fffffff || E <= 0 || (E + 3) / 4 > 256)
    return DIB_E_ARG;
  const int blocks = cdiv(T, std::max(1, 256 / ((E + 3) / 4)));
  DIB_LAUNCH(dib_reparam_kl_bwd_kernel, dim3(blocks, 1), dim3(256), 0, (hipStream_t)stream, enc_out, g_u, u, d_enc_out,
                     beta_dev, inv_batch, (int)T, 1, E, logvar_offset);
  return (int)hipGetLastError();
}

int64_t dib_loss_rows_workspace_bytes(int batch) {
  if (batch <= 0) return DIB_E_ARG;
  return (int64_t)cdiv(batch, 256) * 2 * (int64_t)sizeof(float);
}

int dib_loss_rows(int loss_kind, const float* pred, int out_dim, const float* y, int64_t ldy, int batch,
                  float inv_global_batch, float* g_pred, float* out3, void* ws, dib_stream_t stream) {
  if (!pred || !y || !g_pred || !out3 || !ws || batch <= 0 || out_dim <= 0) return DIB_E_ARG;
  if (loss_kind < 0 || loss_kind > 3) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = cdiv(batch, 256);
  DIB_LAUNCH(dib_loss_kernel, dim3(blocks), dim3(256), 0, st, loss_kind, pred, out_dim, y, (long long)ldy,
                     (const int*)nullptr, 0ll, batch, inv_global_batch, 0, g_pred, (float*)ws);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  DIB_LAUNCH(dib_loss_finalize_kernel, dim3(2), dim3(256), 0, st, (const float*)ws, blocks, (float)batch, out3);
  return (int)hipGetLastError();
}

}  // extern "C"
