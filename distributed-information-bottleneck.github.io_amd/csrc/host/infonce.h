// host/infonce.h - dib_infonce_fwd_bwd (include/dib_hip.h): the one-launch kernel, the MFMA path (csrc/dib_infonce_mfma.h) and the
// VALU path of the l1 / linf similarities.

extern "C" {

int64_t dib_infonce_workspace_bytes(int batch) {
  if (batch <= 0) return DIB_E_ARG;
  // VALU path (l1, linf): S, ST, C, CT, C2, C2T [B^2 floats each] | arg-max, its transpose [B^2 int32 each] | lse [2B] | norms [2B]
  // MFMA path (l2sq, l2, cosine; csrc/dib_infonce_mfma.h): S [B^2] | 32-wide block partials of the row / column log-sum-exp
  // [4 ceil(B/32) B] inside the same 8 B^2 | lse | norms | slice partials of C . Other [2 x 8 x B x 256 at most] and of the row
  // sums [2 x 8 x B]
  return (int64_t)sizeof(float) * (8ll * batch * batch + 4ll * batch + 64 + (4096ll + 16ll) * batch + 64);
}

int dib_infonce_fwd_bwd(const float* emb_x, const float* emb_y, int batch, int dim, int similarity, float temperature,
                        float* g_x, float* g_y, float* loss_out, void* ws, dib_stream_t stream) {
  if (!emb_x || !emb_y || !loss_out || !ws || batch <= 0 || dim <= 0 || temperature <= 0.f) return DIB_E_ARG;
  if (similarity < 0 || similarity > 4 || dim > 256) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t bb = (int64_t)batch * batch;
  float* S = (float*)ws;
  float* ST = S + bb;
  float* C = ST + bb;
  float* CT = C + bb;
  float* C2 = CT + bb;
  float* C2T = C2 + bb;
  int* amax = (int*)(C2T + bb);
  int* amaxT = amax + bb;
  float* lse = (float*)(amaxT + bb);
  float* norms = lse + 2ll * batch;
  const float inv_t = 1.0f / temperature;
  const int tiles = cdiv(batch, 32);
  ProfScope ps(kProfOther, st);
  if ((similarity == 0 || similarity == 1 || similarity == 4) && batch <= DIB_INCE1_MAXB && dim <= 64 && knobs().infonce_one_launch) {
    // the reference's default batch: similarity, log-sum-exps, loss and both gradients in ONE launch (dib_infonce_small_kernel)
    const bool grads = g_x && g_y;
    const dim3 grid(grads ? cdiv(batch, 64) : 1, grads ? 2 : 1);
    const size_t lds = (size_t)DIB_INCE1_LDS_FLOATS * sizeof(float);
#define DIB_INCE_ONE(KD)                                                                                                           \
    launch_lds<&dib_infonce_small_kernel<KD>>(grid, dim3(DIB_INCE1_THREADS), lds, st, emb_x, emb_y, batch, dim, inv_t, temperature, \
                                              grads ? g_x : (float*)nullptr, grads ? g_y : (float*)nullptr, loss_out)
    return similarity == 0 ? DIB_INCE_ONE(0) : (similarity == 1 ? DIB_INCE_ONE(1) : DIB_INCE_ONE(4));
#undef DIB_INCE_ONE
  }
  if (similarity == 0 || similarity == 1 || similarity == 4) {
    // dot-product similarities: S, g_x = C Y, g_y = C^T X as three MFMA products (csrc/dib_infonce_mfma.h)
    const int nb32 = cdiv(batch, 32), t64 = cdiv(batch, 64);
    float* prow = S + bb;
    float* pcol = prow + 2ll * nb32 * batch;
    unsigned* arrive = (unsigned*)(norms + 2ll * batch + 16);
    float* Gp = norms + 2ll * batch + 64;
    // partner slices per (self block, side): one up to B = 256 (the gradient kernel then writes g itself: 3 launches in all);
    // above, enough workgroups to fill 256 CUs twice, at most 8 (the partial buffers' size)
    const int nsplit = t64 <= 4 ? 1 : std::max(1, std::min(std::min(t64, 8), cdiv(512, 2 * t64)));
    float* Rp = Gp + 2ll * nsplit * batch * dim;
    const int nacc = cdiv(dim, 64);
    const size_t os_bytes = (size_t)64 * (64 * nacc + 4) * sizeof(float);
#define DIB_INCE_SIM(KD) DIB_LAUNCH(dib_infonce_sim_mfma_kernel<KD>, dim3(t64, t64), dim3(256), 0, st, emb_x, emb_y, batch, \
                                            dim, inv_t, norms, S, prow, pcol, nb32, arrive)
    if (similarity == 0) DIB_INCE_SIM(0); else if (similarity == 1) DIB_INCE_SIM(1); else DIB_INCE_SIM(4);
#undef DIB_INCE_SIM
    float* lpart = pcol + 2ll * nb32 * batch;   // one loss partial per lse workgroup (still inside the 8 B^2 region)
    DIB_LAUNCH(dib_infonce_lse_loss_kernel, dim3(cdiv(2 * batch, 32)), dim3(256), 0, st, (const float*)prow,
                       (const float*)pcol, (const float*)S, batch, nb32, lse, arrive, lpart, loss_out);
    if (g_x && g_y) {
      const dim3 grid(t64, nsplit, 2);
      // (the output staging of the widest instantiation, 4 accumulators of 64 columns, is 66 560 bytes: launch_lds raises its limit)
#define DIB_INCE_GRAD(NA, KD) launch_lds<&dib_infonce_grad_mfma_kernel<NA, KD>>(grid, dim3(256), os_bytes, st, emb_x, emb_y,           \
                                                 (const float*)S, (const float*)lse, (const float*)norms, batch, dim, inv_t,            \
                                                 temperature, nsplit, Gp, Rp, g_x, g_y)
#define DIB_INCE_GRAD_K(KD) (nacc == 1 ? DIB_INCE_GRAD(1, KD) : nacc == 2 ? DIB_INCE_GRAD(2, KD)                             \
                                       : nacc == 3 ? DIB_INCE_GRAD(3, KD) : DIB_INCE_GRAD(4, KD))
      if (int rc = similarity == 0 ? DIB_INCE_GRAD_K(0) : (similarity == 1 ? DIB_INCE_GRAD_K(1) : DIB_INCE_GRAD_K(4))) return rc;
#undef DIB_INCE_GRAD_K
#undef DIB_INCE_GRAD
      if (nsplit > 1)
        DIB_LAUNCH(dib_infonce_grad_final_kernel, dim3(cdiv(2ll * batch * dim, 256)), dim3(256), 0, st, emb_x, emb_y,
                           (const float*)Gp, (const float*)Rp, batch, dim, similarity, nsplit, g_x, g_y);
    }
    return (int)hipGetLastError();
  }
  // two 32-row tiles of up to 256 (+1) floats: 65 792 bytes at the widest
  if (int rc = launch_lds<&dib_infonce_sim_kernel>(dim3(tiles, tiles), dim3(256), (size_t)2 * 32 * (dim + 1) * sizeof(float), st, emb_x,
                                                   emb_y, batch, dim, similarity, inv_t, (const float*)norms, S, ST, amax, amaxT))
    return rc;
  DIB_LAUNCH(dib_infonce_lse_kernel, dim3(batch, 2), dim3(256), 0, st, (const float*)S, (const float*)ST, batch, lse);
  DIB_LAUNCH(dib_infonce_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)S, (const float*)lse, batch,
                     loss_out);
  if (g_x && g_y) {
    DIB_LAUNCH(dib_infonce_coef_kernel, dim3(grid_for(bb, 256, 2048), 2), dim3(256), 0, st, (const float*)S,
                       (const float*)ST, (const float*)lse, (const float*)norms, batch, similarity, inv_t, temperature, C, CT, C2,
                       C2T);
    DIB_LAUNCH(dib_infonce_grad_kernel, dim3(batch, 2), dim3(256), 256 * sizeof(float), st, emb_x, emb_y,
                       (const float*)C, (const float*)CT, (const float*)C2, (const float*)C2T, (const int*)amax,
                       (const int*)amaxT, batch, dim, similarity, g_x, g_y);
  }
  return (int)hipGetLastError();
}

// ---- R independent problems [R][B][D] in the launches of one: the dot-product similarities on both routes above, the replica
// as a grid index (csrc/dib_infonce_mfma.h, the batched kernels).  Replica r's workspace is `ince_batched_map(batch).stride` floats
// on from replica r - 1's: S [B^2] | row / column block partials [4 ceil(B/32) B] | loss partials [ceil(2B/32)] | lse [2B] |
// norms [2B] | arrival counter | slice partials of C . Other and of the row sums, sized as the single entry point sizes them
// (the B^2 tables of the l1 / linf path, 7/8 of that workspace at B = 2048, are not needed here). ----
struct InceBatchedMap { long long prow, pcol, lpart, lse, norms, stride; };
static InceBatchedMap ince_batched_map(int batch) {
  const long long B = batch, nb32 = cdiv(batch, 32);
  InceBatchedMap m;
  m.prow = B * B;
  m.pcol = m.prow + 2 * nb32 * B;
  m.lpart = m.pcol + 2 * nb32 * B;
  m.lse = (m.lpart + cdiv(2 * batch, 32) + 3) / 4 * 4;
  m.norms = m.lse + 2 * B;
  m.stride = (m.norms + 2 * B + 64 + (4096ll + 16ll) * B + 3) / 4 * 4;
  return m;
}

int64_t dib_infonce_batched_workspace_bytes(int replicas, int batch) {
  if (batch <= 0 || replicas <= 0) return DIB_E_ARG;
  return (int64_t)replicas * ince_batched_map(batch).stride * (int64_t)sizeof(float);
}

int dib_infonce_fwd_bwd_batched(const float* emb_x, const float* emb_y, int replicas, int batch, int dim, int similarity,
                                float temperature, float* g_x, float* g_y, float* loss_out, void* ws, dib_stream_t stream) {
  if (!emb_x || !emb_y || !loss_out || !ws || replicas <= 0 || batch <= 0 || dim <= 0 || temperature <= 0.f) return DIB_E_ARG;
  if (!(similarity == 0 || similarity == 1 || similarity == 4) || dim > 256 || replicas > 32767) return DIB_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int R = replicas;
  const bool grads = g_x && g_y;
  const float inv_t = 1.0f / temperature;
  const InceBatchedMap map = ince_batched_map(batch);
  const long long stride = map.stride;   // a multiple of 4 floats
  ProfScope ps(kProfOther, st);
  if (batch <= DIB_INCE1_MAXB && dim <= 64 && knobs().infonce_one_launch) {
    const dim3 grid(grads ? cdiv(batch, 64) : 1, grads ? 2 : 1, R);
    const size_t lds = (size_t)DIB_INCE1_LDS_FLOATS * sizeof(float);
#define DIB_INCE_ONE(KD)                                                                                                        \
    launch_lds<&dib_infonce_batched_small_kernel<KD>>(grid, dim3(DIB_INCE1_THREADS), lds, st, emb_x, emb_y, batch, dim, inv_t,   \
                                                      temperature, grads ? g_x : (float*)nullptr, grads ? g_y : (float*)nullptr, \
                                                      loss_out)
    return similarity == 0 ? DIB_INCE_ONE(0) : (similarity == 1 ? DIB_INCE_ONE(1) : DIB_INCE_ONE(4));
#undef DIB_INCE_ONE
  }
  // replica 0's regions
  float* S = (float*)ws;
  float* lse = S + map.lse;
  float* norms = S + map.norms;
  const int nb32 = cdiv(batch, 32), t64 = cdiv(batch, 64);
  float* prow = S + map.prow;
  float* pcol = S + map.pcol;
  unsigned* arrive = (unsigned*)(norms + 2ll * batch + 16);
  float* Gp = norms + 2ll * batch + 64;
  const int nsplit = t64 <= 4 ? 1 : std::max(1, std::min(std::min(t64, 8), cdiv(512, 2 * t64)));
  float* Rp = Gp + 2ll * nsplit * batch * dim;
  const int nacc = cdiv(dim, 64);
  const size_t os_bytes = (size_t)64 * (64 * nacc + 4) * sizeof(float);
#define DIB_INCE_SIM(KD) DIB_LAUNCH(dib_infonce_batched_sim_kernel<KD>, dim3(t64, t64, R), dim3(256), 0, st, emb_x, emb_y, batch, \
                                    dim, inv_t, norms, S, prow, pcol, nb32, arrive, stride)
  if (similarity == 0) DIB_INCE_SIM(0); else if (similarity == 1) DIB_INCE_SIM(1); else DIB_INCE_SIM(4);
#undef DIB_INCE_SIM
  float* lpart = S + map.lpart;
  DIB_LAUNCH(dib_infonce_batched_lse_loss_kernel, dim3(cdiv(2 * batch, 32), R), dim3(256), 0, st, (const float*)prow,
             (const float*)pcol, (const float*)S, batch, nb32, lse, arrive, lpart, loss_out, stride);
  if (grads) {
    const dim3 grid(t64, nsplit, 2 * R);
#define DIB_INCE_GRAD(NA, KD) launch_lds<&dib_infonce_batched_grad_kernel<NA, KD>>(grid, dim3(256), os_bytes, st, emb_x, emb_y,    \
                                                 (const float*)S, (const float*)lse, (const float*)norms, batch, dim, inv_t,    \
                                                 temperature, nsplit, Gp, Rp, g_x, g_y, stride)
#define DIB_INCE_GRAD_K(KD) (nacc == 1 ? DIB_INCE_GRAD(1, KD) : nacc == 2 ? DIB_INCE_GRAD(2, KD)                             \
                                       : nacc == 3 ? DIB_INCE_GRAD(3, KD) : DIB_INCE_GRAD(4, KD))
    if (int rc = similarity == 0 ? DIB_INCE_GRAD_K(0) : (similarity == 1 ? DIB_INCE_GRAD_K(1) : DIB_INCE_GRAD_K(4))) return rc;
#undef DIB_INCE_GRAD_K
#undef DIB_INCE_GRAD
    if (nsplit > 1)
      DIB_LAUNCH(dib_infonce_batched_grad_final_kernel, dim3(cdiv(2ll * batch * dim, 256), R), dim3(256), 0, st, emb_x, emb_y,
                 (const float*)Gp, (const float*)Rp, batch, dim, similarity, nsplit, g_x, g_y, stride);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
