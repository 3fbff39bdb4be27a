// host/circuit.h - the Boolean-circuit model (include/dib_circuit.h, csrc/dib_circuit.h).

static_assert(DIB_CIRCUIT_U_LD == DIB_CIRCUIT_LD, "include/dib_circuit.h and csrc/dib_circuit.h disagree on u's pitch");

extern "C" {

int dib_circuit_supported(int G, int B) {
  return G >= 1 && G <= DIB_CIRCUIT_MAX_GATES && B >= 1 && B <= DIB_CIRCUIT_MAX_BATCH ? 1 : 0;
}

int dib_circuit_fwd(const uint32_t* table, int G, int B, const float* sc, uint64_t seed, uint32_t step, float beta,
                    const int32_t* row_idx, int32_t* rows_out, float* u, float* y, float* kl, dib_stream_t stream) {
  if (!dib_circuit_supported(G, B)) return DIB_E_UNSUPPORTED;
  if (!table || !sc || !rows_out || !u || !y || !kl) return DIB_E_ARG;
  DIB_LAUNCH(dib_circuit_fwd_kernel, dim3(cdiv((int64_t)B * DIB_CIRCUIT_LD, 256)), dim3(256), 0, (hipStream_t)stream, table, G, B,
             sc, (unsigned long long)seed, (unsigned)step, beta, row_idx, rows_out, u, y, kl);
  return (int)hipGetLastError();
}

int dib_circuit_bwd(const uint32_t* table, int G, int B, const float* sc, uint64_t seed, uint32_t step, float beta,
                    const int32_t* rows, const float* g_u, float* g_sc, dib_stream_t stream) {
  if (!dib_circuit_supported(G, B)) return DIB_E_UNSUPPORTED;
  if (!table || !sc || !rows || !g_u || !g_sc) return DIB_E_ARG;
  DIB_LAUNCH(dib_circuit_bwd_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, table, G, B, sc, (unsigned long long)seed,
             (unsigned)step, beta, rows, g_u, g_sc);
  return (int)hipGetLastError();
}

int64_t dib_circuit_mi_workspace_bytes(int G, int n, int nb) {
  if (G < 1 || G > DIB_CIRCUIT_MAX_GATES || n < 2 || nb < 1 || nb > 65535) return DIB_E_UNSUPPORTED;
  return (int64_t)G * nb * cdiv(n, DIB_CIRCUIT_MI_ROWS) * 2 * (int64_t)sizeof(double) + align_up((int64_t)G * nb, 64) * (int64_t)sizeof(unsigned);
}

int dib_circuit_mi_bounds(const float* sc, int G, const float* x, int n, int nb, uint64_t seed, double* out, void* ws,
                          dib_stream_t stream) {
  if (dib_circuit_mi_workspace_bytes(G, n, nb) < 0) return DIB_E_UNSUPPORTED;
  if (!sc || !x || !out || !ws) return DIB_E_ARG;
  const int chunks = cdiv(n, DIB_CIRCUIT_MI_ROWS);
  double* parts = (double*)ws;
  unsigned* counters = (unsigned*)(parts + (int64_t)G * nb * chunks * 2);
  DIB_LAUNCH(dib_circuit_mi_kernel, dim3(chunks, nb, G), dim3(256), 0, (hipStream_t)stream, sc, G, x, n, nb, (unsigned long long)seed,
             parts, counters, out);
  return (int)hipGetLastError();
}

}  // extern "C"
