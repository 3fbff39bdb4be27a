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

// ---- R replicas per launch: the replica is a grid index (csrc/dib_circuit.h); ensembles above DIB_CIRCUIT_BATCH replicas are
// split into launches of that many ----
int dib_circuit_batched_supported(const int* G, int replicas, int B) {
  if (!G || replicas < 1) return 0;
  for (int r = 0; r < replicas; ++r) if (!dib_circuit_supported(G[r], B)) return 0;
  return 1;
}

// kind 0: forward, 1: backward.  `ba` holds the base pointers of replica 0; every chunk moves them to its first replica
static int circuit_launch_batched(int kind, const DibCircuitBatchArgs& ba0, int replicas, const int64_t* table_off, const int* G,
                                  const uint64_t* seeds, const float* beta, hipStream_t st) {
  for (int r0 = 0; r0 < replicas; r0 += DIB_CIRCUIT_BATCH) {
    const int n = std::min(replicas - r0, DIB_CIRCUIT_BATCH);
    const long long r = r0, B = ba0.B;
    DibCircuitBatchArgs ba = ba0;
    ba.params += r * ba.param_stride;
    if (ba.row_in) ba.row_in += r * B;
    ba.rows += r * B;
    if (kind == 0) { ba.u += r * B * DIB_CIRCUIT_LD; ba.y += r * B; ba.kl += r * (DIB_CIRCUIT_MAX_GATES + 1); }
    else { ba.g_u += r * B * DIB_CIRCUIT_LD; ba.grads += r * ba.grad_stride; }
    int gmax = 1;
    for (int i = 0; i < DIB_CIRCUIT_BATCH; ++i) {
      const bool on = i < n;
      ba.seeds[i] = on ? seeds[r0 + i] : 0; ba.beta[i] = on ? beta[r0 + i] : 0.f;
      ba.table_off[i] = on ? (int)table_off[r0 + i] : 0; ba.G[i] = on ? G[r0 + i] : 1;
      if (on) gmax = std::max(gmax, G[r0 + i]);
    }
    if (kind == 0) {
      DIB_LAUNCH(dib_circuit_batched_fwd_kernel, dim3(cdiv((int64_t)B * DIB_CIRCUIT_LD, 256), n), dim3(256), 0, st, ba);
    } else {
      DIB_LAUNCH(dib_circuit_batched_bwd_kernel, dim3(gmax, n), dim3(256), 0, st, ba);
    }
    if (int rc = (int)hipGetLastError()) return rc;
  }
  return DIB_OK;
}

// every replica's 2^G words lie inside the buffer of table_words words
static bool circuit_table_offsets_ok(const int64_t* table_off, const int* G, int replicas, int64_t table_words) {
  for (int r = 0; r < replicas; ++r)
    if (table_off[r] < 0 || table_off[r] > INT32_MAX || table_off[r] + ((int64_t)1 << G[r]) > table_words) return false;
  return true;
}

int dib_circuit_fwd_batched(const uint32_t* tables, int64_t table_words, const int64_t* table_off, const int* G, int replicas, int B, const float* params,
                            int64_t param_stride, int64_t sc_off, const uint64_t* seeds, uint32_t step, const float* beta,
                            const int32_t* row_idx, int32_t* rows_out, float* u, float* y, float* kl, dib_stream_t stream) {
  if (!G || !table_off || !seeds || !beta) return DIB_E_ARG;
  if (!dib_circuit_batched_supported(G, replicas, B)) return DIB_E_UNSUPPORTED;
  if (!tables || !params || param_stride < 0 || sc_off < 0 || !rows_out || !u || !y || !kl
      || !circuit_table_offsets_ok(table_off, G, replicas, table_words)) return DIB_E_ARG;
  DibCircuitBatchArgs ba;
  std::memset(&ba, 0, sizeof(ba));
  ba.tables = tables; ba.params = params; ba.param_stride = param_stride; ba.sc_off = sc_off; ba.B = B; ba.step = step;
  ba.row_in = row_idx; ba.rows = rows_out; ba.u = u; ba.y = y; ba.kl = kl;
  return circuit_launch_batched(0, ba, replicas, table_off, G, seeds, beta, (hipStream_t)stream);
}

int dib_circuit_bwd_batched(const uint32_t* tables, int64_t table_words, const int64_t* table_off, const int* G, int replicas, int B, const float* params,
                            int64_t param_stride, int64_t sc_off, const uint64_t* seeds, uint32_t step, const float* beta,
                            const int32_t* rows, const float* g_u, float* grads, int64_t grad_stride, dib_stream_t stream) {
  if (!G || !table_off || !seeds || !beta) return DIB_E_ARG;
  if (!dib_circuit_batched_supported(G, replicas, B)) return DIB_E_UNSUPPORTED;
  if (!tables || !params || param_stride < 0 || sc_off < 0 || !rows || !g_u || !grads || grad_stride < 0
      || !circuit_table_offsets_ok(table_off, G, replicas, table_words)) return DIB_E_ARG;
  DibCircuitBatchArgs ba;
  std::memset(&ba, 0, sizeof(ba));
  ba.tables = tables; ba.params = params; ba.param_stride = param_stride; ba.sc_off = sc_off; ba.B = B; ba.step = step;
  ba.rows = const_cast<int32_t*>(rows); ba.g_u = g_u; ba.grads = grads; ba.grad_stride = grad_stride;
  return circuit_launch_batched(1, ba, replicas, table_off, G, seeds, beta, (hipStream_t)stream);
}

// one slice per replica: the single kernel's workspace at G = 16 (a multiple of 256 bytes)
int64_t dib_circuit_mi_batched_workspace_bytes(int replicas, int n, int nb) {
  const int64_t one = dib_circuit_mi_workspace_bytes(DIB_CIRCUIT_MAX_GATES, n, nb);
  if (replicas < 1 || one < 0) return DIB_E_UNSUPPORTED;
  return (int64_t)replicas * one;
}

int dib_circuit_mi_bounds_batched(const float* params, int64_t param_stride, int64_t sc_off, const int* G, int replicas,
                                  const float* x, int n, int nb, const uint64_t* seeds, double* out, void* ws,
                                  dib_stream_t stream) {
  if (!G || !seeds) return DIB_E_ARG;
  if (dib_circuit_mi_batched_workspace_bytes(replicas, n, nb) < 0) return DIB_E_UNSUPPORTED;
  for (int r = 0; r < replicas; ++r) if (G[r] < 1 || G[r] > DIB_CIRCUIT_MAX_GATES) return DIB_E_UNSUPPORTED;
  if (!params || param_stride < 0 || sc_off < 0 || !x || !out || !ws) return DIB_E_ARG;
  const int chunks = cdiv(n, DIB_CIRCUIT_MI_ROWS);
  const int64_t one = dib_circuit_mi_workspace_bytes(DIB_CIRCUIT_MAX_GATES, n, nb);
  for (int r0 = 0; r0 < replicas; r0 += DIB_CIRCUIT_BATCH) {
    const int m = std::min(replicas - r0, DIB_CIRCUIT_BATCH);
    DibCircuitMiBatchArgs ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.params = params + (int64_t)r0 * param_stride; ba.param_stride = param_stride; ba.sc_off = sc_off;
    ba.xs = x + (int64_t)r0 * nb * n; ba.n = n; ba.nb = nb;
    ba.ws = (char*)ws + (int64_t)r0 * one; ba.ws_stride = one;
    ba.out = out + (int64_t)r0 * DIB_CIRCUIT_MAX_GATES * nb * 2;
    for (int i = 0; i < DIB_CIRCUIT_BATCH; ++i) { ba.seeds[i] = i < m ? seeds[r0 + i] : 0; ba.G[i] = i < m ? G[r0 + i] : 1; }
    DIB_LAUNCH(dib_circuit_batched_mi_kernel, dim3(chunks, nb, DIB_CIRCUIT_MAX_GATES * m), dim3(256), 0, (hipStream_t)stream, ba);
    if (int rc = (int)hipGetLastError()) return rc;
  }
  return DIB_OK;
}

}  // extern "C"
