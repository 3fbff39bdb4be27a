// host/ctw_levels.h - the device CTW estimator (include/dib_ctw_device.h; csrc/dib_ctw_levels.h): the envelope, the workspace
// map, the lgamma tables and the loop over levels.

// DIB_OK inside the envelope, else the code the entry point returns
static int ctw_envelope(int alphabet, int64_t total_symbols, int n_windows) {
  if (alphabet < 1 || total_symbols < 0 || n_windows < 0) return DIB_E_ARG;
  if (alphabet > DIB_CTW_DEVICE_MAX_ALPHABET || total_symbols > DIB_CTW_DEVICE_MAX_SYMBOLS) return DIB_E_UNSUPPORTED;
  return DIB_OK;
}

// most nodes one level can hold: every root at level 0, at most half the elements further down, never more than all nodes
static int64_t ctw_level_nodes(int64_t E, int W, int64_t node_capacity) {
  return std::max<int64_t>(1, std::min<int64_t>(node_capacity, std::max<int64_t>(W, E / 2)));
}

struct CtwWorkspace {   // byte offsets into ws, each a multiple of 256
  int64_t table_beta, table_ab, win_start, win_off, win_len, status, rec, el_t[2], el_node[2], node_win[2], hist_sym, hist_ctx,
      key_info, block_sums, node_L, node_count, node_mask, node_first, bytes;
};

static CtwWorkspace ctw_workspace(int64_t E, int W, int A, int64_t node_capacity) {
  CtwWorkspace m{};
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const int64_t here = at;
    at += (std::max<int64_t>(bytes, 1) + 255) / 256 * 256;
    return here;
  };
  const int64_t nl = ctw_level_nodes(E, W, node_capacity), keys = nl * A, w = std::max(W, 1), e = std::max<int64_t>(E, 1);
  m.table_beta = take(DIB_CTW_TABLE * 8);
  m.table_ab = take(DIB_CTW_TABLE * 8);
  m.win_start = take(w * 8);
  m.win_off = take((w + 1) * 4);
  m.win_len = take(w * 4);
  m.status = take(w * 4);
  m.rec = take((DIB_CTW_LAST_LEVEL + 1) * (int64_t)sizeof(DibCtwLevelRec));
  for (int k = 0; k < 2; ++k) {
    m.el_t[k] = take(e * 4);
    m.el_node[k] = take(e * 4);
    m.node_win[k] = take(nl * 4);
  }
  m.hist_sym = take(keys * 4);
  m.hist_ctx = take(keys * 4);
  m.key_info = take(keys * 8);
  m.block_sums = take((nl + DIB_CTW_THREADS - 1) / DIB_CTW_THREADS * 8);
  m.node_L = take(node_capacity * 8);
  m.node_count = take(node_capacity * 8);
  m.node_mask = take(node_capacity * 4);
  m.node_first = take(node_capacity * 4);
  m.bytes = at;
  return m;
}

static double ctw_lgam(double x) {
  int sign;
  return ::lgamma_r(x, &sign);   // csrc/dib_ctw.cpp lgam: the same libm, the same bits
}

struct CtwTables {
  std::vector<double> beta, ab;   // lgamma(k + beta), lgamma(k + A beta) for k < DIB_CTW_TABLE
  DibCtwParams p;
};

// the constants and tables of one alphabet, computed once per process
static const CtwTables& ctw_tables(int A) {
  static std::mutex mu;
  static std::map<int, CtwTables> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(A);
  if (it != cache.end()) return it->second;
  CtwTables& t = cache[A];
  DibCtwParams& p = t.p;
  p.A = A;
  p.beta = 1. / A;
  p.ab = A * p.beta;
  p.lg_ab = ctw_lgam(p.ab);
  p.lg_b = ctw_lgam(p.beta);
  p.ln2 = std::log(2);
  t.beta.resize(DIB_CTW_TABLE);
  t.ab.resize(DIB_CTW_TABLE);
  for (int k = 0; k < DIB_CTW_TABLE; ++k) {
    t.beta[(size_t)k] = ctw_lgam(k + p.beta);
    t.ab[(size_t)k] = ctw_lgam((double)k + p.ab);
  }
  // a node with one member: the terms of the symbols it does not hold are lgamma(beta) - lgamma(beta) = 0
  double local = t.ab[1] - p.lg_ab;
  local -= t.beta[1] - p.lg_b;
  p.leaf = local / p.ln2;
  return t;
}

extern "C" {

int dib_ctw_device_supported(int alphabet_size, int64_t total_window_symbols, int n_windows) {
  return ctw_envelope(alphabet_size, total_window_symbols, n_windows) == DIB_OK ? 1 : 0;
}

int64_t dib_ctw_device_workspace_bytes(int64_t total_window_symbols, int n_windows, int alphabet_size, int64_t node_capacity) {
  if (ctw_envelope(alphabet_size, total_window_symbols, n_windows) != DIB_OK) return -1;
  if (node_capacity < std::max(n_windows, 1) || node_capacity > DIB_CTW_DEVICE_MAX_SYMBOLS) return -1;
  return ctw_workspace(total_window_symbols, n_windows, alphabet_size, node_capacity).bytes;
}

int dib_ctw_device_estimate(const uint8_t* symbols, int64_t n_symbols, const int64_t* starts, const int64_t* lengths, int n_windows,
                            int alphabet_size, int64_t node_capacity, double* code_bits, double* rates, int64_t* nodes,
                            int32_t* status, void* ws, int64_t ws_bytes, dib_ctw_device_info* info, dib_stream_t stream) {
  if (n_windows < 0 || n_symbols < 0 || (n_windows > 0 && (!starts || !lengths || !code_bits || !rates || !nodes || !status || !ws)))
    return DIB_E_ARG;
  int64_t E = 0;
  for (int w = 0; w < n_windows; ++w) {
    if (lengths[w] < 0 || starts[w] < 0 || starts[w] > n_symbols || lengths[w] > n_symbols - starts[w]) return DIB_E_ARG;
    E += lengths[w];
    if (E > DIB_CTW_DEVICE_MAX_SYMBOLS) return DIB_E_UNSUPPORTED;
  }
  if (int rc = ctw_envelope(alphabet_size, E, n_windows)) return rc;
  if (E > 0 && !symbols) return DIB_E_ARG;
  if (node_capacity < std::max(n_windows, 1) || node_capacity > DIB_CTW_DEVICE_MAX_SYMBOLS) return DIB_E_ARG;
  if (info) *info = dib_ctw_device_info{};
  if (n_windows == 0) return DIB_OK;
  const int W = n_windows, A = alphabet_size;
  const CtwWorkspace m = ctw_workspace(E, W, A, node_capacity);
  if (ws_bytes < m.bytes) return DIB_E_WORKSPACE;
  const CtwTables& tab = ctw_tables(A);
  DibCtwParams p = tab.p;
  p.W = W;

  hipStream_t st = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  auto at = [&](int64_t off) { return static_cast<void*>(base + off); };
  std::vector<long long> h_start((size_t)W);
  std::vector<int> h_off((size_t)W + 1), h_len((size_t)W);
  for (int w = 0; w < W; ++w) {
    h_start[(size_t)w] = starts[w];
    h_len[(size_t)w] = (int)lengths[w];
    h_off[(size_t)w + 1] = h_off[(size_t)w] + (int)lengths[w];
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(at(m.table_beta), tab.beta.data(), DIB_CTW_TABLE * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(at(m.table_ab), tab.ab.data(), DIB_CTW_TABLE * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(at(m.win_start), h_start.data(), (size_t)W * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(at(m.win_off), h_off.data(), ((size_t)W + 1) * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(at(m.win_len), h_len.data(), (size_t)W * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;

  const double* d_tab_beta = static_cast<const double*>(at(m.table_beta));
  const double* d_tab_ab = static_cast<const double*>(at(m.table_ab));
  const long long* d_start = static_cast<const long long*>(at(m.win_start));
  int* d_status = static_cast<int*>(at(m.status));
  DibCtwLevelRec* d_rec = static_cast<DibCtwLevelRec*>(at(m.rec));
  int* d_hist_sym = static_cast<int*>(at(m.hist_sym));
  int* d_hist_ctx = static_cast<int*>(at(m.hist_ctx));
  int2* d_key_info = static_cast<int2*>(at(m.key_info));
  int2* d_block_sums = static_cast<int2*>(at(m.block_sums));
  double* d_L = static_cast<double*>(at(m.node_L));
  long long* d_count = static_cast<long long*>(at(m.node_count));
  unsigned* d_mask = static_cast<unsigned*>(at(m.node_mask));
  int* d_first = static_cast<int*>(at(m.node_first));
  const int level_cap = (int)ctw_level_nodes(E, W, node_capacity);
  auto blocks = [](int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
  const dim3 threads(DIB_CTW_THREADS);

  DIB_LAUNCH(dib_ctw_init_kernel, blocks(std::max<int64_t>(E, W), DIB_CTW_THREADS), threads, 0, st,
             static_cast<const int*>(at(m.win_off)), W, (int)E, static_cast<int*>(at(m.el_t[0])), static_cast<int*>(at(m.el_node[0])),
             static_cast<int*>(at(m.node_win[0])), d_status);

  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::pair<int64_t, int>> levels;   // (first node id, nodes) of every level built
  int64_t node_base = 0, element_steps = 0;
  int nb = W, M = (int)E, cur = 0;
  for (int d = 0; d <= DIB_CTW_LAST_LEVEL; ++d) {
    const int last = d == DIB_CTW_LAST_LEVEL ? 1 : 0;
    const int64_t next_base = node_base + nb;
    const int* el_t = static_cast<const int*>(at(m.el_t[cur]));
    const int* el_node = static_cast<const int*>(at(m.el_node[cur]));
    const int* node_win = static_cast<const int*>(at(m.node_win[cur]));
    if ((e = hipMemsetAsync(d_hist_sym, 0, (size_t)nb * A * 4, st)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(d_hist_ctx, 0, (size_t)nb * A * 4, st)) != hipSuccess) return (int)e;
    if (M > 0)
      DIB_LAUNCH(dib_ctw_count_kernel, blocks(M, DIB_CTW_TILE), threads, 0, st, symbols, d_start, el_t, el_node, node_win, M, d, A,
                 last, d_hist_sym, d_hist_ctx, d_status);
    const dim3 node_blocks = blocks(nb, DIB_CTW_THREADS);
    DIB_LAUNCH(dib_ctw_scan_reduce_kernel, node_blocks, threads, 0, st, d_hist_ctx, nb, A, d_block_sums);
    DIB_LAUNCH(dib_ctw_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, d_block_sums, (int)node_blocks.x, (long long)next_base,
               (long long)node_capacity, level_cap, d_rec + d);
    DIB_LAUNCH(dib_ctw_finalize_kernel, node_blocks, threads, 0, st, d_hist_sym, d_hist_ctx, d_block_sums, nb, p, d_tab_beta,
               d_tab_ab, d_rec + d, (long long)node_base, (long long)next_base, node_win, static_cast<int*>(at(m.node_win[cur ^ 1])),
               d_key_info, d_L, d_mask, d_first, d_status);
    if (M > 0 && !last)
      DIB_LAUNCH(dib_ctw_place_kernel, blocks(M, DIB_CTW_TILE), threads, 0, st, symbols, d_start, el_t, el_node, node_win, M, d, A,
                 d_rec + d, d_hist_ctx, d_key_info, static_cast<int*>(at(m.el_t[cur ^ 1])), static_cast<int*>(at(m.el_node[cur ^ 1])));
    DibCtwLevelRec rec{};
    if ((e = hipMemcpyAsync(&rec, d_rec + d, sizeof rec, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;   // the one synchronisation per level
    levels.emplace_back(node_base, nb);
    element_steps += M;
    if (rec.overflow || rec.next_elems == 0 || last) break;
    node_base = next_base;
    nb = rec.next_nodes;
    M = rec.next_elems;
    cur ^= 1;
  }
  const auto t1 = std::chrono::steady_clock::now();
  for (size_t l = levels.size(); l-- > 0;)
    DIB_LAUNCH(dib_ctw_mix_kernel, blocks(levels[l].second, DIB_CTW_THREADS), threads, 0, st, (long long)levels[l].first,
               levels[l].second, A, p.leaf, d_L, d_mask, d_first, d_count);
  DIB_LAUNCH(dib_ctw_output_kernel, blocks(W, DIB_CTW_THREADS), threads, 0, st, d_L, d_count, static_cast<const int*>(at(m.win_len)),
             d_status, W, code_bits, rates, reinterpret_cast<long long*>(nodes), status);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (info) {
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;   // a caller that asks for the phase times pays one more wait
    const auto t2 = std::chrono::steady_clock::now();
    info->levels = (int32_t)levels.size();
    info->element_steps = element_steps;
    info->big_nodes = levels.back().first + levels.back().second;
    info->level_seconds = std::chrono::duration<double>(t1 - t0).count();
    info->mix_seconds = std::chrono::duration<double>(t2 - t1).count();
  }
  return DIB_OK;
}

}  // extern "C"
