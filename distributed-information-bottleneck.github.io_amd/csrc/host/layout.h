// host/layout.h - dib_layout: the flat parameter layout, the GEMM descriptor tables and the workspace map (include/dib_hip.h).

namespace {

struct GemmCall {  // one grouped launch: slice [first, first+count) of the descriptor table
  int first = 0, count = 0;
  int max_m = 0, max_n = 0;  // max logical dims over the groups (-1 => batch)
};

// Off = {fixed element offset, offset per batch row} : activations are feature-major [F][B][width]
struct Off { int64_t fixed = 0, per_batch = 0; };
inline Off fixed_off(int64_t o) { Off r; r.fixed = o; return r; }
inline Off batch_off(int64_t o) { Off r; r.per_batch = o; return r; }

DibGemmGroup make_group(Off a, int lda, Off b, int ldb, Off c, int ldc, int64_t bias_off, Off aux, int ldaux, int M,
                        int N, int K) {
  DibGemmGroup g;
  std::memset(&g, 0, sizeof(g));
  g.a_off = a.fixed; g.a_boff = a.per_batch; g.b_off = b.fixed; g.b_boff = b.per_batch;
  g.c_off = c.fixed; g.c_boff = c.per_batch; g.aux_off = aux.fixed; g.aux_boff = aux.per_batch;
  g.bias_off = bias_off;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldaux = ldaux;
  return g;
}

}  // namespace

struct dib_layout {
  int F = 0, n_enc = 0, E = 0, n_int = 0, out_dim = 0, use_pe = 0, n_freq = 0, act = 0, out_act = 0;
  std::vector<int> dims, enc_units, int_units;
  int sum_d = 0, pw = 0, n_blocks = 1;    // pw = total encoder-input width, n_blocks = 1 + #sinusoids
  std::vector<int> in_dim, in_off, x_off; // per feature: encoder input width / its first column in P / in x
  std::vector<int> enc_width;             // [n_enc+1] per-feature output width of each encoder layer
  std::vector<int> int_width;             // [n_int+1]
  int64_t n_params = 0;
  long long max_wgrad_tiles64 = 0;        // most 64 x 64 output tiles any one weight-gradient launch has (all groups)
  std::vector<std::vector<int64_t>> enc_w_off, enc_b_off;  // [layer][feature]
  std::vector<int64_t> int_w_off, int_b_off;
  // descriptor table
  std::vector<DibGemmGroup> table;
  std::vector<int4> colmap;
  std::vector<GemmCall> enc_fwd, enc_dgrad, enc_wgrad, int_fwd, int_dgrad, int_wgrad;
  const DibGemmGroup* dev_groups = nullptr;
  const int4* dev_colmap = nullptr;
  // fused encoder-bank kernels (dib_fused.h): -1 = not applicable, else index into the instantiation table
  int fused_id = -1;
  std::vector<long long> fused_offs;   // [3][F] kernel offsets then [3][F] bias offsets
  std::vector<int4> featmap;           // [F] {d_f, in_dim_f, x column, 0}
  const long long* dev_fused_offs = nullptr;
  const int4* dev_featmap = nullptr;
  // the layer-2 weight gradient that recomputes h1 (dib_wgrad_recompute.h): its per-feature side table (empty: not applicable) and
  // what the last training forward into each workspace decided - the backward launches by this record, never by the tuning table
  struct H1Plan { bool recompute = false; int ch = 2, nsplit = 0, rows_per_split = 0; };
  std::vector<DibWgradH1Side> h1_side;
  const DibWgradH1Side* dev_h1_side = nullptr;
  mutable std::map<const void*, H1Plan> h1_plan;   // by workspace (guarded by wg_mu)
  // whether the last forward into each workspace was a training forward (it wrote the stashes a backward and
  // dib_encoder_bank_input_grad read); no entry = no forward since dib_workspace_init (guarded by wg_mu)
  mutable std::map<const void*, bool> fwd_training;
  const unsigned* step_dev = nullptr;  // optional device-resident noise step (dib_layout_set_step_counter)
  // small-batch row-tile kernels (dib_small.h): which halves of the network they cover for this architecture
  bool sb_enc = false, sb_int = false;
  int sb_int_lds = 0;                  // dynamic LDS bytes of dib_small_integration_kernel
  // merged weight-gradient table (one per batch size, kept alive for the asynchronous upload of dib_workspace_init):
  // groups [0, n_enc F): encoder layers 1 .. n_enc (feature-major), then the integration layers 0 .. n_int
  int wg_groups() const { return n_enc * F + n_int + 1; }
  mutable std::map<int, std::vector<DibGemmGroup>> wg_tables;
  mutable std::mutex wg_mu;            // two threads may initialise workspaces of one layout (include/dib_hip.h "Threads")
  // Most batch slabs any weight-gradient launch of this layout has written per (batch size, parameter block) - see
  // retire_stale_slabs.  Conservative across the layout's workspaces (guarded by wg_mu).
  mutable std::map<std::pair<int, long long>, int> slab_hwm;

  // ---- workspace map (float offsets), all per-row widths scale with the batch ----
  struct WsMap {
    int64_t P, enc_out, U, pred, g_pred, g_u, dout;
    std::vector<int64_t> enc_h, int_h, g_enc_h, g_int_h;
    int64_t step_out, kl_partial, loss_partial, wgrad_partial, dw1_partial, h2mask, h1mask, skinny_partial, sync, wg_table, total;
    int64_t cl_sync; std::vector<int64_t> cl_x;   // cluster mode of the row-tile integration kernel (dib_small.h)
    int skinny_chunks, skinny_rows;
    int kl_blocks, loss_blocks, nsplit, rows_per_split;
  };
  WsMap map(int B) const {
    WsMap m;
    int64_t o = 0;
    auto take = [&](int64_t nfloats) { int64_t r = o; o = align_up(o + nfloats); return r; };
    m.P = take((int64_t)B * pw);
    for (int l = 0; l < n_enc; ++l) m.enc_h.push_back(take((int64_t)B * F * enc_units[l]));
    m.enc_out = take((int64_t)B * F * 2 * E);
    m.U = take((int64_t)B * F * E);
    for (int l = 0; l < n_int; ++l) m.int_h.push_back(take((int64_t)B * int_units[l]));
    m.pred = take((int64_t)B * out_dim);
    m.g_pred = take((int64_t)B * out_dim);
    for (int l = 0; l < n_int; ++l) m.g_int_h.push_back(take((int64_t)B * int_units[l]));
    m.g_u = take((int64_t)B * F * E);
    m.dout = take((int64_t)B * F * 2 * E);
    for (int l = 0; l < n_enc; ++l) m.g_enc_h.push_back(take((int64_t)B * F * enc_units[l]));
    m.step_out = take(F + 3);
    const int E4 = (E + 3) / 4;
    const int rpb = std::max(1, 256 / E4);
    m.kl_blocks = cdiv(B, rpb);
    m.kl_partial = take((int64_t)std::max(m.kl_blocks, 8 * 256) * F);  // fused fwd: one row per wave of the persistent grid
    m.loss_blocks = cdiv(B, 256);
    m.loss_partial = take((int64_t)std::max(m.loss_blocks, 512) * 2);  // also the fused output head's per-workgroup partials (<= 512)
    // split-batch wgrad: rows_per_split multiple of 32, <= 32 splits, >= kSplitRows rows per split ...
    int ns = std::min(std::min(kMaxSplits, wgrad_max_splits()), std::max(1, B / kSplitRows));
    // ... unless the layout is so narrow that even its largest weight gradient stays under one workgroup per CU with that
    // many splits (BASELINE config 2, the pendulum layout [2,1,2,1]: 16 tiles x 4 splits of 512 rows at B = 2048 - five
    // launches of 18-24 us, each a workgroup walking 16 dependent K-tiles, 100 of the 510 us step,
    // profiles/r04i_config2_loop_kernel_stats_b2048.csv): then slabs of >= 128 rows
    if (B >= 256 && max_wgrad_tiles64 * ns < 256) ns = std::min(std::min(kMaxSplits, wgrad_max_splits()), std::max(ns, B / 128));
    int rps = cdiv(cdiv(B, ns), 32) * 32;
    ns = cdiv(B, rps);
    m.nsplit = ns;
    m.rows_per_split = rps;
    m.wgrad_partial = take(ns > 1 ? (int64_t)ns * align_up(n_params, 4) : 0);
    // fused backward: per-wave partials of d(W1|b1), [<= ceil(256/F) workgroups x 8 waves][F][16][H1]
    // (small-batch path: one partial per 16-row tile, [<= kSmallMaxEncWgs (tile, feature) pairs][16][H1])
    m.dw1_partial = take(std::max<int64_t>(fused_id >= 0 && n_enc == 2 ? (int64_t)cdiv(256, F) * 8 * F * 16 * enc_units[0] : 0,
                                           sb_enc && B <= kSmallMaxBatch && (int64_t)cdiv(B, DIB_SMALL_ROWS) * F <= kSmallMaxEncWgs
                                               ? (int64_t)cdiv(B, DIB_SMALL_ROWS) * F * 16 * enc_units[0] : 0));
    // [F][B][2] x 64-bit act' masks (fused fwd -> fused bwd), one bit per hidden unit
    m.h2mask = take(fused_id >= 0 ? (int64_t)F * B * 4 : 0);
    m.h1mask = take(fused_id >= 0 ? (int64_t)F * B * 4 : 0);
    // skinny output layer wgrad: row chunks of >= 64 rows (>= 16 up to B = 2048), <= 512 chunks
    // (16-row chunks for small batches: with 64 the fused output head of the reference's default B = 128 step ran on 2
    // workgroups, each wave walking 16 rows one after the other - 21 us, profiles/r04l_default_batch_kernel_stats.csv)
    m.skinny_rows = std::max(B <= 2048 ? 16 : 64, cdiv(B, 512));
    m.skinny_chunks = cdiv(B, m.skinny_rows);
    {
      const int win = n_int == 0 ? F * E : int_units[n_int - 1];
      m.skinny_partial = take(out_dim <= 8 ? (int64_t)m.skinny_chunks * ((int64_t)win * out_dim + out_dim) : 0);
    }
    m.sync = take(DIB_TAIL_SYNC_WORDS);   // arrival counters of dib_step_tail (zeroed by dib_workspace_init, self-cleaning)
    // descriptors of ALL weight gradients of a step with absolute workspace offsets for THIS batch size (written by
    // dib_workspace_init): one grouped launch instead of one per layer (merged_wgrad)
    m.wg_table = take((int64_t)wg_groups() * (int64_t)(sizeof(DibGemmGroup) / sizeof(float)));
    // cluster mode of the row-tile integration kernel: arrival counters per row tile (zeroed by dib_workspace_init, self-cleaning)
    // and the hidden activations' exchange buffers of launches that write no stashes
    const bool cl_ok = sb_int && B <= kSmallMaxBatch;
    m.cl_sync = take(cl_ok ? 2ll * cdiv(B, DIB_SMALL_ROWS) * DIB_SMALL_CL_SYNC_WORDS : 0);   // x 2: a companion network's (paired grid)
    for (int l = 0; l < n_int; ++l) m.cl_x.push_back(take(cl_ok ? (int64_t)B * int_units[l] : 0));
    m.total = o;
    return m;
  }
};

// dynamic LDS bytes of dib_small_encoder_fwd_kernel (bwd = false) / dib_small_encoder_bwd_kernel (bwd = true): their [16][pitch]
// tiles - input [16][20], h1, h2, d(mu|logvar) (the backward also dh2, dh1) - and the slice primitives' wide exchange buffer.
// dib_layout_create admits a layout to the row-tile encoders only where both fit kSmallMaxLds.
static size_t small_encoder_lds(int H1, int H2, int E, bool bwd) {
  const int k = bwd ? 2 : 1;
  return (size_t)DIB_SMALL_ROWS * (20 + k * dib_small_pitch(H1) + k * dib_small_pitch(H2) + dib_small_pitch(2 * E)) * sizeof(float) +
         (size_t)DIB_SMALL_XCH_FLOATS_WIDE * sizeof(float);
}
// dynamic LDS bytes of the integration kernels, from the LDS map they carve from (dib_small.h "LDS maps"): hidden widths
// width[n_hidden]; wide_xch: the cluster kernels; head: with the 1-unit head's scratch
static size_t small_int_lds(int K0, int n_hidden, const int* width, int out_dim, bool wide_xch, bool head) {
  return (size_t)dib_small_int_lds<DibLdsFloats>(0, K0, n_hidden, width, out_dim, wide_xch, head).end * sizeof(float);
}
// A network the row-tile integration kernel can run: 1-3 hidden layers of widths % 16 == 0 (<= 1024: the head's lane-strided dot)
// and a piecewise-linear activation (dib_small.h dib_small_act).  small_int_lds against kSmallAdmitLds supplies the rest; the
// input and output widths and the tuning knobs are each caller's own.
static bool small_int_shape_ok(int n_hidden, const int* width, int act) {
  if (n_hidden < 1 || n_hidden > 3) return false;
  if (!(act >= 0 && act <= 2) && act != DIB_ACT_LEAKY_RELU_01) return false;
  for (int i = 0; i < n_hidden; ++i)
    if (width[i] < 16 || width[i] % 16 != 0 || width[i] > 1024) return false;
  return true;
}

// ---- all weight gradients of a step in ONE grouped launch (host/gemm.h merged_wgrad) ----------------------------------------
// Descriptors with absolute workspace offsets for this batch size (the activation buffers' offsets are not linear in the batch:
// every buffer is 256-byte aligned), A and B both relative to the workspace base, C / bias_out relative to the gradient target.
static const std::vector<DibGemmGroup>& wg_table_host(const dib_layout* l, const dib_layout::WsMap& m, int batch) {
  std::lock_guard<std::mutex> lk(l->wg_mu);   // std::map nodes are stable: the reference outlives the lock
  auto it = l->wg_tables.find(batch);
  if (it != l->wg_tables.end()) return it->second;
  std::vector<DibGemmGroup> t;
  const int64_t B = batch;
  for (int ly = 1; ly <= l->n_enc; ++ly) {
    const int win = l->enc_width[ly - 1], wout = l->enc_width[ly];
    for (int f = 0; f < l->F; ++f)
      t.push_back(make_group(fixed_off(m.enc_h[ly - 1] + (int64_t)f * win * B), win,
                             fixed_off((ly == l->n_enc ? m.dout : m.g_enc_h[ly]) + (int64_t)f * wout * B), wout,
                             fixed_off(l->enc_w_off[ly][f]), wout, l->enc_b_off[ly][f], Off(), 0, win, wout, -1));
  }
  for (int ly = 0; ly <= l->n_int; ++ly) {
    const int win = ly == 0 ? l->F * l->E : l->int_width[ly - 1], wout = l->int_width[ly];
    t.push_back(make_group(fixed_off(ly == 0 ? m.U : m.int_h[ly - 1]), win, fixed_off(ly == l->n_int ? m.g_pred : m.g_int_h[ly]), wout,
                           fixed_off(l->int_w_off[ly]), wout, l->int_b_off[ly], Off(), 0, win, wout, -1));
  }
  return l->wg_tables.emplace(batch, std::move(t)).first->second;
}

static inline float* wgrad_target(const dib_layout::WsMap& m, float* w, float* grads) {
  return m.nsplit > 1 ? w + m.wgrad_partial : grads;
}

// [beg, end) of a gradient bucket in the flat buffers.  The layout is layer-major (all features' kernels of encoder layer 0,
// their biases, layer 1, ..., then the integration network), every block boundary a multiple of 4 floats:
//   0 = encoder bank, 1 = integration network, 2 = encoder layers before the last ("front"), 3 = last encoder layer ("tail"),
//   -1 = everything
static void part_bounds(const dib_layout* l, int part, long long* beg, long long* end) {
  const long long split = l->int_w_off[0], tail = l->enc_w_off[l->n_enc][0], all = l->n_params;
  switch (part) {
    case 0: *beg = 0; *end = split; break;
    case 1: *beg = split; *end = all; break;
    case 2: *beg = 0; *end = tail; break;
    case 3: *beg = tail; *end = split; break;
    default: *beg = 0; *end = all; break;
  }
}

extern "C" {

int dib_layout_create(int F, const int* feature_dims, int n_enc, const int* enc_units, int E, int n_int,
                      const int* int_units, int out_dim, int use_pe, int n_freq, int act, int out_act,
                      dib_layout** out) {
  if (!out || F <= 0 || !feature_dims || n_enc < 0 || n_int < 0 || E <= 0 || out_dim <= 0) return DIB_E_ARG;
  if ((n_enc > 0 && !enc_units) || (n_int > 0 && !int_units)) return DIB_E_ARG;
  if (!act_ok(act) || !act_ok(out_act)) return DIB_E_UNSUPPORTED;
  if ((E + 3) / 4 > 256) return DIB_E_UNSUPPORTED;
  dib_layout* l = new (std::nothrow) dib_layout();
  if (!l) return DIB_E_ARG;
  l->F = F; l->n_enc = n_enc; l->E = E; l->n_int = n_int; l->out_dim = out_dim;
  l->use_pe = use_pe ? 1 : 0; l->n_freq = n_freq; l->act = act; l->out_act = out_act;
  l->dims.assign(feature_dims, feature_dims + F);
  l->enc_units.assign(enc_units, enc_units + n_enc);
  l->int_units.assign(int_units, int_units + n_int);
  // reference models.py:70: frequencies = 2**arange(1, n_freq) -> n_freq-1 sinusoids
  l->n_blocks = (l->use_pe && n_freq > 1) ? n_freq : 1;
  for (int f = 0; f < F; ++f) {
    if (l->dims[f] <= 0) { delete l; return DIB_E_ARG; }
    l->x_off.push_back(l->sum_d);
    l->in_off.push_back(l->pw);
    l->in_dim.push_back(l->dims[f] * l->n_blocks);
    l->sum_d += l->dims[f];
    l->pw += l->dims[f] * l->n_blocks;
    for (int c = 0; c < l->dims[f]; ++c) l->colmap.push_back(make_int4(f, c, l->dims[f], l->in_off[f]));
  }
  for (int i = 0; i < n_enc; ++i) { if (enc_units[i] <= 0) { delete l; return DIB_E_ARG; } l->enc_width.push_back(enc_units[i]); }
  l->enc_width.push_back(2 * E);
  for (int i = 0; i < n_int; ++i) { if (int_units[i] <= 0) { delete l; return DIB_E_ARG; } l->int_width.push_back(int_units[i]); }
  l->int_width.push_back(out_dim);

  // ---- flat parameter layout: per encoder layer {all kernels (feature-major), all biases}, then integration ----
  int64_t o = 0;
  const int LE = n_enc + 1, LI = n_int + 1;
  l->enc_w_off.assign(LE, std::vector<int64_t>(F));
  l->enc_b_off.assign(LE, std::vector<int64_t>(F));
  for (int ly = 0; ly < LE; ++ly) {
    const int wout = l->enc_width[ly];
    for (int f = 0; f < F; ++f) {
      const int win = ly == 0 ? l->in_dim[f] : l->enc_width[ly - 1];
      o = align_up(o, 4);
      l->enc_w_off[ly][f] = o;
      o += (int64_t)win * wout;
    }
    o = align_up(o, 4);
    for (int f = 0; f < F; ++f) { l->enc_b_off[ly][f] = o; o += wout; }
  }
  for (int ly = 0; ly < LI; ++ly) {
    const int win = ly == 0 ? F * E : l->int_width[ly - 1];
    const int wout = l->int_width[ly];
    o = align_up(o, 4);
    l->int_w_off.push_back(o);
    o += (int64_t)win * wout;
    o = align_up(o, 4);
    l->int_b_off.push_back(o);
    o += wout;
  }
  l->n_params = o;

  // ---- GEMM group descriptors.  Encoder-bank activations are FEATURE-MAJOR: [F][B][width], i.e. feature f's
  // operand is the dense matrix at element offset (f*width)*B (ragged first layer: in_off[f]*B).  U / g_u (the
  // integration network's operand, reference models.py:122 tf.concat) stay sample-major [B, F*E]. ----
  auto& T = l->table;
  for (int ly = 0; ly < LE; ++ly) {
    const int wout = l->enc_width[ly];
    GemmCall fw, dg, wg;
    fw.first = (int)T.size();
    for (int f = 0; f < F; ++f) {
      const int win = ly == 0 ? l->in_dim[f] : l->enc_width[ly - 1];
      const Off a = batch_off(ly == 0 ? (int64_t)l->in_off[f] : (int64_t)f * win);
      T.push_back(make_group(a, win, fixed_off(l->enc_w_off[ly][f]), wout, batch_off((int64_t)f * wout), wout,
                             l->enc_b_off[ly][f], Off(), 0, -1, wout, win));
    }
    fw.count = F; fw.max_m = -1; fw.max_n = wout;
    l->enc_fwd.push_back(fw);
    // dgrad (ly >= 1): g_in[B, win] = (g_out[B, wout] @ W[win, wout]^T) * act'(h_in)
    dg.first = (int)T.size();
    if (ly >= 1) {
      const int win = l->enc_width[ly - 1];
      for (int f = 0; f < F; ++f)
        T.push_back(make_group(batch_off((int64_t)f * wout), wout, fixed_off(l->enc_w_off[ly][f]), wout,
                               batch_off((int64_t)f * win), win, -1, batch_off((int64_t)f * win), win, -1, win, wout));
      dg.count = F; dg.max_m = -1; dg.max_n = win;
    }
    l->enc_dgrad.push_back(dg);
    // wgrad: dW[win, wout] = h_in[B, win]^T @ g_out[B, wout] ; db = colsum(g_out)
    wg.first = (int)T.size();
    int max_in = 0;
    for (int f = 0; f < F; ++f) {
      const int win = ly == 0 ? l->in_dim[f] : l->enc_width[ly - 1];
      const Off a = batch_off(ly == 0 ? (int64_t)l->in_off[f] : (int64_t)f * win);
      T.push_back(make_group(a, win, batch_off((int64_t)f * wout), wout, fixed_off(l->enc_w_off[ly][f]), wout,
                             l->enc_b_off[ly][f], Off(), 0, win, wout, -1));
      max_in = std::max(max_in, win);
    }
    wg.count = F; wg.max_m = max_in; wg.max_n = wout;
    l->max_wgrad_tiles64 = std::max(l->max_wgrad_tiles64, (long long)cdiv(max_in, 64) * cdiv(wout, 64) * F);
    l->enc_wgrad.push_back(wg);
  }
  for (int ly = 0; ly < LI; ++ly) {
    const int win = ly == 0 ? F * E : l->int_width[ly - 1];
    const int wout = l->int_width[ly];
    GemmCall fw, dg, wg;
    fw.first = (int)T.size();
    T.push_back(make_group(Off(), win, fixed_off(l->int_w_off[ly]), wout, Off(), wout, l->int_b_off[ly], Off(), 0, -1,
                           wout, win));
    fw.count = 1; fw.max_m = -1; fw.max_n = wout;
    l->int_fwd.push_back(fw);
    dg.first = (int)T.size();
    T.push_back(make_group(Off(), wout, fixed_off(l->int_w_off[ly]), wout, Off(), win, -1, Off(), win, -1, win, wout));
    dg.count = 1; dg.max_m = -1; dg.max_n = win;
    l->int_dgrad.push_back(dg);
    wg.first = (int)T.size();
    T.push_back(make_group(Off(), win, Off(), wout, fixed_off(l->int_w_off[ly]), wout, l->int_b_off[ly], Off(), 0, win,
                           wout, -1));
    wg.count = 1; wg.max_m = win; wg.max_n = wout;
    l->max_wgrad_tiles64 = std::max(l->max_wgrad_tiles64, (long long)cdiv(win, 64) * cdiv(wout, 64));
    l->int_wgrad.push_back(wg);
  }
  // fused encoder-bank path: two hidden layers, instantiated (H1,H2,E), encoder inputs <= 16 wide
  {
    static const int kFused[][3] = {{128, 128, 32}, {32, 32, 32}, {32, 32, 8}, {64, 64, 16}};
    bool in_ok = true;
    for (int f = 0; f < F; ++f) in_ok = in_ok && l->in_dim[f] <= 16;
    if (knobs().fused_encoder && n_enc == 2 && in_ok && act >= 0 && act <= 2)
      for (int i = 0; i < 4; ++i)
        if (kFused[i][0] == enc_units[0] && kFused[i][1] == enc_units[1] && kFused[i][2] == E) l->fused_id = i;
    for (int ly = 0; ly < LE && ly < 3; ++ly)
      for (int f = 0; f < F; ++f) l->fused_offs.push_back(l->enc_w_off[ly][f]);
    for (int ly = LE; ly < 3; ++ly)
      for (int f = 0; f < F; ++f) l->fused_offs.push_back(0);
    for (int ly = 0; ly < LE && ly < 3; ++ly)
      for (int f = 0; f < F; ++f) l->fused_offs.push_back(l->enc_b_off[ly][f]);
    for (int ly = LE; ly < 3; ++ly)
      for (int f = 0; f < F; ++f) l->fused_offs.push_back(0);
    for (int f = 0; f < F; ++f) l->featmap.push_back(make_int4(l->dims[f], l->in_dim[f], l->x_off[f], l->in_off[f]));
    // h1 = act(P W1 + b1) recomputed by the layer-2 weight gradient: the 128-wide fused configuration with inputs <= 8 wide (one
    // k-block of the forward's layer 1)
    bool in8 = true;
    for (int f = 0; f < F; ++f) in8 = in8 && l->in_dim[f] <= 8;
    if (l->fused_id == 0 && in8)
      for (int f = 0; f < F; ++f) {
        DibWgradH1Side sd;
        std::memset(&sd, 0, sizeof(sd));
        sd.p_boff = l->in_off[f]; sd.w1_off = l->enc_w_off[0][f]; sd.b1_off = l->enc_b_off[0][f];
        sd.in_dim = l->in_dim[f]; sd.act = act;
        l->h1_side.push_back(sd);
      }
  }
  // small-batch row-tile kernels (dib_small.h): two-hidden-layer encoders of widths % 16 == 0 (<= 1024, E <= 512) with inputs
  // <= 15 wide (the 16th row of the d(W1|b1) tile carries the bias gradient) whose forward AND backward tiles, wide exchange buffer
  // included (small_encoder_lds), fit one workgroup's 160 KB of LDS - [448, 448] at E = 32 does (162 304 B for the backward),
  // [512, 512] or [1024, 16] do not; linear / relu / leaky_relu.  Integration networks of 1-3 hidden layers of widths % 16 == 0
  // (<= 1024 for the head's lane-strided dot) whose 16-row activation tiles fit 150 KB (cluster mode adds 20 KB of exchange buffer)
  {
    bool in_ok = true;
    for (int f = 0; f < F; ++f) in_ok = in_ok && l->in_dim[f] <= 15;
    const bool pl_act = act >= 0 && act <= 2 && out_act >= 0 && out_act <= 2;   // piecewise-linear activations (dib_small.h)
    l->sb_enc = pl_act && n_enc == 2 && in_ok && enc_units[0] % 16 == 0 && enc_units[1] % 16 == 0 && (2 * E) % 16 == 0 &&
                enc_units[0] <= 1024 && enc_units[1] <= 1024 && E <= 512 &&
                small_encoder_lds(enc_units[0], enc_units[1], E, false) <= kSmallMaxLds &&
                small_encoder_lds(enc_units[0], enc_units[1], E, true) <= kSmallMaxLds;
    // the layout's own: pl_act (the output activation too), an input of whole 16-unit tiles, and the launch size WITH the head's
    // scratch whatever the output layer (one size serves the head and the general output layer)
    if (pl_act && (F * E) % 16 == 0 && small_int_shape_ok(n_int, int_units, act)) {
      l->sb_int_lds = (int)small_int_lds(F * E, n_int, int_units, out_dim, false, true);
      l->sb_int = (size_t)l->sb_int_lds <= kSmallAdmitLds;
    }
  }
  *out = l;
  return DIB_OK;
}

void dib_layout_destroy(dib_layout* l) {
  if (!l) return;
  delete l;
}

int64_t dib_layout_param_count(const dib_layout* l) { return l ? l->n_params : DIB_E_ARG; }

int dib_layout_param_block(const dib_layout* l, int net, int layer, int feature, int what, int64_t* offset,
                           int* rows, int* cols) {
  if (!l || !offset || !rows || !cols) return DIB_E_ARG;
  if (net == 0) {
    if (layer < 0 || layer > l->n_enc || feature < 0 || feature >= l->F) return DIB_E_ARG;
    const int win = layer == 0 ? l->in_dim[feature] : l->enc_width[layer - 1];
    const int wout = l->enc_width[layer];
    if (what == 0) { *offset = l->enc_w_off[layer][feature]; *rows = win; *cols = wout; }
    else { *offset = l->enc_b_off[layer][feature]; *rows = 1; *cols = wout; }
    return DIB_OK;
  }
  if (net == 1) {
    if (layer < 0 || layer > l->n_int) return DIB_E_ARG;
    const int win = layer == 0 ? l->F * l->E : l->int_width[layer - 1];
    const int wout = l->int_width[layer];
    if (what == 0) { *offset = l->int_w_off[layer]; *rows = win; *cols = wout; }
    else { *offset = l->int_b_off[layer]; *rows = 1; *cols = wout; }
    return DIB_OK;
  }
  return DIB_E_ARG;
}

int64_t dib_layout_table_bytes(const dib_layout* l) {
  if (!l) return DIB_E_ARG;
  return align_up((int64_t)l->table.size() * sizeof(DibGemmGroup), 256) +
         align_up((int64_t)l->colmap.size() * sizeof(int4), 256) +
         align_up((int64_t)l->fused_offs.size() * sizeof(long long), 256) +
         align_up((int64_t)l->featmap.size() * sizeof(int4), 256) +
         align_up((int64_t)l->h1_side.size() * sizeof(DibWgradH1Side), 256);
}

int dib_layout_upload_tables(dib_layout* l, void* dev_tables, dib_stream_t stream) {
  if (!l || !dev_tables) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t gbytes = (int64_t)l->table.size() * sizeof(DibGemmGroup);
  char* base = (char*)dev_tables;
  hipError_t e = hipMemcpyAsync(base, l->table.data(), gbytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  char* cm = base + align_up(gbytes, 256);
  e = hipMemcpyAsync(cm, l->colmap.data(), l->colmap.size() * sizeof(int4), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  char* fo = cm + align_up((int64_t)l->colmap.size() * sizeof(int4), 256);
  e = hipMemcpyAsync(fo, l->fused_offs.data(), l->fused_offs.size() * sizeof(long long), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  char* fmp = fo + align_up((int64_t)l->fused_offs.size() * sizeof(long long), 256);
  e = hipMemcpyAsync(fmp, l->featmap.data(), l->featmap.size() * sizeof(int4), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  l->dev_groups = (const DibGemmGroup*)base;
  l->dev_colmap = (const int4*)cm;
  l->dev_fused_offs = (const long long*)fo;
  l->dev_featmap = (const int4*)fmp;
  if (!l->h1_side.empty()) {
    char* hs = fmp + align_up((int64_t)l->featmap.size() * sizeof(int4), 256);
    e = hipMemcpyAsync(hs, l->h1_side.data(), l->h1_side.size() * sizeof(DibWgradH1Side), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    l->dev_h1_side = (const DibWgradH1Side*)hs;
  }
  return DIB_OK;
}

int dib_layout_set_step_counter(dib_layout* l, const uint32_t* step_dev) {
  if (!l) return DIB_E_ARG;
  l->step_dev = (const unsigned*)step_dev;
  return DIB_OK;
}

int64_t dib_workspace_bytes(const dib_layout* l, int batch) {
  if (!l || batch <= 0) return DIB_E_ARG;
  return l->map(batch).total * (int64_t)sizeof(float);
}

int dib_workspace_init(const dib_layout* l, int batch, void* ws, dib_stream_t stream) {
  if (!l || !ws || batch <= 0) return DIB_E_ARG;
  const auto m = l->map(batch);
  { std::lock_guard<std::mutex> lk(l->wg_mu); l->h1_plan.erase(ws); l->fwd_training.erase(ws); }   // a fresh workspace holds no forward's decision
  // the arrival counters of dib_step_tail (self-cleaning afterwards)
  hipError_t e0 = hipMemsetAsync((float*)ws + m.sync, 0, (size_t)DIB_TAIL_SYNC_WORDS * sizeof(unsigned), (hipStream_t)stream);
  if (e0 != hipSuccess) return (int)e0;
  if (l->sb_int && batch <= kSmallMaxBatch) {   // ... and of the integration kernel's cluster mode
    e0 = hipMemsetAsync((float*)ws + m.cl_sync, 0, 2 * (size_t)cdiv(batch, DIB_SMALL_ROWS) * DIB_SMALL_CL_SYNC_WORDS * sizeof(unsigned),
                        (hipStream_t)stream);
    if (e0 != hipSuccess) return (int)e0;
  }
  {  // the merged weight-gradient table of this batch size (the host copy lives in the layout: the copy may be asynchronous)
    const auto& t = wg_table_host(l, m, batch);
    e0 = hipMemcpyAsync((float*)ws + m.wg_table, t.data(), t.size() * sizeof(DibGemmGroup), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e0 != hipSuccess) return (int)e0;
  }
  // the per-step scalars: a caller that accumulates only the KL terms (custom loss) must not pick up stale loss sums
  e0 = hipMemsetAsync((float*)ws + m.step_out, 0, (size_t)(l->F + 3) * sizeof(float), (hipStream_t)stream);
  if (e0 != hipSuccess) return (int)e0;
  if (m.nsplit <= 1) return DIB_OK;
  // the split-batch weight-gradient slabs: dib_grads_finalize sums all nsplit slabs of every block, including the slabs
  // a launch never writes (halved splits of narrow layers, slabs >= 1 of the skinny output layer, the layer-1 block
  // under the fused backward, alignment gaps) - those must read as zero.  Nothing ever writes a non-zero there.
  return (int)hipMemsetAsync((float*)ws + m.wgrad_partial, 0,
                             (size_t)m.nsplit * (size_t)align_up(l->n_params, 4) * sizeof(float), (hipStream_t)stream);
}

int64_t dib_workspace_offset(const dib_layout* l, int batch, int which) {
  if (!l || batch <= 0) return DIB_E_ARG;
  const auto m = l->map(batch);
  int64_t o = -1;
  switch (which) {
    case DIB_WS_U: o = m.U; break;
    case DIB_WS_PRED: o = m.pred; break;
    case DIB_WS_ENC_OUT: o = m.enc_out; break;
    case DIB_WS_G_U: o = m.g_u; break;
    case DIB_WS_STEP_OUT: o = m.step_out; break;
    case DIB_WS_G_PRED: o = m.g_pred; break;
    default:
      if (which >= DIB_WS_ENC_H0 && which < DIB_WS_ENC_H0 + l->n_enc) o = m.enc_h[which - DIB_WS_ENC_H0];
      else if (which >= DIB_WS_INT_H0 && which < DIB_WS_INT_H0 + l->n_int) o = m.int_h[which - DIB_WS_INT_H0];
      else return DIB_E_ARG;
  }
  return o * (int64_t)sizeof(float);
}

int dib_workspace_h1_stashed(const dib_layout* l, const void* ws) {
  if (!l || !ws) return DIB_E_ARG;
  std::lock_guard<std::mutex> lk(l->wg_mu);
  auto it = l->h1_plan.find(ws);
  return it == l->h1_plan.end() || !it->second.recompute ? 1 : 0;
}

int dib_layout_wgrad_splits(const dib_layout* l, int batch) {
  if (!l || batch <= 0) return DIB_E_ARG;
  return l->map(batch).nsplit;
}

int dib_layout_part_range(const dib_layout* l, int part, int64_t* offset, int64_t* count) {
  if (!l || !offset || !count || part < 0 || part > 3) return DIB_E_ARG;
  long long beg, end;
  part_bounds(l, part, &beg, &end);
  *offset = beg;
  *count = end - beg;
  return DIB_OK;
}

}  // extern "C"
