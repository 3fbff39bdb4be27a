// host/encoder.h - the encoder bank: fused large-batch kernels (csrc/dib_fused.h), row-tile kernels (csrc/dib_small.h), the
// grouped-GEMM chain, and the predicates that pick between them.

template <int H1, int H2, int E, bool RELU>
static int launch_fused_fwd(const DibFusedFwdArgs& a, int gx, int F, hipStream_t st) {
  using C = DibFusedCfg<H1, H2, E>;
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  return launch_lds<&dib_fused_encoder_fwd_kernel<H1, H2, E, RELU>>(dim3(gx, F), dim3(512), lds, st, a);
}

// Persistent grid of the fused kernels: gx workgroups per feature, each looping over batch tiles.  One workgroup fills a
// CU (150 KB of LDS), so gx = floor(256 / F): the whole grid is co-resident.  (Rounding UP - the round-1 rule - gave F = 50
// 6 x 50 = 300 workgroups on 256 CUs: a second, 17 %-full wave of workgroups doubled the kernel time.)
static int fused_gx(const dib_layout* l, int batch) { return std::max(1, std::min(cdiv(batch, 256), std::max(1, 256 / l->F))); }

// fused backward dgrad chain is instantiated for the configs whose E is a multiple of 32
static bool fused_bwd_ok(const dib_layout* l) {
  if (!(l->fused_id == 0 || l->fused_id == 1)) return false;
  for (int f = 0; f < l->F; ++f)
    if (l->in_dim[f] > 15) return false;  // row in_dim of the 16-row d(W1|b1) tile carries the bias gradient
  return true;
}

// Whether the training forward of this (layout, batch) may leave h1 unwritten because the layer-2 weight gradient will recompute it
// (csrc/dib_wgrad_recompute.h), and the launch that weight gradient will then be.  Evaluated AT THE FORWARD and recorded per
// workspace (dib_layout::h1_plan); the backward launches by the record, so a dib_set_tuning between the two calls cannot make it
// read a stash that was not written.  All of: fused forward and backward of the 128-wide configuration, not the row-tile regime,
// every feature's input at most 8 wide (one k-block of the forward's layer 1), the tuning key, and the layer-2 weight gradient of
// this batch on the LDS-free kernel's 128-column tiles - the question launch_gemm<2> will ask (wgrad_stream_plan), with the
// arguments encoder_bank_bwd_stages will pass.
static bool use_small_enc(const dib_layout* l, int batch);
static dib_layout::H1Plan h1_recompute_plan(const dib_layout* l, const dib_layout::WsMap& m, const float* w, int batch) {
  dib_layout::H1Plan r;
  if (!knobs().wgrad_recompute_h1 || l->fused_id != 0 || !fused_bwd_ok(l) || l->h1_side.empty() || !l->dev_h1_side) return r;
  if (use_small_enc(l, batch)) return r;
  const GemmCall& c = l->enc_wgrad[1];
  WgradStreamPlan sp;
  if (!wgrad_stream_plan(l->table.data() + c.first, c, w + m.enc_h[0], w + m.g_enc_h[1], batch, m.nsplit, m.rows_per_split,
                         /*auto_split=*/true, m.nsplit, &sp) || sp.nt != 4)
    return r;
  r.recompute = true; r.ch = sp.ch; r.nsplit = sp.nsplit; r.rows_per_split = sp.rows_per_split;
  return r;
}
static void h1_plan_record(const dib_layout* l, const void* ws, const dib_layout::H1Plan& p) {
  std::lock_guard<std::mutex> lk(l->wg_mu);
  if (p.recompute) l->h1_plan[ws] = p;
  else l->h1_plan.erase(ws);   // (no entry = the stash is what the backward reads)
}
static dib_layout::H1Plan h1_plan_of(const dib_layout* l, const void* ws) {
  std::lock_guard<std::mutex> lk(l->wg_mu);
  auto it = l->h1_plan.find(ws);
  return it == l->h1_plan.end() ? dib_layout::H1Plan() : it->second;
}

static int fused_encoder_fwd(dib_layout* l, const dib_layout::WsMap& m, float* w, const float* x, int64_t ldx,
                             const int32_t* row_idx, int64_t row0, int batch, const float* params, uint64_t seed,
                             uint32_t step, int deterministic, hipStream_t st, int* gx_out) {
  DibFusedFwdArgs a;
  a.P = w + m.P; a.row_idx = (const int*)row_idx; a.row0 = row0; a.batch = batch; a.params = params;
  a.w_off = l->dev_fused_offs; a.b_off = l->dev_fused_offs + 3 * l->F; a.featmap = l->dev_featmap;
  a.n_blocks = l->n_blocks; a.act = l->act;
  a.h1 = w + m.enc_h[0]; a.h2 = w + m.enc_h[1]; a.enc_out = w + m.enc_out; a.U = w + m.U;
  a.kl_partial = w + m.kl_partial; a.F = l->F; a.seed = seed; a.step = step;
  a.deterministic = deterministic & DIB_FWD_DETERMINISTIC;
  a.h2mask = (unsigned long long*)(w + m.h2mask);
  a.h1mask = fused_bwd_ok(l) ? (unsigned long long*)(w + m.h1mask) : nullptr;
  if (deterministic & DIB_FWD_INFERENCE) { a.h1 = nullptr; a.h2 = nullptr; a.h2mask = nullptr; a.h1mask = nullptr; }  // no backward follows
  else {   // the layer-2 weight gradient will recompute h1: only its act' bits are stashed
    const dib_layout::H1Plan plan = h1_recompute_plan(l, m, w, batch);
    h1_plan_record(l, w, plan);
    if (plan.recompute) a.h1 = nullptr;
  }
  a.step_dev = l->step_dev;
  const int gx = fused_gx(l, batch);
  *gx_out = gx;
  ProfScope ps(kProfFusedFwd, st);
  switch (l->fused_id) {
    case 0: return l->act == 1 ? launch_fused_fwd<128, 128, 32, true>(a, gx, l->F, st)
                                : launch_fused_fwd<128, 128, 32, false>(a, gx, l->F, st);
    case 1: return l->act == 1 ? launch_fused_fwd<32, 32, 32, true>(a, gx, l->F, st)
                                : launch_fused_fwd<32, 32, 32, false>(a, gx, l->F, st);
    case 2: return l->act == 1 ? launch_fused_fwd<32, 32, 8, true>(a, gx, l->F, st)
                                : launch_fused_fwd<32, 32, 8, false>(a, gx, l->F, st);
    case 3: return l->act == 1 ? launch_fused_fwd<64, 64, 16, true>(a, gx, l->F, st)
                                : launch_fused_fwd<64, 64, 16, false>(a, gx, l->F, st);
    default: return DIB_E_UNSUPPORTED;
  }
}

template <int H1, int H2, int E, bool RELU>
static int launch_fused_bwd(const DibFusedBwdArgs& a, int gx, int F, hipStream_t st) {
  using C = DibFusedBwdCfg<H1, H2, E>;
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  return launch_lds<&dib_fused_encoder_bwd_kernel<H1, H2, E, RELU>>(dim3(gx, F), dim3(512), lds, st, a);
}

static int fused_encoder_bwd(dib_layout* l, const dib_layout::WsMap& m, float* w, int batch, const float* params,
                             const float* beta_dev, float inv_bg, hipStream_t st) {
  DibFusedBwdArgs a;
  a.P = w + m.P; a.batch = batch; a.params = params;
  a.w_off = l->dev_fused_offs; a.b_off = l->dev_fused_offs + 3 * l->F; a.featmap = l->dev_featmap; a.act = l->act;
  a.h2mask = (const unsigned long long*)(w + m.h2mask); a.h1mask = (const unsigned long long*)(w + m.h1mask);
  a.enc_out = w + m.enc_out; a.U = w + m.U; a.GU = w + m.g_u;
  a.dout = w + m.dout; a.dh2 = w + m.g_enc_h[1]; a.dw1_partial = w + m.dw1_partial;
  a.beta_dev = beta_dev; a.inv_bg = inv_bg; a.F = l->F;
  const int gx = fused_gx(l, batch);
  ProfScope ps(kProfFusedBwd, st);
  switch (l->fused_id) {
    case 0: return l->act == 1 ? launch_fused_bwd<128, 128, 32, true>(a, gx, l->F, st)
                                : launch_fused_bwd<128, 128, 32, false>(a, gx, l->F, st);
    case 1: return l->act == 1 ? launch_fused_bwd<32, 32, 32, true>(a, gx, l->F, st)
                                : launch_fused_bwd<32, 32, 32, false>(a, gx, l->F, st);
    default: return DIB_E_UNSUPPORTED;
  }
}

// ---- small-batch row-tile path (dib_small.h) ---------------------------------------------------------------------
static int small_tiles(int batch) { return cdiv(batch, DIB_SMALL_ROWS); }
// The row-tile regime: while (row tiles x features) - the encoder kernels' workgroup count - is at most "small_wgs" (512: two
// rounds of the 256 CUs).  Measured crossover of the Keras-path training step against the large-batch kernels, F = 2 .. 64 x
// B = 128 .. 2048 (profiles/r05x_small_batch_crossover.txt): row tiles win at <= 512 (0.47 - 0.93 of the large path's time), lose
// from 640 up (1.05 - 2.4 x); a fixed row limit of 1024 had F = 64 at B = 1024 at 1.8 x and left F = 4 at B = 2048 (the chaos
// notebook's loop) on the large path at 1 / 0.8.
static bool small_regime(const dib_layout* l, int batch) {
  return knobs().small_batch && batch <= kSmallMaxBatch &&
         (long long)small_tiles(batch) * l->F <= std::min(knobs().small_wgs, kSmallMaxEncWgs);
}
static bool use_small_enc(const dib_layout* l, int batch) { return l->sb_enc && small_regime(l, batch); }
static bool use_small_int(const dib_layout* l, int batch) { return l->sb_int && small_regime(l, batch); }
// the backward's d(W1|b1) comes as per-workgroup partials (fused backward or small-batch backward): how many
static int enc_dw1_parts(const dib_layout* l, int batch) {
  if (use_small_enc(l, batch)) return small_tiles(batch);
  return fused_bwd_ok(l) ? fused_gx(l, batch) * 8 : 0;
}
// rows of the KL partial table the forward of this (layout, batch) writes
static int enc_kl_rows(const dib_layout* l, const dib_layout::WsMap& m, int batch) {
  if (use_small_enc(l, batch)) return small_tiles(batch);
  return l->fused_id >= 0 ? fused_gx(l, batch) * 8 : m.kl_blocks;
}

static int small_encoder_fwd(dib_layout* l, const dib_layout::WsMap& m, float* w, const float* x, int64_t ldx,
                             const int32_t* row_idx, int64_t row0, int batch, const float* params, uint64_t seed, uint32_t step,
                             int flags, hipStream_t st) {
  DibSmallEncFwdArgs a;
  a.X = x; a.ldx = ldx; a.row_idx = (const int*)row_idx; a.row0 = row0; a.batch = batch; a.params = params;
  a.w_off = l->dev_fused_offs; a.b_off = l->dev_fused_offs + 3 * l->F; a.featmap = l->dev_featmap;
  a.n_blocks = l->n_blocks; a.act = l->act; a.F = l->F; a.E = l->E; a.H1 = l->enc_units[0]; a.H2 = l->enc_units[1];
  const bool infer = (flags & DIB_FWD_INFERENCE) != 0;
  a.P = infer ? nullptr : w + m.P; a.h1 = infer ? nullptr : w + m.enc_h[0]; a.h2 = infer ? nullptr : w + m.enc_h[1];
  a.enc_out = w + m.enc_out; a.U = w + m.U; a.kl_partial = w + m.kl_partial;
  a.seed = seed; a.step = step; a.deterministic = flags & DIB_FWD_DETERMINISTIC; a.step_dev = l->step_dev;
  const size_t lds = small_encoder_lds(a.H1, a.H2, a.E, false);
  ProfScope ps(kProfOther, st);
  return launch_lds<&dib_small_encoder_fwd_kernel>(dim3(small_tiles(batch), l->F), dim3(DIB_SMALL_THREADS), lds, st, a);
}

static int small_encoder_bwd(dib_layout* l, const dib_layout::WsMap& m, float* w, int batch, const float* params,
                             const float* beta_dev, float inv_bg, hipStream_t st) {
  DibSmallEncBwdArgs a;
  a.P = w + m.P; a.batch = batch; a.params = params;
  a.w_off = l->dev_fused_offs; a.b_off = l->dev_fused_offs + 3 * l->F; a.featmap = l->dev_featmap;
  a.act = l->act; a.F = l->F; a.E = l->E; a.H1 = l->enc_units[0]; a.H2 = l->enc_units[1];
  a.h1 = w + m.enc_h[0]; a.h2 = w + m.enc_h[1]; a.enc_out = w + m.enc_out; a.U = w + m.U; a.GU = w + m.g_u;
  a.dout = w + m.dout; a.dh2 = w + m.g_enc_h[1]; a.dw1_partial = w + m.dw1_partial; a.beta_dev = beta_dev; a.inv_bg = inv_bg;
  const size_t lds = small_encoder_lds(a.H1, a.H2, a.E, true);
  ProfScope ps(kProfOther, st);
  return launch_lds<&dib_small_encoder_bwd_kernel>(dim3(small_tiles(batch), l->F), dim3(DIB_SMALL_THREADS), lds, st, a);
}

// when one grouped launch for all weight gradients pays: the small-batch regime, where every launch is latency
static bool use_merged_wgrad(const dib_layout* l, int batch) {
  return use_small_enc(l, batch) && use_small_int(l, batch);
}

// ---- forward ---------------------------------------------------------------------------------
static int encoder_chain_fwd(dib_layout* l, const dib_layout::WsMap& m, float* w, int batch, const float* params,
                             int first_group_offset, int group_count, hipStream_t st) {
  const int LE = l->n_enc + 1;
  for (int ly = 0; ly < LE; ++ly) {
    GemmCall c = l->enc_fwd[ly];
    c.first += first_group_offset;
    c.count = group_count;
    const float* A = ly == 0 ? w + m.P : w + m.enc_h[ly - 1];
    float* C = ly == LE - 1 ? w + m.enc_out : w + m.enc_h[ly];
    const int act = ly == LE - 1 ? DIB_ACT_LINEAR : l->act;  // reference models.py:78: last Dense(2E) is linear
    int rc = launch_gemm<0>(l, c, A, params, C, params, nullptr, nullptr, batch, act, 1, 0, 0, st);
    if (rc) return rc;
  }
  return DIB_OK;
}

// stages: bit 0 = the gradient chain (reparam/KL backward + dgrads) and every weight gradient except the last encoder
// layer's; bit 1 = the last layer's weight gradient (independent of the others: it reads dout and the last hidden layer).
// 3 = both, in the single-GPU order (last layer first).  The data-parallel caller runs stage 1, finalizes + all-reduces
// part 2 (the front layers), then runs stage 2 under that all-reduce (dib_encoder_bank_bwd_stage).
static int encoder_bank_bwd_stages(dib_layout* l, int batch, const float* params, float* grads, const float* beta_dev,
                                   float inv_global_batch, int stages, void* ws, dib_stream_t stream) {
  if (!l || !params || !grads || !beta_dev || !ws || batch <= 0 || stages < 1 || stages > 3) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  float* gt = wgrad_target(m, w, grads);
  const long long sstride = align_up(l->n_params, 4);
  int rc = DIB_OK;
  const bool small = use_small_enc(l, batch);
  const bool fused = small || fused_bwd_ok(l);   // d(W1|b1) comes as per-workgroup partials, dgrads in one launch
  const int LE = l->n_enc + 1;
  if (stages & 1) {
    if (small) {  // 16-row tiles (dib_small.h)
      rc = small_encoder_bwd(l, m, w, batch, params, beta_dev, inv_global_batch, st);
    } else if (fused) {  // reparam/KL backward + both dgrads in one launch (dib_fused.h); wgrads below read its outputs
      rc = fused_encoder_bwd(l, m, w, batch, params, beta_dev, inv_global_batch, st);
    } else {
      { ProfScope ps(kProfOther, (hipStream_t)stream);
      DIB_LAUNCH(dib_reparam_kl_bwd_kernel, dim3(m.kl_blocks, l->F), dim3(256), 0, st, w + m.enc_out, w + m.g_u,
                         w + m.U, w + m.dout, beta_dev, inv_global_batch, batch, l->F, l->E); }
      rc = (int)hipGetLastError();
    }
    if (rc) return rc;
  }
  for (int ly = LE - 1; ly >= 0; --ly) {
    const bool last = ly == LE - 1;
    const float* gout = last ? w + m.dout : w + m.g_enc_h[ly];
    const float* hin = ly == 0 ? w + m.P : w + m.enc_h[ly - 1];
    const bool wgrad_here = (last ? (stages & 2) : (stages & 1)) && !(fused && ly == 0);  // fused: d(W1|b1) comes out of the
                                                                                         // fused kernel, reduced at finalize
    if (wgrad_here && ly == 1 && fused && !small) {
      // Layer 2 after a forward that did not stash h1 (h1_recompute_plan): the recorded launch, h1 recomputed from P, W1 and b1.
      // Under the staged data-parallel backward this is stage 1, like every front-layer weight gradient: it runs before any
      // optimizer step touches W1, so the recompute sees the parameters the forward saw.
      const dib_layout::H1Plan plan = h1_plan_of(l, ws);
      if (plan.recompute) {
        const GemmCall& c = l->enc_wgrad[ly];
        rc = launch_wgrad_h1(plan.ch, l->act == 1, l->dev_groups, l->dev_h1_side, c, w + m.P, params, gout, gt, gt, batch, plan.nsplit,
                             plan.rows_per_split, sstride, st);
        if (rc == DIB_OK && m.nsplit > 1)
          rc = retire_stale_slabs(l, batch, l->table.data() + c.first, c.count, plan.nsplit, m.nsplit, gt, sstride, st);
        if (rc) return rc;
        continue;   // (fused: no dgrad launch per layer)
      }
    }
    if (wgrad_here) {
      // narrow outputs (the 2E-wide last layer) run 128x64 tiles at 4 workgroups/CU: half as many, twice as long batch
      // splits fill the chip in one wave (measured 0.88 -> 0.71 ms); the unused slabs of these blocks stay zero.
      // (only from 32 splits = 16384 rows up: at B = 8192 the 16 -> 8 split halving measured 117 vs 103 us)
      // (the per-launch split rule, pick_wgrad_splits, starts from this choice and leaves it unless it predicts > 5 % better)
      const bool halve = l->enc_wgrad[ly].max_n <= 64 && m.nsplit >= 32 && (m.nsplit % 2) == 0;
      rc = launch_gemm<2>(l, l->enc_wgrad[ly], hin, gout, gt, nullptr, nullptr, gt, batch, 0,
                          halve ? m.nsplit / 2 : m.nsplit, halve ? 2 * m.rows_per_split : m.rows_per_split, sstride, st,
                          m.nsplit);
      if (rc) return rc;
    }
    if ((stages & 1) && ly >= 1 && !fused) {
      rc = launch_gemm<1>(l, l->enc_dgrad[ly], gout, params, w + m.g_enc_h[ly - 1], nullptr, hin, nullptr, batch,
                          l->act, 1, 0, 0, st);
      if (rc) return rc;
    }
  }
  return DIB_OK;
}

extern "C" {

int dib_encoder_bank_fwd(dib_layout* l, const float* x, int64_t ldx, const int32_t* row_idx, int64_t row0, int batch,
                         const float* params, uint64_t seed, uint32_t step, int deterministic, void* ws,
                         dib_stream_t stream) {
  if (!l || !x || !params || !ws || batch <= 0) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  { std::lock_guard<std::mutex> lk(l->wg_mu); l->fwd_training[ws] = !(deterministic & DIB_FWD_INFERENCE); }
  if (use_small_enc(l, batch)) {   // gather + positional encoding + Dense chain + reparameterisation + KL partials: one launch
    if (!(deterministic & DIB_FWD_INFERENCE)) h1_plan_record(l, ws, dib_layout::H1Plan());   // (this forward stashes h1)
    int rc = small_encoder_fwd(l, m, w, x, ldx, row_idx, row0, batch, params, seed, step, deterministic, st);
    if (rc || (deterministic & DIB_FWD_DEFER_SUMS)) return rc;
    ProfScope ps(kProfOther, st);
    DIB_LAUNCH(dib_colsum_partials_kernel, dim3(l->F), dim3(256), 0, st, w + m.kl_partial, small_tiles(batch), l->F,
                       w + m.step_out);
    return (int)hipGetLastError();
  }
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  if ((long long)cdiv(l->sum_d, 64) * cdiv(batch, 64) >= 512)
    DIB_LAUNCH(dib_posenc_kernel<64>, dim3(cdiv(l->sum_d, 64), cdiv(batch, 64)), dim3(256), 0, st, x, (long long)ldx,
                       (const int*)row_idx, (long long)row0, batch, l->dev_colmap, l->sum_d, l->n_blocks, w + m.P);
  else
    DIB_LAUNCH(dib_posenc_kernel<16>, dim3(cdiv(l->sum_d, 64), cdiv(batch, 16)), dim3(256), 0, st, x, (long long)ldx,
                       (const int*)row_idx, (long long)row0, batch, l->dev_colmap, l->sum_d, l->n_blocks, w + m.P); }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  if (l->fused_id >= 0) {  // one launch: positional encoding + 3 layers + reparameterisation + KL
    int gx = 1;
    rc = fused_encoder_fwd(l, m, w, x, ldx, row_idx, row0, batch, params, seed, step, deterministic, st, &gx);
    if (rc) return rc;
    if (deterministic & DIB_FWD_DEFER_SUMS) return DIB_OK;   // dib_step_tail(DIB_TAIL_KL) sums the partials
    { ProfScope ps(kProfOther, (hipStream_t)stream);
    DIB_LAUNCH(dib_colsum_partials_kernel, dim3(l->F), dim3(256), 0, st, w + m.kl_partial, gx * 8, l->F,
                       w + m.step_out); }
    return (int)hipGetLastError();
  }
  rc = encoder_chain_fwd(l, m, w, batch, params, 0, l->F, st);
  if (rc) return rc;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_reparam_kl_fwd_kernel, dim3(m.kl_blocks, l->F), dim3(256), 0, st, w + m.enc_out, w + m.U,
                     w + m.kl_partial, (const int*)row_idx, (long long)row0, batch, l->F, l->E,
                     (unsigned long long)seed, (unsigned)step, deterministic & DIB_FWD_DETERMINISTIC, l->step_dev); }
  rc = (int)hipGetLastError();
  if (rc) return rc;
  if (deterministic & DIB_FWD_DEFER_SUMS) return DIB_OK;
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_colsum_partials_kernel, dim3(l->F), dim3(256), 0, st, w + m.kl_partial, m.kl_blocks, l->F,
                     w + m.step_out); }
  return (int)hipGetLastError();
}

int dib_encoder_bank_bwd(dib_layout* l, int batch, const float* params, float* grads, const float* beta_dev,
                         float inv_global_batch, void* ws, dib_stream_t stream) {
  return encoder_bank_bwd_stages(l, batch, params, grads, beta_dev, inv_global_batch, 3, ws, stream);
}

int dib_encoder_bank_bwd_stage(dib_layout* l, int batch, const float* params, float* grads, const float* beta_dev,
                               float inv_global_batch, int stage, void* ws, dib_stream_t stream) {
  if (stage != 1 && stage != 2) return DIB_E_ARG;
  return encoder_bank_bwd_stages(l, batch, params, grads, beta_dev, inv_global_batch, stage, ws, stream);
}

// A caller who wants to LOOK at the first hidden layer after a forward that left it to the weight gradient's recompute: write
// DIB_WS_ENC_H0 + 0 now, from the workspace's P (the last forward's inputs) and `params`, with the grouped GEMM the unfused path
// runs for this layer.  Not the fused forward's arithmetic: a value can differ from the one the step used in its last bit.
int dib_workspace_h1_materialize(dib_layout* l, int batch, const float* params, void* ws, dib_stream_t stream) {
  if (!l || !params || !ws || batch <= 0 || l->n_enc < 1) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  return launch_gemm<0>(l, l->enc_fwd[0], w + m.P, params, w + m.enc_h[0], params, nullptr, nullptr, batch, l->act, 1, 0, 0,
                        (hipStream_t)stream);
}

// ---- evaluation helpers ------------------------------------------------------------------------------
int dib_encode_deterministic(dib_layout* l, int feature, const float* x_f, int n, const float* params, float* out,
                             void* ws, dib_stream_t stream) {
  if (!l || !x_f || !params || !out || !ws || n <= 0) return DIB_E_ARG;
  if (feature < 0 || feature >= l->F) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(n);
  float* w = (float*)ws;
  const int d = l->dims[feature];
  { ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_posenc_kernel<64>, dim3(cdiv(d, 64), cdiv(n, 64)), dim3(256), 0, st, x_f, (long long)d,
                     (const int*)nullptr, 0ll, n, l->dev_colmap + l->x_off[feature], d, l->n_blocks, w + m.P); }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  rc = encoder_chain_fwd(l, m, w, n, params, feature, 1, st);
  if (rc) return rc;
  const int w2 = 2 * l->E;
  return (int)hipMemcpyAsync(out, w + m.enc_out + (int64_t)feature * n * w2, (size_t)n * w2 * sizeof(float),
                             hipMemcpyDeviceToDevice, st);
}

#ifdef DIB_FUSED_TIMING
// diagnostic build only (not declared in include/): phase timers of the last fused encoder forward
int dib_fused_debug_read(long long* out16) {
  if (hipDeviceSynchronize() != hipSuccess) return DIB_E_ARG;
  return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(dib_fused_dbg), 16 * sizeof(long long));
}
#endif

}  // extern "C"
