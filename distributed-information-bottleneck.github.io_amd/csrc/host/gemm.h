// host/gemm.h - tile and split rules of the grouped GEMM (csrc/dib_gemm.h), the layout's weight-gradient launches and the
// stand-alone GEMM entry points (include/dib_hip.h dib_gemm, include/dib_st.h dib_gemm_grouped / dib_gemm_skinny_k).

namespace {

template <int MODE, int NI, int NJ, bool FLAT = false>
int launch_gemm_t(const DibGemmGroup* dev_groups, const GemmCall& c, int M, int N, const float* A, const float* B, float* C,
                  const float* bias, const float* aux, float* bias_out, int batch, int act, int nsplit,
                  int rows_per_split, long long split_stride, hipStream_t st) {
  const int tm = cdiv(M, FLAT ? 32 : 64 * NI), tn = cdiv(N, FLAT ? 256 : 64 * NJ);
  // grid.y / grid.z are limited to 65535: a clean return code instead of a launch error
  if (c.count > 65535 || (MODE == 2 && (long long)tm * tn > 65535)) return DIB_E_UNSUPPORTED;
  dim3 grid;
  if (MODE == 2) grid = dim3(nsplit, tm * tn, c.count);
  else grid = dim3(8 * cdiv(tm, 8) * tn, 1, c.count);  // XCD-aware 1-D tile order, see dib_gemm.h
  // K-tile depth per tile shape (each a same-box A/B, profiles/HISTORY.md): 64 for the 128 x 128 tile of every mode - one
  // prefetch + barrier pair per 64-deep MFMA phase hides the HBM latency a 32-deep phase exposes (+18 %) - and for the 64 x 128
  // weight-gradient tile of the 256 x 256 integration layer (0.136 -> 0.124 ms); 32 for the other narrow tiles.
  // (the flat 32 x 256 weight-gradient tile: 32 - its 256-column operand tile at 64 deep would need 76 KB of static LDS)
  constexpr int BK = FLAT ? 32 : ((NI == 2 && NJ == 2) ? 64 : ((MODE == 2 && NI == 1 && NJ == 2) ? 64 : 32));
  // cache policy of the streamed operands / outputs (dib_gemm.h: stream_flags): non-temporal from 8192 streamed rows up
  // (DIB_GEMM_STREAM_ROWS; M for forward / dgrad, the contracted rows for a weight gradient)
  const long long streamed_rows = MODE == 2 ? (long long)nsplit * rows_per_split : (long long)M;
  // ... and the output non-temporally only when it cannot stay in the 256 MB infinity cache for its consumer anyway (the 67 MB
  // hidden activation of the integration network, stored non-temporally, cost the fused head that reads it next 19 us)
  const bool big_out = MODE != 2 && (long long)M * N * (long long)sizeof(float) * c.count >= (256ll << 20);
  const int stream_flags = streamed_rows >= knobs().stream_rows ? (big_out ? 3 : 1) : 0;
  DIB_LAUNCH((dib_gemm_kernel<MODE, NI, NJ, BK, FLAT>), grid, dim3(256), 0, st, dev_groups + c.first, A, B, C,
                     bias, aux, bias_out, batch, act, tm, tn, rows_per_split, split_stride, stream_flags);
  return (int)hipGetLastError();
}

// ---- the LDS-free weight gradient (csrc/dib_wgrad_stream.h) ----
constexpr int kWgradStreamWavesPerCu = 4;   // one wave-tile per SIMD
// What the kernel asks of a launch apart from its slab length: every group M % 128 == 0 and N == 64 (all groups) or
// N % 128 == 0 (all groups), operands 16-byte aligned with lda / ldb multiples of 4, whole 64-row K-tiles.  Needs the groups on
// the host: launches that only have the device table (dib_gemm_grouped) stay on the tiled kernel.
static bool wgrad_stream_shape_ok(const DibGemmGroup* hg, int count, int batch, const float* A, const float* B, int* nt_out) {
  if (!knobs().wgrad_stream || !hg || count <= 0) return false;
  if ((((uintptr_t)A | (uintptr_t)B) & 15) != 0) return false;
  int nt = 0;
  for (int i = 0; i < count; ++i) {
    const DibGemmGroup& g = hg[i];
    const int M = g.M < 0 ? batch : g.M, N = g.N < 0 ? batch : g.N, K = g.K < 0 ? batch : g.K;
    if (M <= 0 || (M & 127) || K <= 0 || (K & 63)) return false;
    const int nt_g = N == 64 ? 2 : ((N > 0 && (N & 127) == 0) ? 4 : 0);
    if (!nt_g || (nt && nt != nt_g)) return false;
    nt = nt_g;
    if (((g.a_off + g.a_boff * batch) | (g.b_off + g.b_boff * batch) | (long long)g.lda | (long long)g.ldb) & 3) return false;
    if (g.lda < M || g.ldb < N) return false;
  }
  *nt_out = nt;
  return true;
}
// ... and of its slabs: whole K-tiles, at least "wgrad_stream_rows" streamed rows, 32-bit byte offsets inside a slab - and
// enough of them: a wave-tile is a whole 128 x 128 output tile of one slab, four per CU, so a launch with few tiles leaves
// most SIMDs idle where the tiled kernel's smaller tiles fill them (the 256 x 256 integration layer at B = 65536: 4 tiles x 32
// slabs = 128 waves; on this kernel it took as long as the 2048-wave encoder layer and the step lost 0.45 ms).  "wgrad_stream_fill":
// the waves must fill this many percent of one round of the chip's wave slots.
static bool wgrad_stream_slabs_ok(const DibGemmGroup* hg, int count, int batch, long long tiles, int nsplit, int rows_per_split) {
  if (nsplit <= 0 || rows_per_split <= 0 || (long long)nsplit * rows_per_split < knobs().wgrad_stream_rows) return false;
  if (tiles * nsplit * 100 < (long long)knobs().wgrad_stream_fill * split_rule_cus() * kWgradStreamWavesPerCu) return false;
  for (int i = 0; i < count; ++i) {
    const int K = hg[i].K < 0 ? batch : hg[i].K;
    if ((rows_per_split & 63) && !(nsplit == 1 && rows_per_split >= K)) return false;
    if (((long long)std::min(rows_per_split, K) + 8) * std::max(hg[i].lda, hg[i].ldb) * 4 >= (1ll << 31)) return false;
  }
  return true;
}
// The grid of its launches and of dib_wgrad_h1_kernel's: one wave per (128 x tile_n output tile, slab), four waves per workgroup;
// ntl: operands loaded non-temporally - the tiled kernels' cache policy of streamed operands ("stream_rows")
struct WgradWaveGrid { int tm, tn; dim3 grid; bool ntl; };
static int wgrad_wave_grid(int M, int N, int tile_n, int count, int nsplit, int rows_per_split, WgradWaveGrid* w) {
  const int tm = cdiv(M, 128), tn = cdiv(N, tile_n);
  const long long waves = (long long)tm * tn * count * nsplit;
  if (waves >= (1ll << 31)) return DIB_E_UNSUPPORTED;
  *w = {tm, tn, dim3((unsigned)((waves + 3) / 4)), (long long)nsplit * rows_per_split >= knobs().stream_rows};
  return DIB_OK;
}
// NT: 4 = 128-column tiles, 2 = 64-column tiles; CH: the bias chains of the tiled kernel this launch replaces (dib_wgrad_stream.h)
template <int NT, int CH>
int launch_wgrad_stream(const DibGemmGroup* dev_groups, const GemmCall& c, int M, int N, const float* A, const float* B, float* C,
                        float* bias_out, int batch, int nsplit, int rows_per_split, long long split_stride, hipStream_t st) {
  WgradWaveGrid w;
  if (int rc = wgrad_wave_grid(M, N, 32 * NT, c.count, nsplit, rows_per_split, &w)) return rc;
  ProfScope ps(NT == 4 ? kProfWgradStream128 : kProfWgradStream64, st);
  const auto kernel = w.ntl ? dib_wgrad_stream_kernel<NT, CH, true> : dib_wgrad_stream_kernel<NT, CH, false>;
  DIB_LAUNCH(kernel, w.grid, dim3(256), 0, st, dev_groups + c.first, A, B, C, bias_out, batch, c.count, w.tm, w.tn, nsplit,
             rows_per_split, split_stride);
  return (int)hipGetLastError();
}

// ---- the LDS-free forward / dgrad GEMM (csrc/dib_gemm_stream.h) ----
// Whether a forward (mode 0) / dgrad (mode 1) launch goes to dib_gemm_stream_kernel, and with how many waves.  It takes ONE
// group (the integration network's layers, dib_gemm) with M % 128 == 0, N % 128 == 0, K % 32 == 0, operands, output and mask
// 16-byte aligned with leading dimensions that are multiples of 4, 32-bit byte offsets inside a tile's operand extents, a linear /
// relu / leaky-relu activation - from "gemm_stream_rows" rows up, and only when its wave-tiles (128 x 128 output tiles) fill
// "gemm_stream_fill" percent of one round of the chip's wave slots (four per CU): a launch with fewer tiles leaves SIMDs idle where
// the tiled kernel's smaller tiles fill them.  Needs the group on the host (launches that only have the device table stay tiled).
// Every layer it takes measured faster than the tiled kernel in every alternating pair of tools/gemm_stream_bench.hip
// (profiles/HISTORY.md section 27).
struct GemmStreamPlan { int tiles_m = 0, tiles_n = 0, nwaves = 0, kind = 0; };
static bool gemm_stream_plan(int mode, const DibGemmGroup* hg, const GemmCall& c, const float* A, const float* B, const float* C,
                             const float* bias, const float* aux, int batch, int act, GemmStreamPlan* plan) {
  if (!knobs().gemm_stream || !hg || c.count != 1 || (mode != 0 && mode != 1)) return false;
  if (!(act == 0 || act == 1 || act == 2 || act == 7)) return false;   // the activations its unrolled epilogue carries
  const DibGemmGroup& g = hg[0];
  const long long M = g.M < 0 ? batch : g.M, N = g.N < 0 ? batch : g.N, K = g.K < 0 ? batch : g.K;
  if (M <= 0 || (M & 127) || N <= 0 || (N & 127) || K <= 0 || (K & 31)) return false;
  if (M < knobs().gemm_stream_rows) return false;
  const bool mask = mode == 1 && aux != nullptr && act != 0;
  if ((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (mask ? (uintptr_t)aux : 0)) & 15) != 0) return false;
  if (((g.a_off + g.a_boff * batch) | (g.b_off + g.b_boff * batch) | (g.c_off + g.c_boff * batch) | (long long)g.lda | (long long)g.ldb |
       (long long)g.ldc) & 3)
    return false;
  if (mask && (((g.aux_off + g.aux_boff * batch) | (long long)g.ldaux) & 3)) return false;
  if (g.lda < K || g.ldb < (mode == 0 ? N : K) || g.ldc < N || (mask && g.ldaux < N)) return false;
  // a tile's extents: 128 rows of A, C and the mask; K rows (mode 0) / 128 rows (mode 1) of B
  const long long ext = std::max({128ll * g.lda, (mode == 0 ? K : 128ll) * g.ldb, 128ll * g.ldc, mask ? 128ll * g.ldaux : 0ll});
  if ((ext + 8) * 4 >= (1ll << 31)) return false;
  const long long tm = M / 128, tn = N / 128, tiles = tm * tn;
  if (tiles >= (1ll << 31)) return false;
  const long long slots = (long long)split_rule_cus() * kWgradStreamWavesPerCu;
  if (tiles * 100 < (long long)knobs().gemm_stream_fill * slots) return false;
  plan->tiles_m = (int)tm;
  plan->tiles_n = (int)tn;
  plan->nwaves = (int)std::min(tiles, slots);   // one wave per SIMD; a wave walks tiles / nwaves (+ 1) consecutive tiles
  plan->kind = mode == 0 ? (act == 0 ? 0 : (act == 1 ? 1 : 2)) : (mask ? 3 : 0);
  return true;
}
// {whether the plan took the call, the launch's return code}; dev_group / hg: the call's one group on the device / on the host
template <int MODE>
std::pair<bool, int> try_gemm_stream(const DibGemmGroup* dev_group, const DibGemmGroup* hg, const GemmCall& c, const float* A, const float* B,
                                     float* C, const float* bias, const float* aux, int batch, int act, hipStream_t st) {
  GemmStreamPlan sp;
  if (!gemm_stream_plan(MODE, hg, c, A, B, C, bias, aux, batch, act, &sp)) return {false, DIB_OK};
  ProfScope ps(MODE * 4 + 3, st, MODE == 0 ? kPartGemmStreamFwd : kPartGemmStreamDgrad);   // timed with the tiled kernel it stands in for
  // launch_gemm_t's rule for the output: non-temporal stores for a streamed launch whose output cannot stay in the infinity cache
  const long long M = hg->M < 0 ? batch : hg->M, N = hg->N < 0 ? batch : hg->N;
  const int nts = M >= knobs().stream_rows && M * N * (long long)sizeof(float) >= (256ll << 20) ? 1 : 0;
  const dim3 grid((unsigned)((sp.nwaves + 3) / 4));
#define DIB_GO(KIND) DIB_LAUNCH((dib_gemm_stream_kernel<MODE, KIND>), grid, dim3(256), 0, st, dev_group, A, B, C, bias, aux, batch, act, \
                                sp.tiles_m, sp.tiles_n, sp.nwaves, nts)
  if constexpr (MODE == 0) {
    if (sp.kind == 1) DIB_GO(1);
    else if (sp.kind == 0) DIB_GO(0);
    else DIB_GO(2);
  } else {
    if (sp.kind == 3) DIB_GO(3);
    else DIB_GO(0);
  }
#undef DIB_GO
  return {true, (int)hipGetLastError()};
}

// Batch-split count of one weight-gradient launch: `tiles` output tiles (all groups) x ns splits of rps batch rows on `slots`
// co-resident workgroup slots (256 CUs x workgroups per CU of the tile shape).  Equal-length workgroups execute in
// ceil(tiles ns / slots) rounds, so the launch takes ~ rounds x (rps + a fixed cost per workgroup).  The layout-wide rule - 32
// splits of 2048 rows at B = 65536 - is exact for F = 64 (64 tiles x 32 = 4.0 rounds of 512) and off for F = 50: 1600
// workgroups = 3.1 rounds, the fourth 1/8 full; the narrow last-layer gradient (4 workgroups per CU) with its splits halved
// ran 800 workgroups of 4096 rows where 1000 of 3328 fit one round.  BASELINE config 4: encoder wgrads at 0.55-0.61 of the
// fp32-MFMA peak against 0.70-0.72 for config 3 (profiles/r04a_config4_*).  Candidates: 1 .. max_splits splits of a multiple of
// 64 rows (whole K-tiles), at least kSplitRows rows; the cheapest wins, ties go to FEWER, longer workgroups.
// Measured (F = 50, B = 65536, ms/step with one launch's count forced, profiles/r04d_split_sweep_F50.txt): encoder layers 2+3,
// 50 tiles: 32 splits 6.80, 30: 6.78, 28: 6.87, 25: 6.74, 20: 6.68 (2 full rounds), 16: 6.99, 10: 6.71 (1 round);
// integration layer 1, 26 tiles: 32: 6.80, 29: 6.73, 24: 6.83, 19: 6.66 (1 round), 16: 6.82, 13: 7.01.  (A second model, "what
// a CU executes is serial: ceil(tiles ns / 256) x rps", picked 25 and 29 there and measured no gain: r04c.)
// Slabs beyond the chosen count are never written by this launch and stay zero (include/dib_hip.h workspace contract).
static void pick_wgrad_splits(long long tiles, int slots, int K, int max_splits, int* ns_out, int* rps_out) {
  const int min_rows = std::min(kSplitRows, std::max(64, *rps_out));   // narrow layouts come in with shorter slabs (WsMap)
  // The caller's (layout-wide) split is kept whenever it fills its rounds to at least 85 %: BASELINE config 3 (F = 64: 64 or 32
  // tiles x 32 or 16 splits = whole rounds at every batch size) then runs exactly the launches rounds 2-3 measured and
  // validated (same-box A/B of an unconditional rule vs no rule there: 8.00-8.08 vs 7.99-8.02 ms/step,
  // profiles/r04e_split_policy_final_ab.txt).
  const auto cost_of = [&](int ns, int rps) {
    return (double)((tiles * ns + slots - 1) / slots) * (rps + knobs().split_overhead);
  };
  {
    const long long wgs = tiles * *ns_out, rounds = (wgs + slots - 1) / slots;
    if ((double)wgs >= 0.85 * (double)(rounds * slots)) return;
  }
  double best = 1e300;
  int bns = *ns_out, brps = *rps_out;
  for (int ns = 1; ns <= max_splits; ++ns) {
    const int rps = cdiv(cdiv(K, ns), 64) * 64;
    if (ns > 1 && rps < min_rows) break;
    if (cdiv(K, rps) != ns) continue;   // the same split as a smaller ns
    const double cost = cost_of(ns, rps);
    if (cost < best) {
      best = cost;
      bns = ns;
      brps = rps;
    }
  }
  if (best >= cost_of(*ns_out, *rps_out)) return;
  *ns_out = bns;
  *rps_out = brps;
}

// The tile rule of a weight gradient: narrow tiles for narrow outputs, and 64-row (then 64-column) tiles while 128 x 128 tiles x
// splits do not fill 256 CUs (e.g. a 256 x 256 layer, tiny batches)
static void wgrad_tile_rule(int M, int N, int nsplit, int count, bool* ni1, bool* nj1) {
  *ni1 = M <= 64;
  *nj1 = N <= 64;
  if (!*ni1 && !*nj1) {
    const long long wgs = (long long)cdiv(M, 128) * cdiv(N, 128) * nsplit * count;
    if (wgs < 256) *ni1 = true;
    if (*ni1 && !*nj1 && (long long)cdiv(M, 64) * cdiv(N, 128) * nsplit * count < 128) *nj1 = true;  // tiny batches
  }
}

// Whether a weight-gradient launch goes to the LDS-free kernel, and how: nt = 4 / 2 (128- / 64-column tiles), ch = the bias chains
// of the tiled kernel it replaces, the split it will run.  ONE question for the launch (launch_gemm<2>) and for whoever must know
// its answer earlier (the fused forward deciding whether the layer-2 weight gradient will need the h1 stash, host/encoder.h).
struct WgradStreamPlan { int nt = 0, ch = 0, nsplit = 0, rows_per_split = 0; };
static bool wgrad_stream_plan(const DibGemmGroup* host_groups, const GemmCall& c, const float* A, const float* B, int batch, int nsplit,
                              int rows_per_split, bool auto_split, int max_splits, WgradStreamPlan* plan) {
  const int M = c.max_m < 0 ? batch : c.max_m, N = c.max_n < 0 ? batch : c.max_n;
  int nt = 0;
  if (c.count <= 0 || !wgrad_stream_shape_ok(host_groups, c.count, batch, A, B, &nt)) return false;
  int ns = nsplit, rps = rows_per_split;
  const long long tiles = (long long)cdiv(M, 128) * cdiv(N, 32 * nt) * c.count;
  if (auto_split && ns > 1 && knobs().split_policy)
    pick_wgrad_splits(tiles, split_rule_cus() * kWgradStreamWavesPerCu, batch, std::max(ns, max_splits), &ns, &rps);
  if (!wgrad_stream_slabs_ok(host_groups, c.count, batch, tiles, ns, rps)) return false;
  bool ni1, nj1;
  wgrad_tile_rule(M, N, nsplit, c.count, &ni1, &nj1);
  plan->nt = nt;
  // (a 128-column launch the tile rule would have put on 64-column tiles sums its bias the way those do)
  plan->ch = nt == 2 || nj1 ? 4 : 2;
  plan->nsplit = ns;
  plan->rows_per_split = rps;
  return true;
}

// dib_wgrad_stream_kernel<4, CH, NTL>'s launch with the A operand recomputed (csrc/dib_wgrad_recompute.h): P, params and the
// per-group side table instead of A.  ch: the bias chains (2 / 4); relu: the fused forward's RELU specialisation (act == 1)
template <int CH, bool RELU>
int launch_wgrad_h1_t(const DibGemmGroup* dev_groups, const DibWgradH1Side* dev_side, const GemmCall& c, int M, int N, const float* P,
                      const float* params, const float* B, float* C, float* bias_out, int batch, int nsplit, int rows_per_split,
                      long long split_stride, hipStream_t st) {
  WgradWaveGrid w;
  if (int rc = wgrad_wave_grid(M, N, 128, c.count, nsplit, rows_per_split, &w)) return rc;
  ProfScope ps(kProfWgradStream128, st, kPartWgradH1);   // timed with the kernel it stands in for
  const auto kernel = w.ntl ? dib_wgrad_h1_kernel<CH, true, RELU> : dib_wgrad_h1_kernel<CH, false, RELU>;
  DIB_LAUNCH(kernel, w.grid, dim3(256), 0, st, dev_groups + c.first, dev_side, P, params, B, C, bias_out, batch, c.count, w.tm, w.tn,
             nsplit, rows_per_split, split_stride);
  return (int)hipGetLastError();
}
static int launch_wgrad_h1(int ch, bool relu, const DibGemmGroup* dev_groups, const DibWgradH1Side* dev_side, const GemmCall& c,
                           const float* P, const float* params, const float* B, float* C, float* bias_out, int batch, int nsplit,
                           int rows_per_split, long long split_stride, hipStream_t st) {
#define DIB_GO(CH, RELU) launch_wgrad_h1_t<CH, RELU>(dev_groups, dev_side, c, c.max_m, c.max_n, P, params, B, C, bias_out, batch, nsplit, \
                                                     rows_per_split, split_stride, st)
  if (ch == 4) return relu ? DIB_GO(4, true) : DIB_GO(4, false);
  return relu ? DIB_GO(2, true) : DIB_GO(2, false);
#undef DIB_GO
}

template <int MODE>
int launch_gemm(const DibGemmGroup* dev_groups, const GemmCall& c, const float* A, const float* B, float* C,
                const float* bias, const float* aux, float* bias_out, int batch, int act, int nsplit, int rows_per_split,
                long long split_stride, hipStream_t st, bool auto_split = false, int max_splits = 0, int* ns_used = nullptr,
                const DibGemmGroup* host_groups = nullptr) {
  if (ns_used) *ns_used = nsplit;
  if (c.count == 0) return DIB_OK;
  const int M = c.max_m < 0 ? batch : c.max_m;
  const int N = c.max_n < 0 ? batch : c.max_n;
  bool ni1 = (MODE == 2) && M <= 64, nj1 = N <= 64;   // narrow tiles for narrow outputs
  if (MODE != 2) {
    // few 128-row tiles (small batches): 64-row tiles double the workgroup count (2 fit per CU at 128x128, 4 at 64x128)
    const long long wgs = (long long)cdiv(M, 128) * cdiv(N, nj1 ? 64 : 128) * c.count;
    if (wgs < knobs().fwd_small_wgs) ni1 = true;
    // still under two workgroups per CU: halve the per-wave work once more.  Forward GEMMs switch below 1024 workgroups
    // (measured at B = 8192: the integration forward on 512 64x64 tiles instead of 256 64x128 tiles, step -30 us); the
    // dgrads measured no different and keep the round-1 threshold.
    if (ni1 && !nj1 && (long long)cdiv(M, 64) * cdiv(N, 128) * c.count < (MODE == 0 ? knobs().fwd_narrow_wgs : 128)) nj1 = true;
  }
  if (MODE == 2) wgrad_tile_rule(M, N, nsplit, c.count, &ni1, &nj1);
  if constexpr (MODE != 2) {
    // one large group in whole 128 x 128 x 32 tiles: global memory -> registers -> matrix cores (dib_gemm_stream.h; bit-identical
    // outputs).  host_groups: this call's group as the host sees it.
    const auto [went, rc] = try_gemm_stream<MODE>(dev_groups + c.first, host_groups, c, A, B, C, bias, aux, batch, act, st);
    if (went) return rc;
  }
  if constexpr (MODE == 2) {
    // 128-wide row-major operands in whole K-tiles: global memory -> registers -> matrix cores, one 128 x 128 (128 x 64) tile per
    // wave (dib_wgrad_stream.h; bit-identical slabs).  host_groups: this call's groups (c.first .. + count) as the host sees them.
    WgradStreamPlan sp;
    if (wgrad_stream_plan(host_groups, c, A, B, batch, nsplit, rows_per_split, auto_split, max_splits, &sp)) {
      const int ns = sp.nsplit, rps = sp.rows_per_split;
      if (ns_used) *ns_used = ns;
      if (sp.nt == 2) return launch_wgrad_stream<2, 4>(dev_groups, c, M, N, A, B, C, bias_out, batch, ns, rps, split_stride, st);
      return sp.ch == 4 ? launch_wgrad_stream<4, 4>(dev_groups, c, M, N, A, B, C, bias_out, batch, ns, rps, split_stride, st)
                        : launch_wgrad_stream<4, 2>(dev_groups, c, M, N, A, B, C, bias_out, batch, ns, rps, split_stride, st);
    }
  }
  if (MODE == 2 && auto_split && nsplit > 1 && knobs().split_policy) {
    // co-resident workgroups per CU of each tile shape (LDS / register budget of dib_gemm_kernel<2, NI, NJ, BK>)
    const int per_cu = (!ni1 && !nj1) ? 2 : ((!ni1 && nj1) ? 4 : (ni1 && !nj1) ? 3 : 4);
    const long long tiles = (long long)cdiv(M, ni1 ? 64 : 128) * cdiv(N, nj1 ? 64 : 128) * c.count;
    pick_wgrad_splits(tiles, split_rule_cus() * per_cu, batch, std::max(nsplit, max_splits), &nsplit, &rows_per_split);
    if (ns_used) *ns_used = nsplit;
  }
  ProfScope ps(MODE * 4 + (ni1 ? 0 : 2) + (nj1 ? 0 : 1), st);
  if constexpr (MODE == 2) {
    // a 32-row operand against a wide one (q / k / v weight gradients of the set transformer): the flat 32 x 256 tile
    if (M <= 32 && N >= 256 && knobs().wgrad_flat_tile)
      return launch_gemm_t<2, 1, 2, true>(dev_groups, c, M, N, A, B, C, bias, aux, bias_out, batch, act, nsplit, rows_per_split,
                                          split_stride, st);
  }
#define DIB_GO(NI, NJ) launch_gemm_t<MODE, NI, NJ>(dev_groups, c, M, N, A, B, C, bias, aux, bias_out, batch, act, nsplit, \
                                                   rows_per_split, split_stride, st)
  if (ni1) return nj1 ? DIB_GO(1, 1) : DIB_GO(1, 2);
  return nj1 ? DIB_GO(2, 1) : DIB_GO(2, 2);
#undef DIB_GO
}

__global__ void dib_write_desc_kernel(DibGemmGroup* dst, DibGemmGroup g) { *dst = g; }

// The reducers (dib_grads_finalize, the step tail) sum ALL the workspace's slabs of every parameter block, and a launch that
// chose `ns` splits writes slabs [0, ns) of its blocks: the slabs above stay as they are - zero since dib_workspace_init unless a
// DIFFERENT launch over the same block chose more splits earlier (the split rule prices whole launches: the row-tile regime's one
// grouped launch of all weight gradients picked 3 slabs at B = 512 where the per-layer launches of dib_integration_bwd /
// dib_encoder_bank_bwd - the custom-loss entry of a 1-unit output - picked 4, and a training step after a custom-loss step summed
// that step's fourth slab into its gradients).  Per (batch, block) the layout remembers the most slabs any launch has written;
// a launch that writes fewer zero-fills the difference behind itself.  Programs that stay on one path never pay; a program that
// alternates pays a few small memsets per step.  A launch being CAPTURED into a hipGraph cannot know what will run between its
// replays: it zero-fills every slab it does not write (slab_count = the slabs the workspace holds).
static int retire_stale_slabs(const dib_layout* l, int batch, const DibGemmGroup* host_groups, int count, int ns, int slab_count,
                              float* gt, long long split_stride, hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
  std::lock_guard<std::mutex> lk(l->wg_mu);
  for (int i = 0; i < count; ++i) {
    const DibGemmGroup& g = host_groups[i];
    int& mark = l->slab_hwm[std::make_pair(batch, g.c_off)];
    mark = std::max(mark, ns);
    const int hwm = capturing ? std::max(mark, slab_count) : mark;
    if (ns >= hwm) continue;
    const size_t wbytes = (size_t)g.M * (size_t)g.ldc * sizeof(float);   // the block's rows are contiguous (ldc == N)
    for (int s = ns; s < hwm; ++s) {
      hipError_t e = hipMemsetAsync(gt + (long long)s * split_stride + g.c_off, 0, wbytes, st);
      if (e == hipSuccess && g.bias_off >= 0)
        e = hipMemsetAsync(gt + (long long)s * split_stride + g.bias_off, 0, (size_t)g.N * sizeof(float), st);
      if (e != hipSuccess) return (int)e;
    }
  }
  return DIB_OK;
}

template <int MODE>
int launch_gemm(const dib_layout* l, const GemmCall& c, const float* A, const float* B, float* C, const float* bias,
                const float* aux, float* bias_out, int batch, int act, int nsplit, int rows_per_split,
                long long split_stride, hipStream_t st, int slab_count = 0) {
  // the layout's weight gradients contract over the batch: their split count is chosen per launch (pick_wgrad_splits) among
  // 1 .. slab_count (the partial slabs the workspace holds)
  int ns_used = nsplit;
  int rc = launch_gemm<MODE>(l->dev_groups, c, A, B, C, bias, aux, bias_out, batch, act, nsplit, rows_per_split, split_stride,
                             st, /*auto_split=*/MODE == 2, slab_count, &ns_used, l->table.data() + c.first);
  if (MODE == 2 && rc == DIB_OK && slab_count > 1)
    rc = retire_stale_slabs(l, batch, l->table.data() + c.first, c.count, ns_used, slab_count, C, split_stride, st);
  return rc;
}

}  // namespace

// groups [first, first + count) of the table (see dib_layout::wg_groups) into the gradient target gt
static int merged_wgrad(dib_layout* l, const dib_layout::WsMap& m, float* w, int batch, float* gt, int first, int count,
                        hipStream_t st) {
  if (count <= 0) return DIB_OK;
  const auto& host = wg_table_host(l, m, batch);
  GemmCall c;
  c.first = 0; c.count = count;
  for (int i = first; i < first + count; ++i) { c.max_m = std::max(c.max_m, host[i].M); c.max_n = std::max(c.max_n, host[i].N); }
  const DibGemmGroup* dev = reinterpret_cast<const DibGemmGroup*>(w + m.wg_table) + first;
  int ns_used = m.nsplit;
  int rc = launch_gemm<2>(dev, c, w, w, gt, nullptr, nullptr, gt, batch, 0, m.nsplit, m.rows_per_split, align_up(l->n_params, 4), st,
                          /*auto_split=*/true, m.nsplit, &ns_used, host.data() + first);
  if (rc == DIB_OK && m.nsplit > 1)
    rc = retire_stale_slabs(l, batch, host.data() + first, count, ns_used, m.nsplit, gt, align_up(l->n_params, 4), st);
  return rc;
}

extern "C" {

int dib_gemm(int mode, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
             const float* bias, const float* aux, int ldaux, int act, void* dev_desc, dib_stream_t stream) {
  if (!A || !B || !C || !dev_desc || M <= 0 || N <= 0 || K <= 0 || mode < 0 || mode > 2) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  DibGemmGroup g = make_group(Off(), lda, Off(), ldb, Off(), ldc, bias ? 0 : -1, Off(), ldaux, M, N, K);
  if ((((uintptr_t)A | (uintptr_t)B) & 15) != 0) return DIB_E_ARG;  // operands must be 16-byte aligned
  // descriptor travels BY VALUE in a kernel argument and is written on the stream (capture-safe: no host-memory copy node
  // pointing at this stack frame)
  DIB_LAUNCH(dib_write_desc_kernel, dim3(1), dim3(1), 0, st, (DibGemmGroup*)dev_desc, g);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  const int tm = cdiv(M, 128), tn = cdiv(N, 128);
  const DibGemmGroup* dg = (const DibGemmGroup*)dev_desc;
  if (mode != 2) {   // a large product in whole tiles: the LDS-free kernel (dib_gemm_stream.h), bit-identical outputs
    GemmCall c;
    c.first = 0; c.count = 1; c.max_m = M; c.max_n = N;
    const auto [went, rc] = mode == 0 ? try_gemm_stream<0>(dg, &g, c, A, B, C, bias, aux, 0, act, st)
                                      : try_gemm_stream<1>(dg, &g, c, A, B, C, bias, aux, 0, act, st);
    if (went) return rc;
  }
  ProfScope ps(mode * 4 + 3, st);
  const dim3 g1(8 * cdiv(tm, 8) * tn, 1, 1);
  if (mode == 0)
    DIB_LAUNCH((dib_gemm_kernel<0, 2, 2, 32>), g1, dim3(256), 0, st, dg, A, B, C, bias, aux, (float*)nullptr, 0,
                       act, tm, tn, 0, 0ll);
  else if (mode == 1)
    DIB_LAUNCH((dib_gemm_kernel<1, 2, 2, 32>), g1, dim3(256), 0, st, dg, A, B, C, bias, aux, (float*)nullptr, 0,
                       act, tm, tn, 0, 0ll);
  else  // single split over the whole contraction; bias (if given) receives the column sums of B
    DIB_LAUNCH((dib_gemm_kernel<2, 2, 2, 32>), dim3(1, tm * tn, 1), dim3(256), 0, st, dg, A, B, C,
                       (const float*)nullptr, aux, (float*)bias, 0, act, tm, tn, K, 0ll);
  return (int)hipGetLastError();
}

static_assert(sizeof(dib_gemm_desc) == sizeof(DibGemmGroup), "public descriptor must mirror the kernel's group struct");

int dib_gemm_grouped(int mode, int n_groups, const dib_gemm_desc* dev_desc, int max_m, int max_n, const float* A,
                     const float* B, float* C, const float* bias, const float* aux, float* bias_out, int act, int nsplit,
                     int rows_per_split, int64_t split_stride, dib_stream_t stream) {
  if (!dev_desc || !A || !B || !C || n_groups <= 0 || max_m <= 0 || max_n <= 0 || mode < 0 || mode > 2 || !act_ok(act))
    return DIB_E_ARG;
  if (mode == 2 && (nsplit <= 0 || rows_per_split <= 0)) return DIB_E_ARG;
  GemmCall c;
  c.first = 0; c.count = n_groups; c.max_m = max_m; c.max_n = max_n;
  const DibGemmGroup* g = reinterpret_cast<const DibGemmGroup*>(dev_desc);
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case 0: return launch_gemm<0>(g, c, A, B, C, bias, aux, nullptr, 0, act, 1, 0, 0, st);
    case 1: return launch_gemm<1>(g, c, A, B, C, nullptr, aux, nullptr, 0, act, 1, 0, 0, st);
    default: return launch_gemm<2>(g, c, A, B, C, nullptr, nullptr, bias_out, 0, 0, nsplit, rows_per_split,
                                   (long long)split_stride, st);
  }
}

int dib_wgrad_grouped(int n_groups, const dib_gemm_desc* dev_desc, const dib_gemm_desc* host_desc, int max_m, int max_n, int batch,
                      const float* A, const float* B, float* C, float* bias_out, int nsplit, int rows_per_split,
                      int64_t split_stride, dib_stream_t stream) {
  if (!dev_desc || !host_desc || !A || !B || !C || n_groups <= 0 || max_m <= 0 || max_n <= 0 || batch < 0 || nsplit <= 0 ||
      rows_per_split <= 0)
    return DIB_E_ARG;
  GemmCall c;
  c.first = 0; c.count = n_groups; c.max_m = max_m; c.max_n = max_n;
  return launch_gemm<2>(reinterpret_cast<const DibGemmGroup*>(dev_desc), c, A, B, C, nullptr, nullptr, bias_out, batch, 0, nsplit,
                        rows_per_split, (long long)split_stride, (hipStream_t)stream, false, 0, nullptr,
                        reinterpret_cast<const DibGemmGroup*>(host_desc));
}

int dib_gemm_skinny_k(int mode, int n_groups, const dib_gemm_desc* dev_desc, int M, int N, int K, const float* A,
                      const float* B, float* C, const float* bias, dib_stream_t stream) {
  if (!dev_desc || !A || !B || !C || n_groups <= 0 || M <= 0 || N <= 0 || K <= 0 || mode < 0 || mode > 1) return DIB_E_ARG;
  if (K > 32 || (K & 3) || (N & 31) || n_groups > 65535 || cdiv(N, 128) > 65535) return DIB_E_UNSUPPORTED;
  const DibGemmGroup* g = reinterpret_cast<const DibGemmGroup*>(dev_desc);
  // >= ~4096 workgroups of 4 independent waves (16 wave slots per CU), at most 8 row tiles of 64 per workgroup
  const int total_tiles = cdiv(M, 64), cn = cdiv(N, 128);
  int chunks = std::max(1, std::min(total_tiles, cdiv(4096, cn * n_groups)));
  int tiles = std::min(8, cdiv(total_tiles, chunks));
  chunks = cdiv(total_tiles, tiles);
  const int nt_store = (long long)M * N * (long long)sizeof(float) * n_groups >= (256ll << 20) ? 1 : 0;
  const dim3 grid(chunks, cn, n_groups);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    DIB_LAUNCH(dib_gemm_skinnyk_kernel<0>, grid, dim3(256), 0, st, g, A, B, C, bias, M, N, K, tiles, nt_store);
  else
    DIB_LAUNCH(dib_gemm_skinnyk_kernel<1>, grid, dim3(256), 0, st, g, A, B, C, (const float*)nullptr, M, N, K, tiles,
                       nt_store);
  return (int)hipGetLastError();
}

int dib_reduce_splits(const float* partial, int64_t n, int nsplit, int64_t stride, float* out, dib_stream_t stream) {
  if (!partial || !out || n <= 0 || nsplit <= 0 || (n & 3) || (stride & 3)) return DIB_E_ARG;
  DIB_LAUNCH(dib_reduce_splits_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, partial,
                     (long long)n, nsplit, (long long)stride, out, (const float*)nullptr);
  return (int)hipGetLastError();
}

int dib_reduce_splits_add(const float* partial, int64_t n, int nsplit, int64_t stride, float* out, dib_stream_t stream) {
  if (!partial || !out || n <= 0 || nsplit <= 0 || (n & 3) || (stride & 3)) return DIB_E_ARG;
  DIB_LAUNCH(dib_reduce_splits_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, partial,
                     (long long)n, nsplit, (long long)stride, out, (const float*)out);
  return (int)hipGetLastError();
}

}  // extern "C"
