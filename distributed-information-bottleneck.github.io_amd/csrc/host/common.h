// host/common.h - what every host fragment of dib_api.hip shares: the launch counter and the launch helper for kernels with
// dynamic LDS, constants, the optional live kernel timing, the tuning table (dib_set_tuning) and the device's CU count.

// every kernel launch of the library goes through this macro: dib_launch_count() reports how many a step issues (bench.py).
// Relaxed atomic: entry points may run on several host threads at once (include/dib_hip.h "Threads").
static std::atomic<unsigned long long> g_dib_launches{0};
#define DIB_LAUNCH(...) do { g_dib_launches.fetch_add(1, std::memory_order_relaxed); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

namespace {

constexpr int64_t kAlign = 64;  // floats (256 B)
constexpr int kMaxSplits = 32;   // partial slabs of a split-batch weight gradient
// Row-tile kernels of dib_small.h: hard limits (they size workspace regions); WHICH batches take them is the "small_wgs" rule
constexpr int kSmallMaxBatch = 2048;     // rows
constexpr int kSmallMaxEncWgs = 1024;    // row tiles x features (d(W1|b1) partials: one [16][H1] block per encoder workgroup)
constexpr size_t kSmallMaxLds = 160 * 1024;   // LDS one workgroup of a row-tile kernel may have (gfx950: the CU's 160 KB)
// dynamic LDS up to which a shape is ADMITTED to the integration and chain kernels: 10 KB below the CU's LDS, headroom for the
// kernels' static __shared__ words and for regions a kernel gains later - an admitted shape must never become a refused launch
constexpr size_t kSmallAdmitLds = 150 * 1024;
constexpr int kSplitRows = 512;  // minimum batch rows per wgrad split: 8 K-tiles of 64 (measured: 2048 left mid-size batches with 16-256 workgroups)
inline int64_t align_up(int64_t v, int64_t a = kAlign) { return (v + a - 1) / a * a; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline int grid_for(int64_t n, int per_block = 256, int cap = 256 * 16) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, cap));
}

// ---- optional live kernel timing (bench.py roofline): HIP events around every launch, on the launch stream ----
// categories = kernel symbols: 0..11 dib_gemm_kernel<MODE,NI,NJ> at MODE*4 + (NI-1)*2 + (NJ-1); 12 fused encoder fwd;
// 13 fused encoder bwd; 14 every other (HBM-bound) kernel; 15 dib_attn_fwd_kernel; 16 dib_attn_bwd_kernel;
// 17 / 18 dib_wgrad_stream_kernel on 128- / 64-column tiles (dib_profile_summary_n only: dib_profile_summary's arrays hold 17);
// dib_wgrad_h1_kernel (dib_wgrad_recompute.h) is timed in 17 with the kernel it stands in for, and entry 19 of
// dib_profile_summary_n reports which of 17's spans were its launches; dib_gemm_stream_kernel<0 / 1> (dib_gemm_stream.h) likewise is
// timed in 3 / 7 with the 128 x 128 tiled kernel it stands in for, and entries 20 / 21 report which of those spans were its launches
constexpr int kProfCats = 19;
constexpr int kProfWgradH1Part = 19;
constexpr int kProfGemmStreamPart = 20;   // + MODE
constexpr int kProfFusedFwd = 12, kProfFusedBwd = 13, kProfOther = 14, kProfAttnFwd = 15, kProfAttnBwd = 16;
constexpr int kProfWgradStream128 = 17, kProfWgradStream64 = 18;
// which kernel a span of category 17 / 3 / 7 timed: the category's own, or the one standing in for it (entries 19 / 20 / 21)
enum ProfPart : unsigned char { kPartNone, kPartWgradH1, kPartGemmStreamFwd, kPartGemmStreamDgrad };
struct ProfSpan { hipEvent_t a, b; ProfPart part; };
struct Prof {   // diagnostics (bench.py roofline): the tables are guarded, so a second thread's launches are recorded, not racy
  std::atomic<bool> on{false};
  std::mutex mu;
  std::vector<hipEvent_t> pool;                     // recycled events
  std::vector<ProfSpan> spans[kProfCats];
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
} g_prof;

struct ProfScope {
  int cat; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
  ProfPart part;
  ProfScope(int c, hipStream_t s, ProfPart p = kPartNone) : cat(c), st(s), part(p) {
    // the small HBM-bound kernels are not bracketed (event pairs serialise kernel boundaries: ~10 us each); rocprofv3
    // reports them (profiles/*_kernel_stats.csv)
    if (g_prof.on.load(std::memory_order_relaxed) && cat != 14) {
      { std::lock_guard<std::mutex> lk(g_prof.mu); a = g_prof.get(); b = g_prof.get(); }
      (void)hipEventRecord(a, st);
    }
  }
  ~ProfScope() {
    if (a) {
      (void)hipEventRecord(b, st);
      std::lock_guard<std::mutex> lk(g_prof.mu);
      g_prof.spans[cat].push_back({a, b, part});
    }
  }
};

const char* kVersion = "dib_hip 0.4 (gfx950: fused encoder-bank fwd/bwd + grouped fp32-MFMA GEMM + flash attention)";

int act_ok(int a) { return a >= 0 && a <= 7; }

// Tile / split rules.  The defaults are the measured choices; dib_set_tuning (include/dib_hip.h) is the ONE documented way to
// change them (A/B measurements, tools/ab_bench.sh) - the library reads no environment variable.
struct Tuning {
  int fwd_small_wgs = 512;   // forward/dgrad: below this many 128-row workgroups use 64-row tiles
  int fwd_narrow_wgs = 1024; // forward: below this many 64x128 workgroups use 64x64 tiles (round 3: 512 -> 1024, the set
                             // transformer's q/k/v projection at 1600 tokens: step 1.99 -> 1.87 ms; profiles/r03l_forward_tile_rule.txt)
  int stream_rows = 8192;    // GEMMs with at least this many streamed rows load / store them non-temporally (1 << 30: never)
  int split_policy = 1;      // weight gradients of the layout: 1 = pick the batch-split count per launch so that the workgroups
                             // fill whole rounds of the chip's workgroup slots (pick_wgrad_splits); 0 = the layout-wide count
  int split_overhead = 128;  // ... with this per-workgroup fixed cost, in batch rows (prologue + partial-tile store)
  int fused_encoder = 1;     // layouts created from now on may use the fused encoder-bank kernels (0: grouped-GEMM path)
  int fused_head = 1;        // dib_output_head_fused_supported may answer 1
  int small_batch = 1;       // row-tile kernels (csrc/dib_small.h) where the layout allows, while ...
  int small_wgs = 512;       // ... (row tiles of 16) x (features) <= this (and batch <= 2048)
  int mlp_row_tiles = 1;     // ... and for a plain MLP (dib_mlp_small_*: the custom loop's output encoder)
  int infonce_one_launch = 1; // dib_infonce_fwd_bwd at B <= 128, D <= 64 (dot-product similarities): one launch instead of three
  int attn_small_bwd_waves = 8;  // dib_attention_bwd for <= 64 particles: 8 waves (two per SIMD) or the 4-wave kernel
  int wgrad_flat_tile = 1;   // weight gradients with <= 32 rows and >= 256 columns on the 32 x 256 tile (0: 64 x 128, A/B)
  int wgrad_stream = 1;      // weight gradients of 128-wide row-major operands in whole K-tiles on the LDS-free kernel
                             // (dib_wgrad_stream.h; 0: the tiled kernel - bit-identical slabs) from ...
  int wgrad_stream_rows = 8192;  // ... this many streamed rows up, when its wave-tiles (128 x 128 output tile x slab) fill ...
  int wgrad_stream_fill = 85;    // ... this many percent of the chip's wave slots (four per CU) at least
  int gemm_stream = 1;       // forward / dgrad GEMMs of one group with M % 128 == 0, N % 128 == 0, K % 32 == 0 and a linear / relu / leaky
                             // activation on the LDS-free kernel (dib_gemm_stream.h; 0: the tiled kernel - bit-identical outputs) from ...
  int gemm_stream_rows = 8192;   // ... this many rows (M) up, when its wave-tiles (128 x 128 output tiles) fill ...
  int gemm_stream_fill = 85;     // ... this many percent of the chip's wave slots (four per CU) at least
  int wgrad_recompute_h1 = 1;    // fused encoder + that kernel for the layer-2 weight gradient + inputs <= 8 wide: the forward does not
                                 // stash h1, the weight gradient recomputes it in registers (dib_wgrad_recompute.h; 0: stash and
                                 // stream it - bit-identical gradients).  Read at the FORWARD; the backward follows its record
  int attn_fwd_waves = 8;    // dib_attention_fwd for P >= 256: 8-wave workgroups of 256 queries sharing one staged K / V tile (4: the 4-wave
                             // kernel, which shorter sets always take; bit-identical outputs)
  int int_cluster_short_exchange = 1;  // clusters on one XCD exchange through that XCD's L2 (0: always the agent-scope protocol - the
                             // path a cluster takes when it is NOT on one XCD; tests)
  int int_cluster = 8;       // row-tile integration kernel: workgroups per row tile (each a column slice of every layer, exchange
                             // through L2: dib_small.h "cluster mode"; <= 1: one per tile) while row tiles x this <= ...
  int int_cluster_wgs = 256; // ... this (one workgroup per CU; 8 per tile up to 32 row tiles, 4 up to 64: profiles/r06u_int_cluster_sweep.txt) and
  int int_cluster_min_weights = 65536;  // ... the network's hidden layers have at least this many weights (measured down to 4
                             // features x 32 -> 256 -> 256: 98 304)
  int wgrad_max_splits = 32; // most batch slabs of a layout's weight gradients (<= 32; read when a workspace is sized: set it first)
  int subset_low_bits = 0;   // dib_subset_information: low key bits a workgroup folds in LDS (0: the most that fits; include/dib_subsets.h)
  int num_cus = 0;           // compute units the split rule prices rounds with; 0 = the current device's own count (device_cus)
};
// Process-wide and written ONLY by dib_set_tuning, which the header documents as a configuration call made while no other
// entry point is running; every other entry point only reads it.
inline Tuning& tuning() { static Tuning t; return t; }
inline const Tuning& knobs() { return tuning(); }
inline int wgrad_max_splits() { return std::max(1, std::min(32, knobs().wgrad_max_splits)); }   // dib_set_tuning("wgrad_max_splits")
// compute units of the CURRENT device, queried once per device ordinal (no process-wide "the device": one process may drive
// several GPUs from several threads)
inline int device_cus() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cus[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
  cus[dev].store(v, std::memory_order_relaxed);
  return v;
}
inline int split_rule_cus() { return knobs().num_cus > 0 ? knobs().num_cus : device_cus(); }

// ---- kernels with dynamic LDS --------------------------------------------------------------------------------------------
// A launch with more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize raised first.  The attribute
// belongs to the KERNEL FUNCTION on one device, so what has been granted is remembered per kernel - one instantiation of this
// template per kernel, however many call sites launch it - and per device ordinal (two engines on two GPUs in one process are
// allowed).  It only ever goes up: to what a launch needs, when that exceeds what is recorded.  Two host threads may reach the
// same first launch together (include/dib_hip.h "Threads"): the steady state is one acquire load, the slow path is serialised,
// and the new size is published only after the attribute call succeeded - a failure returns its error and records nothing.
std::mutex g_attr_mu;
template <auto* Kernel>
int raise_dynamic_lds(size_t bytes) {
  if (bytes <= 64 * 1024) return DIB_OK;
  static std::atomic<size_t> granted[64];
  int dev = 0;
  std::atomic<size_t>* slot = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 ? &granted[dev] : nullptr;   // else: uncached
  if (slot && slot->load(std::memory_order_acquire) >= bytes) return DIB_OK;
  std::lock_guard<std::mutex> lk(g_attr_mu);
  if (slot && slot->load(std::memory_order_relaxed) >= bytes) return DIB_OK;
  hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return (int)e;
  if (slot) slot->store(bytes, std::memory_order_release);
  return DIB_OK;
}
// ... and the launch itself: launch_lds<&kernel>(grid, block, lds bytes, stream, kernel arguments...)
template <auto* Kernel, typename... Args>
int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
  if (int rc = raise_dynamic_lds<Kernel>(lds)) return rc;
  DIB_LAUNCH(Kernel, grid, block, lds, st, std::forward<Args>(args)...);
  return (int)hipGetLastError();
}

// ---- tuning: the one documented switchboard (no environment variables) -------------------------------------------
static int* tuning_slot(const char* key) {
  Tuning& t = tuning();
  if (!key) return nullptr;
  if (!std::strcmp(key, "fwd_small_wgs")) return &t.fwd_small_wgs;
  if (!std::strcmp(key, "fwd_narrow_wgs")) return &t.fwd_narrow_wgs;
  if (!std::strcmp(key, "stream_rows")) return &t.stream_rows;
  if (!std::strcmp(key, "split_policy")) return &t.split_policy;
  if (!std::strcmp(key, "split_overhead")) return &t.split_overhead;
  if (!std::strcmp(key, "fused_encoder")) return &t.fused_encoder;
  if (!std::strcmp(key, "fused_head")) return &t.fused_head;
  if (!std::strcmp(key, "small_batch")) return &t.small_batch;
  if (!std::strcmp(key, "small_wgs")) return &t.small_wgs;
  if (!std::strcmp(key, "mlp_row_tiles")) return &t.mlp_row_tiles;
  if (!std::strcmp(key, "infonce_one_launch")) return &t.infonce_one_launch;
  if (!std::strcmp(key, "attn_small_bwd_waves")) return &t.attn_small_bwd_waves;
  if (!std::strcmp(key, "wgrad_flat_tile")) return &t.wgrad_flat_tile;
  if (!std::strcmp(key, "wgrad_stream")) return &t.wgrad_stream;
  if (!std::strcmp(key, "wgrad_stream_rows")) return &t.wgrad_stream_rows;
  if (!std::strcmp(key, "wgrad_stream_fill")) return &t.wgrad_stream_fill;
  if (!std::strcmp(key, "gemm_stream")) return &t.gemm_stream;
  if (!std::strcmp(key, "gemm_stream_rows")) return &t.gemm_stream_rows;
  if (!std::strcmp(key, "gemm_stream_fill")) return &t.gemm_stream_fill;
  if (!std::strcmp(key, "wgrad_recompute_h1")) return &t.wgrad_recompute_h1;
  if (!std::strcmp(key, "wgrad_max_splits")) return &t.wgrad_max_splits;
  if (!std::strcmp(key, "num_cus")) return &t.num_cus;
  if (!std::strcmp(key, "subset_low_bits")) return &t.subset_low_bits;
  if (!std::strcmp(key, "attn_fwd_waves")) return &t.attn_fwd_waves;
  if (!std::strcmp(key, "int_cluster_short_exchange")) return &t.int_cluster_short_exchange;
  if (!std::strcmp(key, "int_cluster")) return &t.int_cluster;
  if (!std::strcmp(key, "int_cluster_wgs")) return &t.int_cluster_wgs;
  if (!std::strcmp(key, "int_cluster_min_weights")) return &t.int_cluster_min_weights;
  return nullptr;
}

}  // namespace

extern "C" {

const char* dib_version(void) { return kVersion; }
int dib_abi_version(void) { return DIB_ABI_VERSION; }

const char* dib_error_string(int code) {
  switch (code) {
    case DIB_OK: return "ok";
    case DIB_E_ARG: return "invalid argument";
    case DIB_E_SHAPE: return "shape mismatch";
    case DIB_E_WORKSPACE: return "workspace / descriptor tables missing";
    case DIB_E_UNSUPPORTED: return "unsupported configuration";
    case DIB_E_NODEVICE: return "no HIP device";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown dib error";
  }
}

int dib_set_tuning(const char* key, int value) {
  int* p = tuning_slot(key);
  if (!p || value < 0) return DIB_E_ARG;
  *p = value;
  return DIB_OK;
}

int dib_get_tuning(const char* key, int* value) {
  const int* p = tuning_slot(key);
  if (!p || !value) return DIB_E_ARG;
  *value = *p;
  return DIB_OK;
}

int64_t dib_launch_count(void) { return (int64_t)g_dib_launches.load(std::memory_order_relaxed); }

int dib_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  for (int c = 0; c < kProfCats; ++c) {
    for (auto& sp : g_prof.spans[c]) { g_prof.pool.push_back(sp.a); g_prof.pool.push_back(sp.b); }
    g_prof.spans[c].clear();
  }
  g_prof.on = on != 0;
  return DIB_OK;
}

int dib_profile_summary_n(double* ms_by_category, int* launches_by_category, int n) {
  if (!ms_by_category || !launches_by_category || n < 0) return DIB_E_ARG;
  std::lock_guard<std::mutex> lk(g_prof.mu);
  for (int c = 0; c < std::min(n, kProfCats); ++c) {
    double tot = 0.0;
    for (auto& sp : g_prof.spans[c]) {
      hipError_t e = hipEventSynchronize(sp.b);
      if (e != hipSuccess) return (int)e;
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, sp.a, sp.b);
      if (e != hipSuccess) return (int)e;
      tot += ms;
    }
    ms_by_category[c] = tot;
    launches_by_category[c] = (int)g_prof.spans[c].size();
  }
  for (int c = kProfCats; c < n; ++c) { ms_by_category[c] = 0.0; launches_by_category[c] = 0; }
  // the parts of categories 17 / 3 / 7 that ran dib_wgrad_h1_kernel / dib_gemm_stream_kernel<0> / <1>
  static constexpr struct { int entry, cat; ProfPart part; } kParts[] = {{kProfWgradH1Part, kProfWgradStream128, kPartWgradH1},
                                                                         {kProfGemmStreamPart, 3, kPartGemmStreamFwd},
                                                                         {kProfGemmStreamPart + 1, 7, kPartGemmStreamDgrad}};
  for (const auto& p : kParts) {
    if (n <= p.entry) continue;
    double tot = 0.0;
    int launches = 0;
    for (const auto& sp : g_prof.spans[p.cat]) {
      if (sp.part != p.part) continue;
      float ms = 0.f;   // (synchronised above)
      hipError_t e = hipEventElapsedTime(&ms, sp.a, sp.b);
      if (e != hipSuccess) return (int)e;
      tot += ms;
      ++launches;
    }
    ms_by_category[p.entry] = tot;
    launches_by_category[p.entry] = launches;
  }
  return DIB_OK;
}

int dib_profile_summary(double* ms_by_category, int* launches_by_category) {
  return dib_profile_summary_n(ms_by_category, launches_by_category, DIB_PROFILE_CATEGORIES);
}

}  // extern "C"
