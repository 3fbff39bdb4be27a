// host/mi_features.h - every feature's sandwich bounds in one evaluation (include/dib_mi_features.h; csrc/dib_mi_features.h):
// the third tiled family on host/mi.h's workspace layout (TiledWs), with a split rule of its own.

struct MifPlan {
  int G = 0, tiles = 0, npad = 0, S = 1, rps = 0, rb = 0, emax = 0;
  size_t lds = 0;
  TiledWs ws;
};

// grid and workspace of one dib_mif_bounds_kernel launch; DIB_OK or the code every entry point returns
static int mif_plan(int F, int E, int n, int nb, MifPlan& p) {
  if (F <= 0 || E <= 0 || n <= 0 || nb <= 0) return DIB_E_ARG;
  if (E > 256 || (E > 64 && (E & 3)) || n < 2 || n > 16384 || (int64_t)F * nb > 65535) return DIB_E_UNSUPPORTED;
  p.G = F * nb;
  p.npad = (n + 63) / 64 * 64;
  p.tiles = p.npad / 64;
  p.emax = E <= 32 ? 32 : (E <= 64 ? 64 : 0);
  p.rb = p.emax ? (E <= 32 ? 64 : 32) : (E <= 128 ? 16 : 4);
  const int pitch = p.emax ? (E + 7) & ~7 : E;   // registers: staged rows are padded to blocks of 8 dimensions
  // at most 37 376 B with the sample in registers; E = 256 in LDS: 4 staged rows + the tile's samples = 151 584 B < the CU's 160 KB
  p.lds = (size_t)p.rb * pitch * 16 + (size_t)p.rb * 8 + (p.emax ? 0 : (size_t)64 * E * 8) + 4 * 64 * 16;
  // row splits: a function of n and NOT of F or nb (nor of the device), so that a group's merge order - its bits - is the same
  // whichever groups share the launch.  Every workgroup draws its 64 samples before its first row (Philox + 32 float64 exps and
  // divisions per lane, in each of the four waves): with 256 rows per split - what the sibling families take for a lone group -
  // that prologue is paid four times per tile at n = 1024 (512 groups of 1024 rows, E = 32: 4.51 ms split in four, 4.05 ms
  // unsplit), so a split keeps >= 1024 rows and a group of up to 2047 rows is one split; an evaluation has F x nb groups to
  // fill the chip with
  const int S = std::max(1, n / 1024);
  p.rps = (n + S - 1) / S;
  p.S = (n + p.rps - 1) / p.rps;
  p.ws = tiled_ws((int64_t)p.G * n, E, p.S, p.G, p.npad);
  return DIB_OK;
}

extern "C" {

int dib_mi_features_supported(int F, int E, int n, int nb) {
  MifPlan p;
  return mif_plan(F, E, n, nb, p) == DIB_OK ? 1 : 0;
}

int64_t dib_mi_features_workspace_bytes(int F, int E, int n, int nb) {
  MifPlan p;
  if (int rc = mif_plan(F, E, n, nb, p)) return rc;
  return p.ws.bytes;
}

int dib_mi_features_bounds(const float* enc, int64_t plane_rows, int64_t row0, int F, int E, int n, int nb, uint64_t seed,
                           uint32_t step0, uint32_t feature0, double* out, double* lower_rows, double* upper_rows, double* u_out,
                           void* ws, dib_stream_t stream) {
  MifPlan p;
  if (int rc = mif_plan(F, E, n, nb, p)) return rc;
  if (!enc || !out || !ws || ((uintptr_t)ws & 15)) return DIB_E_ARG;
  if (plane_rows <= 0 || row0 < 0 || row0 + (int64_t)nb * n > plane_rows) return DIB_E_ARG;
  if ((lower_rows == nullptr) != (upper_rows == nullptr)) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* w = (double*)ws;
  DibMifArgs a;
  std::memset(&a, 0, sizeof(a));
  a.enc = enc; a.tab = (const double2*)w; a.tab_c = w + p.ws.off_c; a.part = (double2*)(w + p.ws.off_part);
  a.lii = w + p.ws.off_own; a.u_out = u_out; a.seed = (unsigned long long)seed; a.plane_rows = plane_rows; a.row0 = row0;
  a.step0 = step0; a.feature0 = feature0;
  a.E = E; a.n = n; a.nb = nb; a.G = p.G; a.S = p.S; a.npad = p.npad; a.rps = p.rps; a.rb = p.rb;
  DIB_LAUNCH(dib_mif_table_kernel, dim3(cdiv((int64_t)p.G * n, 256)), dim3(256), 0, st, a, (double2*)w, w + p.ws.off_c);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  const dim3 grid(p.tiles, p.G, p.S);
  if (p.emax == 32) {
    DIB_LAUNCH(dib_mif_bounds_kernel<32>, grid, dim3(DIB_MIF_THREADS), p.lds, st, a);
  } else if (p.emax == 64) {
    DIB_LAUNCH(dib_mif_bounds_kernel<64>, grid, dim3(DIB_MIF_THREADS), p.lds, st, a);
  } else if (int rc = launch_lds<&dib_mif_bounds_kernel<0>>(grid, dim3(DIB_MIF_THREADS), p.lds, st, a)) {
    return rc;
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  DIB_LAUNCH(dib_mif_combine_kernel, dim3(p.G), dim3(256), 0, st, a, out, lower_rows, upper_rows);
  return (int)hipGetLastError();
}

}  // extern "C"
