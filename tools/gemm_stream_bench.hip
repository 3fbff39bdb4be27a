// gemm_stream_bench.hip - the LDS-free forward / dgrad kernel (csrc/dib_gemm_stream.h) beside the tiled one (csrc/dib_gemm.h) on
// the four integration-network launches of BASELINE config 3 (F = 64, B = 65536), same data, alternating launches.
// (tools only; not part of the product)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gemm_stream_bench.hip -o exp/gemm_stream_bench && exp/gemm_stream_bench
//
// Per shape: REPS alternating pairs of launches, each timed with HIP events; prints every time, min / median per arm, the
// fp32-MFMA rate, and whether the two kernels' outputs are equal bit for bit.  `exp/gemm_stream_bench B` runs another batch size (a multiple of 128).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../distributed-information-bottleneck.github.io_amd/csrc/dib_gemm_stream.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// relu: ReLU-ed values (many exact zeros, like u's neighbours a1 / a2); else values with a zeroed block (like a masked gradient)
__global__ void fill_kernel(float* p, size_t n, unsigned seed, int relu, float scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned s = (unsigned)i * 2654435761u + seed;
    s ^= s >> 15; s *= 2246822519u; s ^= s >> 13; s *= 3266489917u; s ^= s >> 16;
    float v = ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * 2.0f * scale;
    if (relu) v = v > 0.f ? v : 0.f;
    else if (((i >> 12) & 7) == 3) v = 0.f;
    p[i] = v;
  }
}

struct Shape { const char* name; int mode, N, K, bias, aux, act; };

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 65536, REPS = 7;
  if (B <= 0 || (B & 127)) { printf("batch must be a multiple of 128\n"); return 1; }
  const size_t n_wide = (size_t)B * 2048, n_w = (size_t)2048 * 256;
  float *A, *W, *X, *bias, *C[2];
  DibGemmGroup* dg;
  CK(hipMalloc(&A, n_wide * 4));
  CK(hipMalloc(&X, (size_t)B * 256 * 4));
  CK(hipMalloc(&W, n_w * 4));
  CK(hipMalloc(&bias, 256 * 4));
  for (int k = 0; k < 2; ++k) CK(hipMalloc(&C[k], n_wide * 4));
  CK(hipMalloc(&dg, sizeof(DibGemmGroup)));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, A, n_wide, 1u, 0, 1.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, X, (size_t)B * 256, 2u, 1, 1.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(256), dim3(256), 0, 0, W, n_w, 3u, 0, 0.05f);
  hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, 0, bias, (size_t)256, 4u, 0, 0.1f);
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  int cus = 256;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  // A is [B, K] with lda = K (the first B x K floats of the wide buffer)
  const Shape shapes[4] = {{"forward L1  u[B,2048] W1[2048,256] + b, relu  ", 0, 256, 2048, 1, 0, 1},
                           {"forward L2  a1[B,256] W2[256,256] + b, relu   ", 0, 256, 256, 1, 0, 1},
                           {"dgrad L2    (g_a2[B,256] W2^T) * relu'(a1)    ", 1, 256, 256, 0, 1, 1},
                           {"dgrad L1    g_a1[B,256] W1[2048,256]^T        ", 1, 2048, 256, 0, 0, 0}};
  std::vector<float> h0, h1;
  for (const Shape& s : shapes) {
    DibGemmGroup g;
    std::memset(&g, 0, sizeof(g));
    g.bias_off = s.bias ? 0 : -1;
    g.M = B; g.N = s.N; g.K = s.K; g.lda = s.K; g.ldb = s.mode == 0 ? s.N : s.K; g.ldc = s.N; g.ldaux = s.N;
    if ((size_t)B * s.K > n_wide || (size_t)B * s.N > n_wide || (size_t)s.N * s.K > n_w || (s.aux && s.N != 256) || (s.bias && s.N > 256) ||
        (s.N & 127) || (s.K & 31)) { printf("bad shape\n"); return 1; }
    CK(hipMemcpy(dg, &g, sizeof(g), hipMemcpyHostToDevice));
    const size_t n_out = (size_t)B * s.N;
    for (int k = 0; k < 2; ++k) CK(hipMemset(C[k], 0xFF, n_out * 4));
    const int tm = B / 128, tn = s.N / 128;
    const bool big_out = n_out * 4 >= ((size_t)256 << 20);
    const float* bp = s.bias ? bias : nullptr;
    const float* xp = s.aux ? X : nullptr;
    const int nwaves = std::min(tm * tn, 4 * cus);
    const dim3 sgrid((nwaves + 3) / 4);
    auto tiled = [&]() {
      const dim3 grid(8 * ((tm + 7) / 8) * tn);
      if (s.mode == 0)
        hipLaunchKernelGGL((dib_gemm_kernel<0, 2, 2, 64>), grid, dim3(256), 0, 0, dg, A, W, C[0], bp, xp, (float*)nullptr, B, s.act, tm, tn, 0,
                           0ll, big_out ? 3 : 1);
      else
        hipLaunchKernelGGL((dib_gemm_kernel<1, 2, 2, 64>), grid, dim3(256), 0, 0, dg, A, W, C[0], bp, xp, (float*)nullptr, B, s.act, tm, tn, 0,
                           0ll, big_out ? 3 : 1);
    };
#define GS_GO(MODE, KIND) hipLaunchKernelGGL((dib_gemm_stream_kernel<MODE, KIND>), sgrid, dim3(256), 0, 0, dg, A, W, C[1], bp, xp, B, s.act, tm, tn, \
                                             nwaves, big_out ? 1 : 0)
    auto stream = [&]() {
      if (s.mode == 0) GS_GO(0, 1);
      else if (s.aux) GS_GO(1, 3);
      else GS_GO(1, 0);
    };
#undef GS_GO
    tiled();
    stream();
    CK(hipDeviceSynchronize());   // a fault in either kernel ends the program here
    h0.resize(n_out);
    h1.resize(n_out);
    CK(hipMemcpy(h0.data(), C[0], n_out * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h1.data(), C[1], n_out * 4, hipMemcpyDeviceToHost));
    size_t diff = 0, first = 0;
    for (size_t i = 0; i < n_out; ++i)
      if (std::memcmp(&h0[i], &h1[i], 4) != 0) { if (!diff) first = i; ++diff; }
    std::vector<float> t[2];
    for (int rep = 0; rep < REPS; ++rep) {
      for (int arm = 0; arm < 2; ++arm) {
        CK(hipEventRecord(e0, 0));
        if (arm == 0) tiled(); else stream();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        t[arm].push_back(ms);
      }
    }
    const double tf = 2.0 * (double)B * s.N * s.K / 1e9;   // GFLOP -> TFLOP/s = tf / ms
    printf("%s B = %d, %d waves\n  bit-identical: %s", s.name, B, nwaves, diff ? "NO" : "yes");
    if (diff) printf(" (%zu words differ, first at %zu: %g vs %g)", diff, first, h0[first], h1[first]);
    const char* names[2] = {"tiled ", "stream"};
    for (int arm = 0; arm < 2; ++arm) {
      printf("\n  %s ms:", names[arm]);
      for (float v : t[arm]) printf(" %.4f", v);
    }
    printf("\n");
    for (int arm = 0; arm < 2; ++arm) {
      std::sort(t[arm].begin(), t[arm].end());
      printf("  %s min %.4f median %.4f max %.4f  (%.1f TFLOP/s at the median)\n", names[arm], t[arm].front(), t[arm][REPS / 2], t[arm].back(),
             tf / t[arm][REPS / 2]);
    }
    fflush(stdout);
  }
  return 0;
}
