// wgrad_stream_bench.hip - the LDS-free weight-gradient kernel (csrc/dib_wgrad_stream.h) beside the tiled one (csrc/dib_gemm.h)
// on the three large weight gradients of BASELINE config 3 (F = 64, B = 65536), same data, alternating launches.
// (tools only; not part of the product)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/wgrad_stream_bench.hip -o exp/wgrad_stream_bench && exp/wgrad_stream_bench
//
// Per shape: REPS alternating pairs of launches, each timed with HIP events; prints every time, min / median per arm, the
// fp32-MFMA rate, and whether the two kernels' slab buffers (weights and bias rows) are equal bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../distributed-information-bottleneck.github.io_amd/csrc/dib_wgrad_stream.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// A: ReLU-ed values (many exact zeros, like h1 / h2); B: values with a zeroed block (like a masked gradient)
__global__ void fill_kernel(float* p, size_t n, unsigned seed, int relu) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned s = (unsigned)i * 2654435761u + seed;
    s ^= s >> 15; s *= 2246822519u; s ^= s >> 13; s *= 3266489917u; s ^= s >> 16;
    float v = ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * 2.0f;
    if (relu) v = v > 0.f ? v : 0.f;
    else if (((i >> 12) & 7) == 3) v = 0.f;
    p[i] = v;
  }
}

struct Shape { const char* name; int groups, M, N, ns, rps; };

int main() {
  const int F = 64, B = 65536, REPS = 7;
  const size_t n_op = (size_t)F * B * 128;
  const long long stride = (long long)F * (128 * 128 + 128);
  const int max_ns = 32;
  float *A, *Bm, *C0, *C1;
  DibGemmGroup* dg;
  CK(hipMalloc(&A, n_op * 4));
  CK(hipMalloc(&Bm, n_op * 4));
  CK(hipMalloc(&C0, (size_t)max_ns * stride * 4));
  CK(hipMalloc(&C1, (size_t)max_ns * stride * 4));
  CK(hipMalloc(&dg, F * sizeof(DibGemmGroup)));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, A, n_op, 1u, 1);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, Bm, n_op, 2u, 0);
  CK(hipDeviceSynchronize());
  CK(hipFuncSetAttribute((const void*)dib_wgrad_stream_kernel<2, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const Shape shapes[3] = {{"encoder layer 2  64 x [65536,128]^T[65536,128]", 64, 128, 128, 32, 2048},
                           {"encoder layer 3  64 x [65536,128]^T[65536,64] ", 64, 128, 64, 16, 4096},
                           {"integration 1    [65536,2048]^T[65536,256]     ", 1, 2048, 256, 32, 2048}};
  std::vector<float> h0((size_t)max_ns * stride), h1((size_t)max_ns * stride);
  for (const Shape& s : shapes) {
    std::vector<DibGemmGroup> hg(s.groups);
    for (int f = 0; f < s.groups; ++f) {
      DibGemmGroup g;
      std::memset(&g, 0, sizeof(g));
      g.a_off = (long long)f * B * s.M; g.b_off = (long long)f * B * s.N;
      g.c_off = (long long)f * ((long long)s.M * s.N + s.N); g.bias_off = g.c_off + (long long)s.M * s.N;
      g.M = s.M; g.N = s.N; g.K = B; g.lda = s.M; g.ldb = s.N; g.ldc = s.N;
      hg[f] = g;
    }
    // every slab this shape writes lies inside the C buffers (max_ns x stride floats)
    if ((long long)s.groups * ((long long)s.M * s.N + s.N) > stride || s.ns > max_ns || (long long)s.ns * s.rps != B ||
        (size_t)s.groups * B * s.M > n_op || (size_t)s.groups * B * s.N > n_op) { printf("bad shape\n"); return 1; }
    CK(hipMemcpy(dg, hg.data(), s.groups * sizeof(DibGemmGroup), hipMemcpyHostToDevice));
    CK(hipMemset(C0, 0xFF, (size_t)max_ns * stride * 4));
    CK(hipMemset(C1, 0xFF, (size_t)max_ns * stride * 4));
    const int tm = s.M / 128, tn = (s.N + 127) / 128;
    auto tiled = [&]() {
      if (s.N == 64)
        hipLaunchKernelGGL((dib_gemm_kernel<2, 2, 1, 32>), dim3(s.ns, tm, s.groups), dim3(256), 0, 0, dg, A, Bm, C0, nullptr, nullptr,
                           C0, B, 0, tm, 1, s.rps, stride, 1);
      else
        hipLaunchKernelGGL((dib_gemm_kernel<2, 2, 2, 64>), dim3(s.ns, tm * tn, s.groups), dim3(256), 0, 0, dg, A, Bm, C0, nullptr,
                           nullptr, C0, B, 0, tm, tn, s.rps, stride, 1);
    };
    // lds: dynamic LDS bytes nobody uses - above half a CU's 160 KB they keep a second workgroup off the CU (the 64-column
    // kernel's registers would let two waves share a SIMD)
    auto stream = [&](size_t lds = 0) {
      const int waves = tm * tn * s.groups * s.ns;
      if (s.N == 64)
        hipLaunchKernelGGL((dib_wgrad_stream_kernel<2, 4, true>), dim3((waves + 3) / 4), dim3(256), lds, 0, dg, A, Bm, C1, C1, B,
                           s.groups, tm, 1, s.ns, s.rps, stride);
      else
        hipLaunchKernelGGL((dib_wgrad_stream_kernel<4, 2, true>), dim3((waves + 3) / 4), dim3(256), 0, 0, dg, A, Bm, C1, C1, B,
                           s.groups, tm, tn, s.ns, s.rps, stride);
    };
    tiled();
    stream();
    CK(hipDeviceSynchronize());   // a fault in either kernel ends the program here
    CK(hipMemcpy(h0.data(), C0, h0.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h1.data(), C1, h1.size() * 4, hipMemcpyDeviceToHost));
    size_t diff = 0, first = 0;
    for (size_t i = 0; i < h0.size(); ++i)
      if (std::memcmp(&h0[i], &h1[i], 4) != 0) { if (!diff) first = i; ++diff; }
    std::vector<float> t0, t1, t2;
    const int arms = s.N == 64 ? 3 : 2;
    for (int rep = 0; rep < REPS; ++rep) {
      for (int arm = 0; arm < arms; ++arm) {
        CK(hipEventRecord(e0, 0));
        if (arm == 0) tiled(); else if (arm == 1) stream(); else stream(96 * 1024);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        (arm == 0 ? t0 : arm == 1 ? t1 : t2).push_back(ms);
      }
    }
    const double tf = 2.0 * s.groups * (double)s.M * s.N * B / 1e9;   // GFLOP -> TFLOP/s = tf / ms
    printf("%s  bit-identical: %s", s.name, diff ? "NO" : "yes");
    if (diff) printf(" (%zu words differ, first at %zu: %g vs %g)", diff, first, h0[first], h1[first]);
    printf("\n  tiled  ms:");
    for (float v : t0) printf(" %.4f", v);
    printf("\n  stream ms:");
    for (float v : t1) printf(" %.4f", v);
    if (arms == 3) {
      printf("\n  stream, one workgroup per CU ms:");
      for (float v : t2) printf(" %.4f", v);
    }
    std::sort(t0.begin(), t0.end());
    std::sort(t1.begin(), t1.end());
    printf("\n  tiled  min %.4f median %.4f max %.4f  (%.1f TFLOP/s at the median)\n", t0.front(), t0[REPS / 2], t0.back(), tf / t0[REPS / 2]);
    printf("  stream min %.4f median %.4f max %.4f  (%.1f TFLOP/s at the median)\n", t1.front(), t1[REPS / 2], t1.back(), tf / t1[REPS / 2]);
    fflush(stdout);
  }
  return 0;
}
