// The partial-row reductions of the per-channel kernels (chan.hip, sg2_bf16.hip, norm.hip): a pass stores every block's sums as one row
// of a workspace, sum_parts_kernel adds the rows afterwards -- deterministic, and nothing has to be zeroed.  Thousands of fp32 atomics
// on a few hundred addresses serialise in L2 instead (measured: 0.2 ms per launch for 2048 blocks x 128 channels, 4x the streaming
// time of the pass itself).  Several files include this header: everything is forceinline, static or in the anonymous namespace.
#pragma once
#include "common.h"
#ifndef FMI_HOST_EMU

namespace {

// 256 threads = (256 / C8) rows x C8 eight-channel chunks per pass; the threads that own one chunk are combined through LDS and the
// block's sums are stored as row `dst` of the workspace.
__device__ __forceinline__ void chunk_reduce_store(float (&acc)[8], float* __restrict__ dst /*[C]*/, int C8, float (*part)[8]) {
  const int RL = 256 / C8, cg = threadIdx.x % C8;
#pragma unroll
  for (int e = 0; e < 8; ++e) part[threadIdx.x][e] = acc[e];
  __syncthreads();
  if ((int)threadIdx.x < C8) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = part[threadIdx.x][e];
    for (int l = 1; l < RL; ++l)
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += part[l * C8 + cg][e];
    *reinterpret_cast<float4*>(dst + 8 * cg) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<float4*>(dst + 8 * cg + 4) = make_float4(t[4], t[5], t[6], t[7]);
  }
  __syncthreads();
}
// out[g][i] = sum_{p < nparts} ws[(g * nparts + p) * width + i], g = blockIdx.y; T = float or double.
// 64 columns x 16 row lanes per workgroup, eight independent loads in flight per thread, the lanes' sums added in a fixed order (one
// thread per column walking up to 1024 rows with four accumulators was a latency chain: 18 - 37 us per launch, 200 launches per pSp step)
template <typename T>
__global__ void __launch_bounds__(1024) sum_parts_kernel(const T* __restrict__ ws, T* __restrict__ out, int nparts, int width) {
  __shared__ T part[16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  const T* p = ws + (int64_t)blockIdx.y * nparts * width + i;
  T a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (i < width) {
    int q = ty;
    for (; q + 7 * 16 < nparts; q += 8 * 16) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += p[(int64_t)(q + 16 * u) * width];
    }
    for (; q < nparts; q += 16) a[0] += p[(int64_t)q * width];
  }
  part[ty][tx] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (ty == 0 && i < width) {
    T t = 0;
#pragma unroll
    for (int l = 0; l < 16; ++l) t += part[l][tx];
    out[(int64_t)blockIdx.y * width + i] = t;
  }
}
template <typename T>
void launch_sum_parts(const T* ws, T* out, int nparts, int width, int64_t groups, hipStream_t st) {
  hipLaunchKernelGGL(sum_parts_kernel<T>, dim3((unsigned)((width + 63) / 64), (unsigned)groups), dim3(1024), 0, st, ws, out, nparts, width);
}
// how many row blocks a reduction pass uses: enough to fill the chip, at most what the workspace holds (width floats per block)
inline int64_t parts_for(int64_t rows, int64_t groups, int64_t width, int64_t ws_floats) {
  int64_t b = ceil_div64(rows, 64);
  const int64_t want = ceil_div64(2048, groups);
  if (b > want) b = want;
  const int64_t fit = ws_floats / (groups * width);
  if (b > fit) b = fit;
  return b;
}
inline bool c8_ok(int C) {
  const int c8 = C / 8;
  return C % 8 == 0 && c8 >= 1 && c8 <= 256 && (c8 & (c8 - 1)) == 0;
}

}  // namespace
#endif
