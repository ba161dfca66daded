// Stand-in for <hip/hip_runtime.h> when common.h is compiled with g++ -DFMI_HOST_THREADS (tests/test_host_mask_detector_train.py): the HIP
// execution model for kernels with workgroup reductions -- one OS thread per work-item, a pthread barrier for __syncthreads, __shfl_xor
// through a shared slot array, workgroups run one after another, `__shared__` = static.  It defines the runtime's names only; the
// reduction helpers and launch-size functions are common.h's own.  Test infrastructure: far too slow for anything but small cases.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct float4 { float x, y, z, w; };
struct longlong2 { long long x, y; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
// the separately rounded fp32 operations (build without -ffast-math / FMA contraction, as the tests do)
static inline float __fmul_rn(float a, float b) { return a * b; }
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static dim3 gridDim, blockDim;
static pthread_barrier_t g_bar;
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
template <class T>
static inline T __shfl_xor(T v, int off, int) {
  static T slots[1024];
  slots[threadIdx.x] = v;
  __syncthreads();
  T r = slots[threadIdx.x ^ off];
  __syncthreads();
  return r;
}
typedef int hipError_t;
static const hipError_t hipSuccess = 0;
static inline hipError_t hipGetLastError() { return hipSuccess; }
template <class K, class... A>
static void emu_launch(K k, dim3 g, dim3 b, A... a) {
  gridDim = g;
  blockDim = b;
  pthread_barrier_init(&g_bar, nullptr, b.x);
  for (unsigned by = 0; by < g.y; ++by)
    for (unsigned bx = 0; bx < g.x; ++bx) {
      std::vector<std::thread> ts;
      for (unsigned t = 0; t < b.x; ++t)
        ts.emplace_back([=] {
          threadIdx = dim3(t);
          blockIdx = dim3(bx, by);
          k(a...);
        });
      for (auto& th : ts) th.join();
    }
  pthread_barrier_destroy(&g_bar);
}
#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...) emu_launch(kern, grid, block, __VA_ARGS__)
