// Shared helpers for the gfx950 kernels of libfmi_hip.so.
#pragma once
#include <stdint.h>
#include "../../include/fmi_hip.h"

// may p be accessed 16 bytes at a time?  The launchers' test for the vector form of a kernel
static inline bool fmi_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#ifdef FMI_HOST_EMU
// CPU emulation build (tests/test_host_geometry.py): the operand loaders and epilogues of gemm_core.h are
// compiled with g++ and driven by a plain triple loop, so that every piece of index algebra of the implicit
// GEMM (taps, sub-pixel phases, reflect padding, packed weight rows, output mapping, fast division) is
// checked on the CPU.  Only the MFMA tile loop itself is GPU-only.
#include <math.h>
#include <string.h>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
struct float4 {
  float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline void atomicAdd(float* p, float v) { *p += v; }
typedef void* hipStream_t;
static inline int fmi_launch_status() { return FMI_OK; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool fmi_det() { return false; }          // the launch-decomposition switches have no meaning in the emulation

#else  // ------------------------------- device build -------------------------------
#ifdef FMI_HOST_THREADS
// The same branch compiled with g++ for kernels that FMI_HOST_EMU's single-threaded loops cannot drive -- workgroup reductions with
// wave shuffles, LDS and __syncthreads (csrc/segloss.hip; tests/test_host_mask_detector_train.py): host_threads.h stands in for the HIP
// runtime header only (one OS thread per work-item), so every helper below is the one the device build uses.
#include "host_threads.h"
#else
#include <hip/hip_runtime.h>

// Launch of a kernel that carves more than 64 KB of dynamic LDS.  That much must be opted into per kernel AND per device
// (hipFuncSetAttribute acts on the current device's code object): one atomic flag per (kernel instantiation, device ordinal), safe from
// the forward and the autograd thread alike.  FMI_ERR_LAUNCH if the opt-in fails; the launch itself is checked by fmi_launch_status().
struct fmi_attr_flags {
  unsigned char done[64];
};
static inline bool fmi_attr_needed(fmi_attr_flags& f, int& dev) {
  dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
  return !__atomic_load_n(&f.done[dev], __ATOMIC_ACQUIRE);
}
static inline void fmi_attr_mark(fmi_attr_flags& f, int dev) {
  if (dev >= 0 && dev < 64) __atomic_store_n(&f.done[dev], (unsigned char)1, __ATOMIC_RELEASE);
}
template <auto Kernel>
static fmi_attr_flags fmi_attr_flags_of{};
template <auto Kernel, class... A>
static int fmi_launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t st, A... args) {
  int dev;
  if (fmi_attr_needed(fmi_attr_flags_of<Kernel>, dev)) {
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) return FMI_ERR_LAUNCH;
    fmi_attr_mark(fmi_attr_flags_of<Kernel>, dev);
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
  return FMI_OK;
}
#endif
#include <stdlib.h>

#define FMI_WAVE 64

extern "C" int fmi_deterministic_flag;  // misc.hip: reproducible mode (single-contributor reductions), see fmi_set_deterministic
static inline bool fmi_det() { return fmi_deterministic_flag != 0; }

static inline int fmi_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? FMI_OK : FMI_ERR_LAUNCH;
}

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// thinin.hip: the streaming kernels behind fmi_conv2d_thin_input_dgrad_f32 (thinconv.hip), FMI_ERR_UNSUPPORTED for shapes they leave alone
int fmi_thin_in_dgrad_try(const fmi_conv_desc* d, const float* dy, const float* wt, float* dx, void* stream);

// grid size for grid-stride bandwidth kernels: enough workgroups to fill 256 CUs x 8, capped
static inline int fmi_bw_grid(int64_t work_items, int block) {
  int64_t g = ceil_div64(work_items, block);
  if (g < 1) g = 1;
  if (g > 256 * 16) g = 256 * 16;
  return (int)g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Block-wide reductions for 256-thread blocks (4 waves); result valid in every thread.
__device__ __forceinline__ float block_sum_256(float v, float* lds4) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[w] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}
__device__ __forceinline__ double block_sum_256_d(double v, double* lds4) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[w] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}
__device__ __forceinline__ float block_max_256(float v, float* lds4) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(lds4[0], lds4[1]), fmaxf(lds4[2], lds4[3]));
}

// Workgroups are dealt round-robin to the 8 XCDs (each with a private L2): hand every XCD a
// contiguous chunk of the logical tile order so that neighbouring tiles share an L2.
// Bijective for any nwg (guide: cdna_hip_programming.md, "XCD swizzle must be bijective").
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// ---- bilinear, align_corners=True (same source-index arithmetic as ATen's upsample_bilinear2d); pool.hip and ganhead.hip ----
struct Lerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lerp lerp_of(int o, int in, int out) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float r = scale * (float)o;
  Lerp l;
  l.i0 = (int)r;
  l.i1 = l.i0 + (l.i0 < in - 1 ? 1 : 0);
  l.l1 = r - (float)l.i0;
  l.l0 = 1.f - l.l1;
  return l;
}
// reproducible form of the adjoint: every INPUT pixel gathers from the output pixels whose interpolation footprint contains it, in a
// fixed order (gx is written, not accumulated).  Candidates: outputs around i / scale, tested with the forward's own lerp_of.
__device__ __forceinline__ void resize_cands(int i, int in, int out, int& lo, int& hi) {
  const float inv = in > 1 ? (float)(out - 1) / (float)(in - 1) : 0.f;
  lo = (int)((float)(i - 1) * inv) - 2;
  hi = (int)((float)(i + 1) * inv) + 2;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}
#endif
