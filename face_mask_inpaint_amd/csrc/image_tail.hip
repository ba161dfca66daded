// The image tail of pSp inference: everything between the decoder's NHWC fp32 image and what the harness consumes, from ONE read of
// the image -- AdaptiveAvgPool2d((256, 256)) (psp.py:33,113-114), the (x + 1) / 2 operand of SSIM / MS-SSIM (psp_inference.py:116-117)
// and tensor2im's uint8 HWC picture (psp_inference.py:106-112, gradio_serve.py:45-51).  Bandwidth kernels: no LDS, no atomics.
#include "common.h"

namespace {

// tensor2im in its literal order, every step a separately rounded fp32 operation (no FMA contraction), as numpy evaluates it:
// t = (v + shift) * scale; t[t < 0] = 0; t[t > 1] = 1; (t * 255).astype(uint8).  NaN (outside the contract) -> 0.
__device__ __forceinline__ uint32_t to_u8(float v, float shift, float scale) {
  float t = __fmul_rn(__fadd_rn(v, shift), scale);
  t = t < 0.f ? 0.f : t;
  t = t > 1.f ? 1.f : t;
  t = __fmul_rn(t, 255.f);
  return t == t ? (uint32_t)(int)t : 0u;
}

// One thread = four neighbouring output pixels of one output row: F input rows of 4 F pixels x RGB = 3 F float4 each, contiguous and
// 16-byte aligned.  Every output value is summed row-major over its F x F window and multiplied by 1 / F^2 once (a power of two:
// exact), so the result does not depend on the launch shape.  Stores: one float4 per channel plane, 12 bytes of HWC uint8.
template <int F>
__global__ void __launch_bounds__(64) image_tail_kernel(const float4* __restrict__ x, float* __restrict__ pooled, float* __restrict__ unit,
                                                        uint8_t* __restrict__ u8, float shift, float scale, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;  // (n, oy, ox / 4)
  if (i >= total) return;
  const int q = (int)(i & 63), oy = (int)((i >> 6) & 255);
  const int64_t n = i >> 14;
  constexpr int ROW4 = 256 * F * 3 / 4;  // float4 per input row
  const float4* src = x + ((n * 256 + oy) * F) * (int64_t)ROW4 + q * (3 * F);
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
#pragma unroll
  for (int a = 0; a < F; ++a) {
    float v[12 * F];
#pragma unroll
    for (int j = 0; j < 3 * F; ++j) {
      const float4 t = src[a * ROW4 + j];
      v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int b = 0; b < F; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[p * 3 + c] = __fadd_rn(acc[p * 3 + c], v[(p * F + b) * 3 + c]);
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = __fmul_rn(acc[k], 1.f / (float)(F * F));
  const int64_t plane = ((n * 3) * 256 + oy) * 256 + q * 4;  // channel 0 of this sample; channel c is 65 536 floats further
  if (pooled) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(pooled + plane + c * 65536) = make_float4(acc[c], acc[3 + c], acc[6 + c], acc[9 + c]);
  }
  if (unit) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(unit + plane + c * 65536) =
          make_float4(__fmul_rn(__fadd_rn(acc[c], 1.f), 0.5f), __fmul_rn(__fadd_rn(acc[3 + c], 1.f), 0.5f), __fmul_rn(__fadd_rn(acc[6 + c], 1.f), 0.5f),
                      __fmul_rn(__fadd_rn(acc[9 + c], 1.f), 0.5f));
  }
  if (u8) {
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      w[k] = to_u8(acc[4 * k], shift, scale) | (to_u8(acc[4 * k + 1], shift, scale) << 8) | (to_u8(acc[4 * k + 2], shift, scale) << 16) |
             (to_u8(acc[4 * k + 3], shift, scale) << 24);
    uint32_t* dst = reinterpret_cast<uint32_t*>(u8 + ((n * 256 + oy) * 256 + q * 4) * 3);
    dst[0] = w[0], dst[1] = w[1], dst[2] = w[2];
  }
}

// planes [N][C][H][W] (C = 3, or C = 1 replicated into the three channels) -> uint8 HWC [N][H][W][3].  VEC: four pixels per thread
// (needs H * W % 4 == 0 and aligned bases); otherwise one pixel per thread.
template <bool VEC>
__global__ void __launch_bounds__(256) planes_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ u8, int C, int64_t hw, float shift,
                                                           float scale, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  if (VEC) {
    const int64_t per = hw >> 2, n = i / per, p = (i - n * per) << 2;
    float v[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 t = *reinterpret_cast<const float4*>(x + (n * C + (C == 3 ? c : 0)) * hw + p);
      v[c] = t.x, v[3 + c] = t.y, v[6 + c] = t.z, v[9 + c] = t.w;
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(u8 + (n * hw + p) * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      dst[k] = to_u8(v[4 * k], shift, scale) | (to_u8(v[4 * k + 1], shift, scale) << 8) | (to_u8(v[4 * k + 2], shift, scale) << 16) |
               (to_u8(v[4 * k + 3], shift, scale) << 24);
  } else {
    const int64_t n = i / hw, p = i - n * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) u8[i * 3 + c] = (uint8_t)to_u8(x[(n * C + (C == 3 ? c : 0)) * hw + p], shift, scale);
  }
}

}  // namespace

static inline bool host_al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int fmi_image_tail_f32(const float* x, float* pooled, float* unit, uint8_t* u8, int N, int S, float shift, float scale, void* stream) {
  if (!x || (!pooled && !unit && !u8) || N <= 0) return FMI_ERR_BAD_ARG;
  if (S != 256 && S != 512 && S != 1024) return FMI_ERR_UNSUPPORTED;
  if (!host_al(x, 16) || !host_al(pooled, 16) || !host_al(unit, 16) || !host_al(u8, 4)) return FMI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * 256 * 64;
  const dim3 grid((unsigned)(total / 64)), block(64);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  if (S == 256)
    hipLaunchKernelGGL(image_tail_kernel<1>, grid, block, 0, (hipStream_t)stream, x4, pooled, unit, u8, shift, scale, total);
  else if (S == 512)
    hipLaunchKernelGGL(image_tail_kernel<2>, grid, block, 0, (hipStream_t)stream, x4, pooled, unit, u8, shift, scale, total);
  else
    hipLaunchKernelGGL(image_tail_kernel<4>, grid, block, 0, (hipStream_t)stream, x4, pooled, unit, u8, shift, scale, total);
  return fmi_launch_status();
}

extern "C" int fmi_planes_to_u8_f32(const float* x, uint8_t* u8, int N, int C, int H, int W, float shift, float scale, void* stream) {
  if (!x || !u8 || N <= 0 || H <= 0 || W <= 0) return FMI_ERR_BAD_ARG;
  if (C != 1 && C != 3) return FMI_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)H * W;
  const bool vec = hw % 4 == 0 && host_al(x, 16) && host_al(u8, 4);
  const int64_t total = vec ? (int64_t)N * (hw / 4) : (int64_t)N * hw;
  const dim3 grid((unsigned)ceil_div64(total, 256)), block(256);
  if (vec)
    hipLaunchKernelGGL(planes_to_u8_kernel<true>, grid, block, 0, (hipStream_t)stream, x, u8, C, hw, shift, scale, total);
  else
    hipLaunchKernelGGL(planes_to_u8_kernel<false>, grid, block, 0, (hipStream_t)stream, x, u8, C, hw, shift, scale, total);
  return fmi_launch_status();
}
