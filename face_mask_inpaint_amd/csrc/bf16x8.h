// Eight bf16 values (16 bytes, raw bits) <-> eight floats: the unit the element-wise bf16 kernels of the IR-SE body move per thread
// (enc_bf16.hip, irse_infer_bf16.hip).  Round to nearest even; inputs are finite.
#pragma once
#include "common.h"

typedef uint16_t bf16_t;
__device__ __forceinline__ float e_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float e_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ uint32_t e_pack(float a, float b) {  // round to nearest even
  uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
  ua += 0x7fffu + ((ua >> 16) & 1u);
  ub += 0x7fffu + ((ub >> 16) & 1u);
  return (ua >> 16) | (ub & 0xffff0000u);
}
__device__ __forceinline__ void e_unpack8(const uint4& v, float (&f)[8]) {
  f[0] = e_lo(v.x), f[1] = e_hi(v.x), f[2] = e_lo(v.y), f[3] = e_hi(v.y);
  f[4] = e_lo(v.z), f[5] = e_hi(v.z), f[6] = e_lo(v.w), f[7] = e_hi(v.w);
}
__device__ __forceinline__ uint4 e_pack8(const float (&f)[8]) {
  return make_uint4(e_pack(f[0], f[1]), e_pack(f[2], f[3]), e_pack(f[4], f[5]), e_pack(f[6], f[7]));
}
__device__ __forceinline__ void e_load8f(const float* p, float (&f)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}
static bool e_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
