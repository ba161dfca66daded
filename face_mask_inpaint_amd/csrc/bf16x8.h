// bf16 (raw bits in uint16_t) <-> fp32: the only home of the conversion in this library, and the 16-byte chunk the per-channel
// bandwidth kernels move per thread (chan.hip, irse_infer_bf16.hip, sg2_bf16.hip, unet_bf16.hip).
//
// Two roundings, and every store site names the one it uses:
//   bf_round      round to nearest even; the input is FINITE (a NaN whose low 16 bits carry may round to an infinity).  Kernels whose
//                 input is an activation this library produced itself.
//   bf_round_nan  a NaN is first made quiet and keeps its sign; everything else (infinities included) rounds as bf_round does.  Kernels that
//                 take a caller's tensor as it comes: fused_bias_act and upfirdn2d.
// bf_trunc2 does not round at all: for values that are bf16 already.  The three-way piece splits of x6.h / p3.hip / conv_p3.h are a
// different operation and live there.
#pragma once
#include "common.h"

typedef uint16_t bf16_t;

#ifndef FMI_HOST_EMU
// ---- widening (exact) ----
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }          // low half of a packed pair
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }  // high half
__device__ __forceinline__ float bf_widen(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// ---- narrowing ----
__device__ __forceinline__ uint32_t bf_round(float f) {  // the 16 bits, in the low half of a word
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ uint16_t bf_round_nan(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) u |= 0x00400000u;  // quiet NaN keeps its sign and payload
  else u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint32_t bf_pack2(float a, float b) {  // bf_round of both, a in the low half
  uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
  ua += 0x7fffu + ((ua >> 16) & 1u);
  ub += 0x7fffu + ((ub >> 16) & 1u);
  return (ua >> 16) | (ub & 0xffff0000u);
}
// bit patterns of two values that are bf16 already (a maximum, a routed gradient): truncation, no rounding step
__device__ __forceinline__ uint32_t bf_trunc2(float a, float b) { return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u); }
typedef __bf16 bf16x2h __attribute__((ext_vector_type(2)));
typedef float f32x2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bf_pack2_hw(float a, float b) {  // v_cvt_pk_bf16_f32: round to nearest even, one instruction
  const bf16x2h r = __builtin_convertvector((f32x2h){a, b}, bf16x2h);
  return *reinterpret_cast<const uint32_t*>(&r);
}
// ---- eight at a time ----
__device__ __forceinline__ void bf_unpack8(const uint4& v, float (&f)[8]) {
  f[0] = bf_lo(v.x), f[1] = bf_hi(v.x), f[2] = bf_lo(v.y), f[3] = bf_hi(v.y);
  f[4] = bf_lo(v.z), f[5] = bf_hi(v.z), f[6] = bf_lo(v.w), f[7] = bf_hi(v.w);
}
__device__ __forceinline__ uint4 bf_pack8(const float (&f)[8]) {
  return make_uint4(bf_pack2(f[0], f[1]), bf_pack2(f[2], f[3]), bf_pack2(f[4], f[5]), bf_pack2(f[6], f[7]));
}
__device__ __forceinline__ uint4 bf_pack8_hw(const float (&f)[8]) {
  return make_uint4(bf_pack2_hw(f[0], f[1]), bf_pack2_hw(f[2], f[3]), bf_pack2_hw(f[4], f[5]), bf_pack2_hw(f[6], f[7]));
}
__device__ __forceinline__ uint4 bf_trunc8(const float (&f)[8]) {
  return make_uint4(bf_trunc2(f[0], f[1]), bf_trunc2(f[2], f[3]), bf_trunc2(f[4], f[5]), bf_trunc2(f[6], f[7]));
}
// ---- one element of a tensor of either type (kernels templated on the element type) ----
__device__ __forceinline__ float bf_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float bf_ld(const uint16_t* p, int64_t i) { return bf_widen(p[i]); }
__device__ __forceinline__ void bf_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void bf_st(uint16_t* p, int64_t i, float v) { p[i] = (uint16_t)bf_round(v); }
__device__ __forceinline__ void bf_st_nan(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void bf_st_nan(uint16_t* p, int64_t i, float v) { p[i] = bf_round_nan(v); }

// ---- the 16 bytes one thread moves: N elements of T as one vector access, arithmetic on float[N] ----
template <typename T>
struct Chunk;
template <>
struct Chunk<float> {
  typedef float4 vec;
  static constexpr int N = 4;
  static __device__ __forceinline__ void widen(const vec& v, float (&f)[4]) { f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w; }
  static __device__ __forceinline__ vec narrow(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
  static __device__ __forceinline__ void loadf(const float* p, float (&f)[4]) { widen(*reinterpret_cast<const float4*>(p), f); }
};
template <>
struct Chunk<uint16_t> {
  typedef uint4 vec;
  static constexpr int N = 8;
  static __device__ __forceinline__ void widen(const vec& v, float (&f)[8]) { bf_unpack8(v, f); }
  static __device__ __forceinline__ vec narrow(const float (&f)[8]) { return bf_pack8(f); }  // bf_round
  static __device__ __forceinline__ void loadf(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
  }
};
__device__ __forceinline__ void bf_load8f(const float* p, float (&f)[8]) { Chunk<uint16_t>::loadf(p, f); }
#endif
