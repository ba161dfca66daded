// The stride-1 ResBlock's `conv3x3(x1, W1) + conv1x1(x2, W2)` as ONE reduction (forward) and ONE walk over dy (weight gradient).
//
// Forward: after the 9 * C1 (tap, channel) steps of x1 the k-loop goes on over the C2 channels of x2 at the centre tap, with the second
// weight pack; accumulators and epilogue are shared.  Weight gradient: the A operand gets C2 more rows after the 9 * C1 (tap, channel) rows,
// gathered from x2 at the anchor pixel itself, then the row of ones (the gradient of BOTH biases); the epilogue writes the row ranges to two
// packs.  The second source lives in loader / epilogue types of its own, so the single-source kernels stay the instantiations they were.
// Geometry everywhere: 3x3, stride 1, pad 1, zero padding, so anchor index == pixel index of x2 ([N][H][W] flattened, pitch cs2).
#pragma once
#include "gemm_core.h"

struct ConvK2 {  // A operand: ConvK over x1 for k < K1 = 9 * C1, then x2[anchor][k - K1]
  static constexpr bool KMODE = true;
  ConvK a;
  const float* p2;
  int C2, cs2, K1;
  using Ctx = ConvK::Ctx;
  __device__ __forceinline__ void set_batch(int) {}  // shared weights only
  __device__ __forceinline__ Ctx prep(int x) const { return a.prep(x); }
  __device__ __forceinline__ float4 load4(const Ctx& c, int x, int k) const {
    if (k < K1) return a.load4(c, x, k);
    if (c.rn < 0 || k - K1 >= C2) return zero4();
    return ldg4(p2 + (int64_t)x * cs2 + (k - K1));
  }
  __host__ __device__ __forceinline__ bool dma_ok() const { return a.dma_ok() && (C2 & 15) == 0 && (cs2 & 3) == 0 && ((uintptr_t)p2 & 15) == 0; }
  struct DCtx {
    ConvK::DCtx d;
    int64_t boff2;  // element offset of (anchor pixel, channel kq) in x2
  };
  struct Tile {
    ConvK::Tile t;
    int off2;  // first channel of the tile in x2; -1: the tile lies in x1
  };
  __device__ __forceinline__ DCtx dprep(int x, int kq) const { return DCtx{a.dprep(x, kq), (int64_t)x * cs2 + kq}; }
  __device__ __forceinline__ Tile tile(int k0) const {
    if (k0 < K1) return Tile{a.tile(k0), -1};
    Tile t{};
    t.off2 = k0 - K1;
    return t;
  }
  __device__ __forceinline__ const float* chunk(const DCtx& d, const Tile& t) const {
    if (t.off2 < 0) return a.chunk(d.d, t.t);
    return (d.d.ry > -0x10000000 && t.off2 < C2) ? p2 + d.boff2 + t.off2 : nullptr;  // rows beyond M carry ry far outside the image
  }
  __device__ __forceinline__ void dstart(DCtx&, int) const {}
  __device__ __forceinline__ void advance(DCtx&) const {}
};

struct ConvWX2 {  // B operand: ConvWX over [9][C1][Nout] for k < K1, then the 1x1 pack [C2][Nout]
  static constexpr bool KMODE = false;
  static constexpr bool SPLIT3 = false;
  ConvWX a;
  const float* p2;
  int C2, K1;
  struct Ctx {};
  __device__ __forceinline__ void set_batch(int) {}
  __device__ __forceinline__ Ctx prep(int) const { return Ctx{}; }
  __device__ __forceinline__ float4 load4(const Ctx&, int x, int k) const {
    if (k < K1) return a.load4(ConvWX::Ctx{}, x, k);
    if (k - K1 >= C2 || x >= a.Nout) return zero4();
    const float* q = p2 + (int64_t)(k - K1) * a.Nout + x;
    if (a.vec && x + 3 < a.Nout) return ldg4(q);
    float4 r = zero4();
    r.x = q[0];
    if (x + 1 < a.Nout) r.y = q[1];
    if (x + 2 < a.Nout) r.z = q[2];
    if (x + 3 < a.Nout) r.w = q[3];
    return r;
  }
  __host__ __device__ __forceinline__ bool dma_ok() const { return a.dma_ok() && (C2 & 15) == 0 && ((uintptr_t)p2 & 15) == 0; }
  using DCtx = ConvWX::DCtx;
  using Tile = ConvWX::Tile;
  __device__ __forceinline__ DCtx dprep(int x, int kr) const { return a.dprep(x, kr); }
  __device__ __forceinline__ Tile tile(int k0) const {
    if (k0 < K1) return a.tile(k0);
    return Tile{k0 - K1 < C2 ? p2 + (int64_t)(k0 - K1) * a.Nout : nullptr};
  }
  __device__ __forceinline__ const float* chunk(const DCtx& d, const Tile& t) const { return a.chunk(d, t); }
  __device__ __forceinline__ void dstart(DCtx&, int) const {}
  __device__ __forceinline__ void advance(DCtx&) const {}
};

#ifndef FMI_HOST_EMU
struct ConvWX32 {  // B operand from bf16 piece images: ConvWX3 over [3][9][C1 / 8][Nout][8] for k < K1, then [3][1][C2 / 8][Nout][8]
  static constexpr bool KMODE = false;
  static constexpr bool SPLIT3 = true;
  ConvWX3 a;
  const uint16_t* p32;
  int C2, K1;
  struct Ctx {};
  __device__ __forceinline__ void set_batch(int) {}
  __device__ __forceinline__ Ctx prep(int) const { return Ctx{}; }
  __device__ __forceinline__ float4 load4(const Ctx&, int x, int k) const {  // register-staged path (debugging): the exact sum of the pieces
    if (k < K1) return a.load4(ConvWX3::Ctx{}, x, k);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int c = k - K1;
    const int64_t ps = (int64_t)C2 * a.Nout;
    if (c < C2)
      for (int e = 0; e < 4; ++e) {
        if (x + e >= a.Nout) break;
        const uint16_t* q = p32 + ((int64_t)(c >> 3) * a.Nout + x + e) * 8 + (c & 7);
        v[e] = (__uint_as_float((uint32_t)q[2 * ps] << 16) + __uint_as_float((uint32_t)q[ps] << 16)) + __uint_as_float((uint32_t)q[0] << 16);
      }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
  __host__ __device__ __forceinline__ bool dma_ok() const { return a.dma_ok() && (C2 & 15) == 0 && ((uintptr_t)p32 & 15) == 0; }
  struct DCtx {
    int64_t off, off2;  // chunk offset inside the first / the second piece images, -1 for columns beyond Nout
  };
  struct Tile {
    const uint16_t* base;
    bool second;
  };
  __device__ __forceinline__ DCtx dprep3(int piece, int kg, int x) const {
    if (x >= a.Nout) return DCtx{-1, -1};
    const int64_t o = ((int64_t)kg * a.Nout + x) * 8;
    return DCtx{piece * a.pstride + o, piece * ((int64_t)C2 * a.Nout) + o};
  }
  __device__ __forceinline__ Tile tile(int k0) const {
    if (k0 < K1) return Tile{a.tile(k0).base, false};
    return Tile{k0 - K1 < C2 ? p32 + ((int64_t)(k0 - K1) >> 3) * a.Nout * 8 : nullptr, true};
  }
  __device__ __forceinline__ const void* chunk(const DCtx& d, const Tile& t) const {
    return (d.off >= 0 && t.base) ? (const void*)(t.base + (t.second ? d.off2 : d.off)) : nullptr;
  }
};
#endif

// epilogue of the pair's forward: ConvEp with the second bias added in front of it (mask is null in a forward, so the order of ConvEp's own
// steps -- bias, residual, activation -- is kept); the split-reduction mode (act == 3) only adds partial sums
struct ConvEp2 : ConvEp {
  const float* bias2 = nullptr;
  __device__ __forceinline__ void store4(int64_t off, int col, float4 v) const {
    if (bias2) {
      const float4 b4 = *reinterpret_cast<const float4*>(bias2 + col);
      v.x += b4.x, v.y += b4.y, v.z += b4.z, v.w += b4.w;
    }
    ConvEp::store4(off, col, v);
  }
  __device__ __forceinline__ void store(int64_t off, int col, float v) const {
    if (bias2 && act != 3) v += bias2[col];
    ConvEp::store(off, col, v);
  }
};

struct WgradAX2 {  // A operand of the pair's weight gradient: rows [0, R1) = WgradAX over x1, [R1, R1 + C2) = x2's channels, then the ones row
  static constexpr bool KMODE = false;
  WgradAX a;  // a.ones_row = -1: the row of ones is placed here
  const float* p2;
  int C2, cs2, R1, ones_row;  // R1 = 9 * C1; ones_row = R1 + C2, or -1 without a bias gradient
  using Ctx = WgradAX::Ctx;
  __device__ __forceinline__ void set_batch(int) {}
  __device__ __forceinline__ Ctx prep(int x) const { return a.prep(x); }
  __device__ __forceinline__ float4 load4(const Ctx& cx, int x, int k) const {
    if (x < R1) return a.load4(cx, x, k);
    if (k >= a.g.Mdim()) return zero4();
    if (x >= R1 + C2) return x == ones_row ? make_float4(1.f, 0.f, 0.f, 0.f) : zero4();
    return ldg4(p2 + (int64_t)k * cs2 + (x - R1));
  }
  __host__ __device__ __forceinline__ bool dma_ok() const { return a.dma_ok() && (C2 & 3) == 0 && (cs2 & 3) == 0 && ((uintptr_t)p2 & 15) == 0; }
  using DCtx = WgradAX::DCtx;
  using Tile = WgradAX::Tile;
  __device__ __forceinline__ void dstart(DCtx& d, int k_begin) const { a.dstart(d, k_begin); }
  __device__ __forceinline__ void advance(DCtx& d) const { a.advance(d); }
  __device__ __forceinline__ DCtx dprep(int x, int kr) const { return a.dprep(x, kr); }
  __device__ __forceinline__ Tile tile(int k0) const { return Tile{k0}; }
#ifndef FMI_HOST_EMU
  __device__ __forceinline__ const float* chunk(const DCtx& d, const Tile& t) const {
    if (d.x < R1) return a.chunk(d, t);
    if (d.k >= a.g.Mdim()) return nullptr;
    if (d.x >= R1 + C2) return d.x == ones_row ? fmi_chunk_one : nullptr;
    return p2 + (int64_t)d.k * cs2 + (d.x - R1);
  }
#endif
};

struct WgradEp2 {  // rows [0, R1) -> dw1 in WgradEp's layout, [R1, R1 + C2) -> dw2[(row - R1) * K + col], the ones row -> dbias
  static constexpr bool HAS_VEC4 = false;
  WgradEp a;
  float* dw2;
  int R1;
  __device__ __forceinline__ void set_batch(int) {}
  __device__ __forceinline__ int64_t row_off(int row) const {
    if (row < R1) return a.row_off(row);
    if (row == a.ones_row) return -1;
    return -2 - (int64_t)(row - R1) * a.Kout;
  }
  __device__ __forceinline__ void store(int64_t off, int col, float v) const {
    if (off >= 0) atomicAdd(a.dw + off + col, v);
    else if (off == -1) atomicAdd(a.dbias + col, v);
    else atomicAdd(dw2 + (-2 - off) + col, v);
  }
};
