// fp32 VGG16 trunk of VGGLoss (modules/loss.py:33-65 of the reference): the passes at the points where the losses tap a feature map.
// NHWC fp32 maps, C % 4 == 0.  The activated map of a block's last convolution IS the tap (no copy); what is left around it is
//   forward : the 2 x 2 max pool that opens the next block and, where the next convolution reads them, the pooled map's bf16 pieces;
//   backward: dy = a > 0 ? (tap gradient + un-pooled gradient of the next block) : 0 and, where the adjoint reads them, dy's bf16 pieces
// -- each ONE pass instead of pool + split and cat + add + un-pool + ReLU mask + split.  One thread owns one 2 x 2 window of 4 (V = 1) or 8
// (V = 2: with pieces, a thread then writes whole 16-byte runs of the piece image) channels and moves 16 bytes per access.  Every value is
// what the composed kernels give, bit for bit: the pool is maxpool2_kernel's fmaxf chain, the winner maxpool2_bwd_kernel's first maximum
// in row-major order (strict >), the sum one fp32 add, the pieces split3_kernel's.  No atomics: both modes of fmi_set_deterministic run
// the same code.
#include "common.h"
#include "x6.h"

#define VT_MAX_SLICES 4

// pieces of the 8 channels (chunk i of the image, i = pixel * C / 8 + channel / 8), as split3_kernel writes them
__device__ __forceinline__ void vt_pieces(uint16_t* __restrict__ x3, int64_t i, const float4& a, const float4& b) {
  uint32_t w[3][4];
  split3_pair(a.x, a.y, w[0][0], w[1][0], w[2][0]);
  split3_pair(a.z, a.w, w[0][1], w[1][1], w[2][1]);
  split3_pair(b.x, b.y, w[0][2], w[1][2], w[2][2]);
  split3_pair(b.z, b.w, w[0][3], w[1][3], w[2][3]);
  uint16_t* q = x3 + (i >> 1) * 48 + (i & 1) * 8;
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<uint4*>(q + pc * 16) = make_uint4(w[pc][0], w[pc][1], w[pc][2], w[pc][3]);
}

__device__ __forceinline__ float vt_max4(float p0, float p1, float p2, float p3) { return fmaxf(fmaxf(fmaxf(p0, p1), p2), p3); }

// one thread per pooled pixel and channel chunk; CV = chunks per pixel
template <int V>
__global__ void __launch_bounds__(256) vgg_tap_fwd_f32_kernel(const float4* __restrict__ a, float4* __restrict__ pooled, uint16_t* __restrict__ pooled3,
                                                              int H, int W, int CV, int64_t total) {
  const int OH = H >> 1, OW = W >> 1;
  const int64_t right = (int64_t)CV * V, down = (int64_t)W * CV * V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % CV);
    int64_t r = i / CV;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH);
    const int64_t n = r / OH;
    const int64_t o = (((n * H + oy * 2) * W + ox * 2) * CV + c) * V;
    float4 m[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float4 p0 = a[o + e], p1 = a[o + right + e], p2 = a[o + down + e], p3 = a[o + down + right + e];
      m[e] = make_float4(vt_max4(p0.x, p1.x, p2.x, p3.x), vt_max4(p0.y, p1.y, p2.y, p3.y), vt_max4(p0.z, p1.z, p2.z, p3.z),
                         vt_max4(p0.w, p1.w, p2.w, p3.w));
      pooled[i * V + e] = m[e];
    }
    if constexpr (V == 2) vt_pieces(pooled3, i, m[0], m[1]);
  }
}

__device__ __forceinline__ uint32_t vt_arg(float v0, float v1, float v2, float v3) {
  uint32_t arg = 0;
  float m = v0;
  if (v1 > m) { m = v1; arg = 1; }
  if (v2 > m) { m = v2; arg = 2; }
  if (v3 > m) { m = v3; arg = 3; }
  return arg;
}
// channel ch of window position k: ReLU mask bit k * 4 V + ch of posm, the window's winner in bits 2 ch, 2 ch + 1 of argm.
// ADD: an un-pooled gradient exists (the composed path then adds it everywhere, zeros included: -0 + 0 = +0)
template <int V, bool ADD>
__device__ __forceinline__ float vt_dy(float g, float gp, uint32_t posm, uint32_t argm, int k, int ch) {
  if (ADD) g = g + (((argm >> (2 * ch)) & 3u) == (uint32_t)k ? gp : 0.f);
  return ((posm >> (k * 4 * V + ch)) & 1u) ? g : 0.f;
}

// one thread per 2 x 2 window (the windows cover odd extents too: their missing row / column is skipped and they receive no pooled
// gradient) and channel chunk.  g0..g3: the tap gradient as batch slices of slice_f4 float4s each, a null slice is zeros.
template <int V, bool ADD>
__global__ void __launch_bounds__(256) vgg_tap_bwd_f32_kernel(const float4* __restrict__ a, const float4* __restrict__ g0, const float4* __restrict__ g1,
                                                              const float4* __restrict__ g2, const float4* __restrict__ g3, int per_slice,
                                                              int64_t slice_f4, const float4* __restrict__ gpool, float4* __restrict__ dy,
                                                              uint16_t* __restrict__ dy3, int H, int W, int CV, int64_t total) {
  const int OH = H >> 1, OW = W >> 1, WH = (H + 1) >> 1, WW = (W + 1) >> 1;
  const int64_t right = (int64_t)CV * V, down = (int64_t)W * CV * V;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % CV);
    int64_t r = i / CV;
    const int wx = (int)(r % WW);
    r /= WW;
    const int wy = (int)(r % WH);
    const int64_t n = r / WH;
    const bool has_r = wx * 2 + 1 < W, has_d = wy * 2 + 1 < H;
    const bool pool = ADD && wy < OH && wx < OW;  // a whole window: has_r and has_d hold
    const int64_t o = (((n * H + wy * 2) * W + wx * 2) * CV + c) * V;
    const int s = (int)(n / per_slice);
    const float4* gsl = s == 0 ? g0 : s == 1 ? g1 : s == 2 ? g2 : g3;
    const int64_t go = o - (int64_t)s * slice_f4;
    const int64_t off[4] = {0, right, down, down + right};
    const bool has[4] = {true, has_r, has_d, has_r && has_d};
    uint32_t posm = 0, argm = 0;
    float4 gp[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float4 p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p[k] = has[k] ? a[o + off[k] + e] : z4;
        posm |= ((p[k].x > 0.f ? 1u : 0u) | (p[k].y > 0.f ? 2u : 0u) | (p[k].z > 0.f ? 4u : 0u) | (p[k].w > 0.f ? 8u : 0u)) << (k * 4 * V + e * 4);
      }
      gp[e] = z4;  // outside a whole window nothing is routed: every winner test then adds zero
      if (pool) {
        gp[e] = gpool[((((n * OH + wy) * OW + wx) * CV) + c) * V + e];
        argm |= (vt_arg(p[0].x, p[1].x, p[2].x, p[3].x) | vt_arg(p[0].y, p[1].y, p[2].y, p[3].y) << 2 | vt_arg(p[0].z, p[1].z, p[2].z, p[3].z) << 4 |
                 vt_arg(p[0].w, p[1].w, p[2].w, p[3].w) << 6) << (e * 8);
      }
    }
#pragma unroll 1  // position by position: the loads of all four at once cost the eighth wave per SIMD
    for (int k = 0; k < 4; ++k) {
      if (((k & 1) && !has_r) || ((k & 2) && !has_d)) continue;
      const int64_t offk = (k & 1 ? right : 0) + (k & 2 ? down : 0);
      float4 out[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float4 g = gsl ? gsl[go + offk + e] : z4;
        out[e] = make_float4(vt_dy<V, ADD>(g.x, gp[e].x, posm, argm, k, e * 4), vt_dy<V, ADD>(g.y, gp[e].y, posm, argm, k, e * 4 + 1),
                             vt_dy<V, ADD>(g.z, gp[e].z, posm, argm, k, e * 4 + 2), vt_dy<V, ADD>(g.w, gp[e].w, posm, argm, k, e * 4 + 3));
        if (dy) dy[o + offk + e] = out[e];
      }
      if constexpr (V == 2) {
        if (dy3) vt_pieces(dy3, (o + offk) >> 1, out[0], out[1]);  // o / V = pixel * CV + c
      }
    }
  }
}

/* pooled = maxpool2(a) (floor mode, fmi_maxpool2_f32's values) and, when pooled3 is not NULL, pooled's bf16 piece image (fmi_split3_f32's
 * bits) from ONE pass over the activated map a [N,H,W,C]; a itself is the tap.  C % 4 == 0, pieces C % 16 == 0, 16-byte aligned
 * pointers, else FMI_ERR_UNSUPPORTED */
extern "C" int fmi_vgg_tap_fwd_f32(const float* a, float* pooled, void* pooled3, int N, int H, int W, int C, void* stream) {
  if (!a || !pooled || N <= 0 || H < 2 || W < 2 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 4 != 0 || (pooled3 && C % 16 != 0) || !fmi_al16(a) || !fmi_al16(pooled) || !fmi_al16(pooled3)) return FMI_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t windows = (int64_t)N * (H / 2) * (W / 2);
  if (pooled3) {
    const int64_t total = windows * (C / 8);
    hipLaunchKernelGGL(vgg_tap_fwd_f32_kernel<2>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const float4*)a, (float4*)pooled,
                       (uint16_t*)pooled3, H, W, C / 8, total);
  } else {
    const int64_t total = windows * (C / 4);
    hipLaunchKernelGGL(vgg_tap_fwd_f32_kernel<1>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const float4*)a, (float4*)pooled,
                       (uint16_t*)nullptr, H, W, C / 4, total);
  }
  return fmi_launch_status();
}

template <int V>
static void vt_launch_bwd(const float* a, const float4* const (&gs)[VT_MAX_SLICES], int per_slice, const float* gpool, float* dy, void* dy3, int N, int H, int W, int C,
                          hipStream_t st) {
  const int CV = C / (4 * V);
  const int64_t total = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * CV;
  const int64_t slice_f4 = (int64_t)per_slice * H * W * (C / 4);
  const dim3 grid(fmi_bw_grid(total, 256)), block(256);
  if (gpool)
    hipLaunchKernelGGL((vgg_tap_bwd_f32_kernel<V, true>), grid, block, 0, st, (const float4*)a, gs[0], gs[1], gs[2], gs[3], per_slice, slice_f4, (const float4*)gpool,
                       (float4*)dy, (uint16_t*)dy3, H, W, CV, total);
  else
    hipLaunchKernelGGL((vgg_tap_bwd_f32_kernel<V, false>), grid, block, 0, st, (const float4*)a, gs[0], gs[1], gs[2], gs[3], per_slice, slice_f4, (const float4*)nullptr,
                       (float4*)dy, (uint16_t*)dy3, H, W, CV, total);
}

/* dy = a > 0 ? (gtap + unpool(gpool)) : 0 for the activated map a [N,H,W,C] of a block's last convolution.  gtap: nslice (1..4) batch
 * slices gslice[s] of rows_per_slice = N / nslice images each, a NULL slice is zeros (neither filled nor read); gpool [N,H/2,W/2,C]
 * (NULL: none, and no add) goes to the FIRST maximum of its window in row-major order (strict >), rows and columns beyond 2 (H/2),
 * 2 (W/2) receive nothing.  dy (fp32) and dy3 (dy's bf16 piece image, fmi_split3_f32's bits) are each optional, one of them is needed; a
 * NULL one is not written.  Bit-equal to zeros / cat, add, fmi_maxpool2_bwd_f32 and FMI_EW_RELU_BWD_OUT on the same operands.
 * C % 4 == 0, pieces C % 16 == 0, 16-byte aligned pointers, else FMI_ERR_UNSUPPORTED */
extern "C" int fmi_vgg_tap_bwd_f32(const float* a, const float* const* gslice, int nslice, int rows_per_slice, const float* gpool, float* dy,
                                   void* dy3, int N, int H, int W, int C, void* stream) {
  if (!a || !gslice || (!dy && !dy3) || N <= 0 || H <= 0 || W <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (nslice < 1 || nslice > VT_MAX_SLICES || rows_per_slice < 1 || (int64_t)nslice * rows_per_slice != N) return FMI_ERR_BAD_ARG;
  if (gpool && (H < 2 || W < 2)) return FMI_ERR_BAD_ARG;
  if (C % 4 != 0 || (dy3 && C % 16 != 0) || !fmi_al16(a) || !fmi_al16(gpool) || !fmi_al16(dy) || !fmi_al16(dy3)) return FMI_ERR_UNSUPPORTED;
  const float4* gs[VT_MAX_SLICES] = {nullptr, nullptr, nullptr, nullptr};
  for (int s = 0; s < nslice; ++s) {
    if (!fmi_al16(gslice[s])) return FMI_ERR_UNSUPPORTED;
    gs[s] = (const float4*)gslice[s];
  }
  if (dy3) vt_launch_bwd<2>(a, gs, rows_per_slice, gpool, dy, dy3, N, H, W, C, (hipStream_t)stream);
  else vt_launch_bwd<1>(a, gs, rows_per_slice, gpool, dy, dy3, N, H, W, C, (hipStream_t)stream);
  return fmi_launch_status();
}
