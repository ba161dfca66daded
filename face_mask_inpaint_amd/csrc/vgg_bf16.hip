// bf16 VGG16 trunk of VGGLoss (modules/loss.py:33-65 of the reference: the four blocks of vgg16.features[:23], each followed by a loss
// term on its activated map): the passes at the points where the losses tap a feature map.  NHWC bf16 maps (uint16_t = raw bits),
// C % 8 == 0: one thread moves 8 channels (16 bytes) of one 2 x 2 window, as the pool kernels of unet_bf16.hip do.  The loss kernels read
// fp32, so the tap is the widened map (exact); the pool that opens the next block is taken in the same pass.  No atomics: both modes of
// fmi_set_deterministic run the same code.
#include "bf16x8.h"

// the pool's winner rule (unet_bf16.hip): the FIRST maximum of the window in row-major order wins and a later NaN replaces the running one
__device__ __forceinline__ bool vt_takes(float v, float t) { return v > t || v != v; }

__device__ __forceinline__ void vt_store8f(float* p, const float (&f)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// one thread per WINDOW (H, W even) or per PIXEL (POOL = false: the last block, and maps of odd extent without a pool)
template <bool POOL>
__global__ void __launch_bounds__(256) vgg_tap_fwd_bf16_kernel(const uint4* __restrict__ a, float* __restrict__ tap, uint4* __restrict__ pooled, int H,
                                                               int W, int C8, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if constexpr (!POOL) {
      float v[8];
      bf_unpack8(a[i], v);
      vt_store8f(tap + i * 8, v);
    } else {
      const int OH = H >> 1, OW = W >> 1;
      const int c = (int)(i % C8);
      int64_t r = i / C8;
      const int ox = (int)(r % OW);
      r /= OW;
      const int oy = (int)(r % OH);
      const int64_t n = r / OH;
      const int64_t o = ((n * H + oy * 2) * W + ox * 2) * C8 + c, down = (int64_t)W * C8;
      float v0[8], v1[8], v2[8], v3[8], m[8];
      bf_unpack8(a[o], v0);
      bf_unpack8(a[o + C8], v1);
      bf_unpack8(a[o + down], v2);
      bf_unpack8(a[o + down + C8], v3);
      vt_store8f(tap + o * 8, v0);
      vt_store8f(tap + (o + C8) * 8, v1);
      vt_store8f(tap + (o + down) * 8, v2);
      vt_store8f(tap + (o + down + C8) * 8, v3);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = v0[e];
        if (vt_takes(v1[e], t)) t = v1[e];
        if (vt_takes(v2[e], t)) t = v2[e];
        if (vt_takes(v3[e], t)) t = v3[e];
        m[e] = t;
      }
      pooled[i] = bf_trunc8(m);  // a maximum of bf16 values: no rounding step
    }
  }
}

// dy = a > 0 ? gtap + unpool(gpool) : 0: the fp32 sum, one rounding to nearest even
__device__ __forceinline__ uint4 vt_bwd8(const float (&av)[8], const float* gt, const float (&gp)[8]) {
  float g[8], o[8];
  bf_load8f(gt, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = av[e] > 0.f ? g[e] + gp[e] : 0.f;
  return bf_pack8(o);
}
template <bool POOL>
__global__ void __launch_bounds__(256) vgg_tap_bwd_bf16_kernel(const uint4* __restrict__ a, const float* __restrict__ gtap,
                                                               const uint4* __restrict__ gpool, uint4* __restrict__ dy, int H, int W, int C8,
                                                               int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if constexpr (!POOL) {
      float v[8];
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      bf_unpack8(a[i], v);
      dy[i] = vt_bwd8(v, gtap + i * 8, z);
    } else {
      const int OH = H >> 1, OW = W >> 1;
      const int c = (int)(i % C8);
      int64_t r = i / C8;
      const int ox = (int)(r % OW);
      r /= OW;
      const int oy = (int)(r % OH);
      const int64_t n = r / OH;
      const int64_t o = ((n * H + oy * 2) * W + ox * 2) * C8 + c, down = (int64_t)W * C8;
      float v0[8], v1[8], v2[8], v3[8], g[8], q[4][8];
      bf_unpack8(a[o], v0);
      bf_unpack8(a[o + C8], v1);
      bf_unpack8(a[o + down], v2);
      bf_unpack8(a[o + down + C8], v3);
      bf_unpack8(gpool[i], g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int arg = 0;
        float t = v0[e];
        if (vt_takes(v1[e], t)) { t = v1[e]; arg = 1; }
        if (vt_takes(v2[e], t)) { t = v2[e]; arg = 2; }
        if (vt_takes(v3[e], t)) { t = v3[e]; arg = 3; }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k][e] = arg == k ? g[e] : 0.f;
      }
      dy[o] = vt_bwd8(v0, gtap + o * 8, q[0]);
      dy[o + C8] = vt_bwd8(v1, gtap + (o + C8) * 8, q[1]);
      dy[o + down] = vt_bwd8(v2, gtap + (o + down) * 8, q[2]);
      dy[o + down + C8] = vt_bwd8(v3, gtap + (o + down + C8) * 8, q[3]);
    }
  }
}

static int vt_args(const void* a, const void* b, const void* c, const void* opt, int N, int H, int W, int C) {
  if (!a || !b || !c || N <= 0 || H <= 0 || W <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(a) || !fmi_al16(b) || !fmi_al16(c) || !fmi_al16(opt)) return FMI_ERR_UNSUPPORTED;
  if (opt && ((H & 1) || (W & 1))) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
/* tap = float(a) (exact) and, when pooled is not NULL, pooled = maxpool2(a) with fmi_maxpool2_bf16's winner rule: one pass over a */
extern "C" int fmi_vgg_tap_fwd_bf16(const uint16_t* a, float* tap, uint16_t* pooled, int N, int H, int W, int C, void* stream) {
  const int rc = vt_args(a, tap, tap, pooled, N, H, W, C);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pooled) {
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(vgg_tap_fwd_bf16_kernel<true>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const uint4*)a, tap, (uint4*)pooled, H, W,
                       C / 8, total);
  } else {
    const int64_t total = (int64_t)N * H * W * (C / 8);
    hipLaunchKernelGGL(vgg_tap_fwd_bf16_kernel<false>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const uint4*)a, tap, (uint4*)nullptr, H, W,
                       C / 8, total);
  }
  return fmi_launch_status();
}
/* dy = bf16(a > 0 ? gtap + unpool(gpool) : 0): the ReLU's mask, the tap's fp32 gradient and the pooled map's bf16 gradient (NULL: none)
 * routed to each window's winner, summed in fp32 and rounded once */
extern "C" int fmi_vgg_tap_bwd_bf16(const uint16_t* a, const float* gtap, const uint16_t* gpool, uint16_t* dy, int N, int H, int W, int C,
                                    void* stream) {
  const int rc = vt_args(a, gtap, dy, gpool, N, H, W, C);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (gpool) {
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(vgg_tap_bwd_bf16_kernel<true>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const uint4*)a, gtap, (const uint4*)gpool,
                       (uint4*)dy, H, W, C / 8, total);
  } else {
    const int64_t total = (int64_t)N * H * W * (C / 8);
    hipLaunchKernelGGL(vgg_tap_bwd_bf16_kernel<false>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, (const uint4*)a, gtap,
                       (const uint4*)nullptr, (uint4*)dy, H, W, C / 8, total);
  }
  return fmi_launch_status();
}
