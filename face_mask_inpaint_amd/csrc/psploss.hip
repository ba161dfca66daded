// The pixel head of pSpLoss.__call__ (modules/psp/criteria/__init__.py:58-65,80-87): from ONE read of the images the generator and the
// dataloader hand over -- y_hat, y, ref [N][3][H][W] planar (y_hat also in the channels-last memory pSp.forward's pool leaves it in) and
// the mask [N][H][W] -- the two masked NHWC batches LPIPS consumes
// (cat(y_hat (1 - m), y (1 - m)) and cat(y_hat m, ref m), [2N][H][W][3]) and the two F.mse_loss values; and its backward in one pass
// that recomputes the products (nothing per pixel is saved).  Bandwidth kernels: a thread takes four neighbouring pixels of a sample
// (one 16-byte load per plane, three 16-byte stores per interleaved output) or, when H * W % 4 != 0 or a base is not 16-byte aligned,
// one pixel.  The sums of squares are accumulated in fp64 and reduced wave shuffle -> LDS -> one partial row per workgroup; a finishing
// launch adds the rows in a fixed order (the scheme of segloss.hip): no atomics, nothing to zero, bit-reproducible in either mode.
// Every product is one rounded fp32 multiply and 1 - m one rounded subtraction (never contracted), so the batches equal torch's bit for bit.
#include "common.h"

namespace {

constexpr int HEAD_GX_MAX = 64;  // workgroups (= partial rows) per sample of the forward

// v[k] (k < 2) of every thread -> part[row][k]: wave shuffle, LDS, the four waves added in a fixed order
__device__ __forceinline__ void head_rows_out(double* v, double* __restrict__ part, int64_t row) {
  __shared__ double red[4][2];
  v[0] = wave_sum_d(v[0]), v[1] = wave_sum_d(v[1]);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = v[0], red[threadIdx.x >> 6][1] = v[1];
  __syncthreads();
  if (threadIdx.x < 2) part[row * 2 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// PX pixels of one plane starting at element e
template <int PX>
__device__ __forceinline__ void load_px(const float* __restrict__ x, int64_t e, float* v) {
  if (PX == 4) {
    const float4 t = *reinterpret_cast<const float4*>(x + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = x[e];
  }
}
// 3 PX interleaved values to / from element e of an NHWC image
template <int PX>
__device__ __forceinline__ void store_hwc(float* __restrict__ x, int64_t e, const float* v) {
  if (PX == 4) {
    float4* q = reinterpret_cast<float4*>(x + e);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) x[e + k] = v[k];
  }
}
template <int PX>
__device__ __forceinline__ void load_hwc(const float* __restrict__ x, int64_t e, float* v) {
  if (PX == 4) {
    const float4* q = reinterpret_cast<const float4*>(x + e);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = q[k];
      v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x[e + k];
  }
}

// PX pixels x RGB of y_hat into a[c][j]: from three planes, or from an interleaved [N][H][W][3] image (hwc)
template <int PX>
__device__ __forceinline__ void load_yh(const float* __restrict__ yh, bool hwc, int64_t n, int64_t hw, int64_t p, float (*a)[PX]) {
  if (hwc) {
    float t[3 * PX];
    load_hwc<PX>(yh, (n * hw + p) * 3, t);
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c][j] = t[j * 3 + c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) load_px<PX>(yh, (n * 3 + c) * hw + p, a[c]);
  }
}

// grid (gx, N); per = work items of a sample (H W / 4 groups of four pixels, or H W pixels); part (may be NULL: no sums wanted)
template <int PX>
__global__ void __launch_bounds__(256) psp_head_fwd_kernel(const float* __restrict__ yh, const float* __restrict__ y, const float* __restrict__ ref,
                                                           const float* __restrict__ mask, float* __restrict__ pair_out, float* __restrict__ pair_in,
                                                           double* __restrict__ part, int N, int64_t hw, int64_t per, bool yh_hwc) {
  const int64_t n = blockIdx.y;
  const bool inner = ref != nullptr && mask != nullptr;
  double acc[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i * PX;
    float m[PX], im[PX], a[3][PX], b[3][PX], r[3][PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) m[j] = 0.f, im[j] = 1.f;
    if (mask) {
      load_px<PX>(mask, n * hw + p, m);
#pragma unroll
      for (int j = 0; j < PX; ++j) im[j] = __fsub_rn(1.f, m[j]);
    }
    load_yh<PX>(yh, yh_hwc, n, hw, p, a);
#pragma unroll
    for (int c = 0; c < 3; ++c) load_px<PX>(y, (n * 3 + c) * hw + p, b[c]);
    float oa[3 * PX], ob[3 * PX];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = __fmul_rn(a[c][j], im[j]), v = __fmul_rn(b[c][j], im[j]);
        oa[j * 3 + c] = u, ob[j * 3 + c] = v;
        const double d = (double)__fsub_rn(u, v);
        acc[0] += d * d;
      }
    if (pair_out) {
      store_hwc<PX>(pair_out, (n * hw + p) * 3, oa);
      store_hwc<PX>(pair_out, ((N + n) * hw + p) * 3, ob);
    }
    if (inner) {
#pragma unroll
      for (int c = 0; c < 3; ++c) load_px<PX>(ref, (n * 3 + c) * hw + p, r[c]);
#pragma unroll
      for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float u = __fmul_rn(a[c][j], m[j]), v = __fmul_rn(r[c][j], m[j]);
          oa[j * 3 + c] = u, ob[j * 3 + c] = v;
          const double d = (double)__fsub_rn(u, v);
          acc[1] += d * d;
        }
      if (pair_in) {
        store_hwc<PX>(pair_in, (n * hw + p) * 3, oa);
        store_hwc<PX>(pair_in, ((N + n) * hw + p) * 3, ob);
      }
    }
  }
  if (part) head_rows_out(acc, part, n * gridDim.x + blockIdx.x);
}

// one workgroup: thread t adds rows t, t + 256, ... in order, then the block in a fixed order
__global__ void __launch_bounds__(256) psp_head_finish_kernel(const double* __restrict__ part, int64_t rows, double count, double* __restrict__ sums,
                                                              float* __restrict__ out2) {
  __shared__ double red[4];
  for (int k = 0; k < 2; ++k) {
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += 256) s += part[r * 2 + k];
    s = block_sum_256_d(s, red);
    if (threadIdx.x == 0) {
      if (sums) sums[k] = s;
      if (out2) out2[k] = (float)(s / count);
    }
  }
}

// grid (gx, N); s[k] = g2[k] * 2 / count.  The differences are taken in their factored form im (y_hat - y) and m (y_hat - ref) -- the same
// value with one rounding of the difference itself instead of one per product, so an entry is within a few ulps of ITS terms even where
// y_hat is close to y and im is not a power of two
template <int PX>
__global__ void __launch_bounds__(256) psp_head_bwd_kernel(const float* __restrict__ yh, const float* __restrict__ y, const float* __restrict__ ref,
                                                           const float* __restrict__ mask, const float* __restrict__ g_pair_out,
                                                           const float* __restrict__ g_pair_in, const float* __restrict__ g2, float* __restrict__ d_yh,
                                                           double count, int64_t hw, int64_t per, bool yh_hwc) {
  const int64_t n = blockIdx.y;
  const bool inner = ref != nullptr && mask != nullptr;
  const float s0 = (float)((double)g2[0] * 2.0 / count), s1 = (float)((double)g2[1] * 2.0 / count);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i * PX;
    float m[PX], im[PX], a[3][PX], b[3][PX], go[3 * PX], gi[3 * PX], d[3][PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) m[j] = 0.f, im[j] = 1.f;
#pragma unroll
    for (int k = 0; k < 3 * PX; ++k) go[k] = 0.f, gi[k] = 0.f;
    if (mask) {
      load_px<PX>(mask, n * hw + p, m);
#pragma unroll
      for (int j = 0; j < PX; ++j) im[j] = __fsub_rn(1.f, m[j]);
    }
    load_yh<PX>(yh, yh_hwc, n, hw, p, a);
#pragma unroll
    for (int c = 0; c < 3; ++c) load_px<PX>(y, (n * 3 + c) * hw + p, b[c]);
    if (g_pair_out) load_hwc<PX>(g_pair_out, (n * hw + p) * 3, go);
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float diff = im[j] * (a[c][j] - b[c][j]);
        d[c][j] = im[j] * (go[j * 3 + c] + s0 * diff);
      }
    if (inner) {
#pragma unroll
      for (int c = 0; c < 3; ++c) load_px<PX>(ref, (n * 3 + c) * hw + p, b[c]);
      if (g_pair_in) load_hwc<PX>(g_pair_in, (n * hw + p) * 3, gi);
#pragma unroll
      for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float diff = m[j] * (a[c][j] - b[c][j]);
          d[c][j] += m[j] * (gi[j * 3 + c] + s1 * diff);
        }
    }
    if (yh_hwc) {  // the gradient in y_hat's own layout
#pragma unroll
      for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) go[j * 3 + c] = d[c][j];
      store_hwc<PX>(d_yh, (n * hw + p) * 3, go);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (PX == 4)
          *reinterpret_cast<float4*>(d_yh + (n * 3 + c) * hw + p) = make_float4(d[c][0], d[c][1], d[c][2], d[c][3]);
        else
          d_yh[(n * 3 + c) * hw + p] = d[c][0];
      }
    }
  }
}

inline bool head_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool head_al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int head_gx(int64_t per, int cap) {
  int64_t g = ceil_div64(per, 256);
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

extern "C" int fmi_psp_pixel_head_fwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, float* pair_out, float* pair_in,
                                          double* sums, float* out2, int N, int H, int W, int y_hat_hwc, double* ws_part, int64_t ws_doubles, void* stream) {
  if (!y_hat || !y || (y_hat_hwc != 0 && y_hat_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0) return FMI_ERR_BAD_ARG;
  if (!pair_out && !pair_in && !sums && !out2) return FMI_ERR_BAD_ARG;
  if (pair_in && (!ref || !mask)) return FMI_ERR_BAD_ARG;  // the inner pair needs both
  const void* all[] = {y_hat, y, ref, mask, pair_out, pair_in, out2};
  for (const void* q : all)
    if (!head_al4(q)) return FMI_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(sums) & 7) || (reinterpret_cast<uintptr_t>(ws_part) & 7)) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W;
  bool vec = (hw & 3) == 0;
  for (const void* q : all) vec = vec && head_al16(q);
  const int64_t per = vec ? hw >> 2 : hw;
  const int gx = head_gx(per, HEAD_GX_MAX);
  const bool want_sums = sums || out2;
  if (want_sums && (!ws_part || ws_doubles < (int64_t)N * gx * 2)) return FMI_ERR_BAD_ARG;
  double* part = want_sums ? ws_part : nullptr;
  const dim3 grid(gx, N), block(256);
  if (vec)
    hipLaunchKernelGGL(psp_head_fwd_kernel<4>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, pair_out, pair_in, part, N, hw, per, y_hat_hwc != 0);
  else
    hipLaunchKernelGGL(psp_head_fwd_kernel<1>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, pair_out, pair_in, part, N, hw, per, y_hat_hwc != 0);
  if (want_sums)
    hipLaunchKernelGGL(psp_head_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int64_t)N * gx, 3.0 * (double)N * (double)hw, sums, out2);
  return fmi_launch_status();
}

extern "C" int fmi_psp_pixel_head_bwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, const float* g_pair_out,
                                          const float* g_pair_in, const float* g2, float* d_y_hat, int N, int H, int W, int y_hat_hwc, void* stream) {
  if (!y_hat || !y || !g2 || !d_y_hat || (y_hat_hwc != 0 && y_hat_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0) return FMI_ERR_BAD_ARG;
  if (g_pair_in && (!ref || !mask)) return FMI_ERR_BAD_ARG;
  const void* all[] = {y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat};
  for (const void* q : all)
    if (!head_al4(q)) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W;
  bool vec = (hw & 3) == 0;
  for (const void* q : all)
    if (q != g2) vec = vec && head_al16(q);
  const int64_t per = vec ? hw >> 2 : hw;
  const dim3 grid(head_gx(per, 1024), N), block(256);
  const double count = 3.0 * (double)N * (double)hw;
  if (vec)
    hipLaunchKernelGGL(psp_head_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat, count, hw, per, y_hat_hwc != 0);
  else
    hipLaunchKernelGGL(psp_head_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat, count, hw, per, y_hat_hwc != 0);
  return fmi_launch_status();
}
