// The pixel head of pSpLoss.__call__ (modules/psp/criteria/__init__.py:58-65,80-87): from ONE read of the images the generator and the
// dataloader hand over -- y_hat, y, ref [N][3][H][W] planar (y_hat also in the channels-last memory pSp.forward's pool leaves it in) and
// the mask [N][H][W] -- the two masked NHWC batches LPIPS consumes
// (cat(y_hat (1 - m), y (1 - m)) and cat(y_hat m, ref m), [2N][H][W][3]) and the two F.mse_loss values; and its backward in one pass
// that recomputes the products (nothing per pixel is saved).  Bandwidth kernels: a thread takes four neighbouring pixels of a sample
// (one 16-byte load per plane, three 16-byte stores per interleaved output) or, when H * W % 4 != 0 or a base is not 16-byte aligned,
// one pixel.  The sums of squares are accumulated in fp64, reduced to one partial row per workgroup and finished by a second launch
// in a fixed order (the scheme, its helpers and the RGB pixel I/O: head.h): no atomics, nothing to zero, bit-reproducible in either mode.
// Every product is one rounded fp32 multiply and 1 - m one rounded subtraction (never contracted), so the batches equal torch's bit for bit.
#include "common.h"
#include "head.h"

namespace {

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
    load_rgb_run<PX>(yh, yh_hwc, n, hw, p, a);
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
  if (part) block_rows_out<2>(acc, part, n * gridDim.x + blockIdx.x);
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
    load_rgb_run<PX>(yh, yh_hwc, n, hw, p, a);
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
    store_rgb_run<PX>(d_yh, yh_hwc, n, hw, p, d);  // the gradient in y_hat's own layout
  }
}

}  // namespace

extern "C" int fmi_psp_pixel_head_fwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, float* pair_out, float* pair_in,
                                          double* sums, float* out2, int N, int H, int W, int y_hat_hwc, double* ws_part, int64_t ws_doubles, void* stream) {
  if (!y_hat || !y || (y_hat_hwc != 0 && y_hat_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0) return FMI_ERR_BAD_ARG;
  if (!pair_out && !pair_in && !sums && !out2) return FMI_ERR_BAD_ARG;
  if (pair_in && (!ref || !mask)) return FMI_ERR_BAD_ARG;  // the inner pair needs both
  const void* all[] = {y_hat, y, ref, mask, pair_out, pair_in, out2};
  for (const void* q : all)
    if (!al4(q)) return FMI_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(sums) & 7) || (reinterpret_cast<uintptr_t>(ws_part) & 7)) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W;
  bool vec = (hw & 3) == 0;
  for (const void* q : all) vec = vec && fmi_al16(q);
  const int64_t per = vec ? hw >> 2 : hw;
  const int gx = rows_for(per, ROWS_PER_PLANE);
  const bool want_sums = sums || out2;
  if (want_sums && (!ws_part || ws_doubles < (int64_t)N * gx * 2)) return FMI_ERR_BAD_ARG;
  double* part = want_sums ? ws_part : nullptr;
  const dim3 grid(gx, N), block(256);
  if (vec)
    hipLaunchKernelGGL(psp_head_fwd_kernel<4>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, pair_out, pair_in, part, N, hw, per, y_hat_hwc != 0);
  else
    hipLaunchKernelGGL(psp_head_fwd_kernel<1>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, pair_out, pair_in, part, N, hw, per, y_hat_hwc != 0);
  if (want_sums)
    hipLaunchKernelGGL(rows_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int64_t)N * gx, 2, 3.0 * (double)N * (double)hw, sums, out2);
  return fmi_launch_status();
}

extern "C" int fmi_psp_pixel_head_bwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, const float* g_pair_out,
                                          const float* g_pair_in, const float* g2, float* d_y_hat, int N, int H, int W, int y_hat_hwc, void* stream) {
  if (!y_hat || !y || !g2 || !d_y_hat || (y_hat_hwc != 0 && y_hat_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0) return FMI_ERR_BAD_ARG;
  if (g_pair_in && (!ref || !mask)) return FMI_ERR_BAD_ARG;
  const void* all[] = {y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat};
  for (const void* q : all)
    if (!al4(q)) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W;
  bool vec = (hw & 3) == 0;
  for (const void* q : all)
    if (q != g2) vec = vec && fmi_al16(q);
  const int64_t per = vec ? hw >> 2 : hw;
  const dim3 grid(rows_for(per, 1024), N), block(256);
  const double count = 3.0 * (double)N * (double)hw;
  if (vec)
    hipLaunchKernelGGL(psp_head_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat, count, hw, per, y_hat_hwc != 0);
  else
    hipLaunchKernelGGL(psp_head_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, y_hat, y, ref, mask, g_pair_out, g_pair_in, g2, d_y_hat, count, hw, per, y_hat_hwc != 0);
  return fmi_launch_status();
}
