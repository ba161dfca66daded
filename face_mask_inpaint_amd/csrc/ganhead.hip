// The image head of GANOptimizer.__call__ (modules/loss.py:48-51,84-95,115): from ONE read of the images the generator and the dataloader
// hand over -- gen [N][3][H][W] (planar, or the channels-last memory ReferenceFill.forward leaves it in), gt, src, ref planar and the
// mask [N][H][W] -- the two NHWC batches VGGLoss.forward_multi feeds its first block,
//   x_in [3N][OH][OW][3] = norm(R(gen)), norm(R(gen (1 - m))), norm(R(gen m))        y_in = norm(R(gt)), norm(R(src)), norm(R(ref m))
// (R: bilinear, align_corners=True, lerp_of of common.h; norm(v) = (v - mean[c]) / std[c]; the mask multiplied in BEFORE R), and the
// L1 term mean |gen - gt|; and its backward in one launch that recomputes the products (nothing per pixel is saved) with R's adjoint in
// gather form: every input pixel sums its contributing output pixels in a fixed order, so d_gen is written, not accumulated -- no
// atomics, no zero fill, bit-reproducible in either mode.  Bandwidth kernels: a thread takes four neighbouring output pixels of a row
// (three 16-byte stores per stream) on the forward, four neighbouring input pixels on the backward, or one pixel when the row length is
// not a multiple of four or a base is not 16-byte aligned.  |gen - gt| is accumulated in fp64, reduced to one partial row per workgroup and
// finished by a second launch in a fixed order (the scheme, its helpers and the RGB pixel I/O: head.h).
// Every product is one rounded fp32 multiply and 1 - m one rounded subtraction.  The file is compiled without FMA contraction (the pragma
// below, ahead of the includes so that it covers them): lerp_of's l1 = r - i0 is then taken from the ROUNDED r = scale * o, the value its
// index i0 = (int)r comes from, in the forward and in the backward alike -- fused, scale * o - i0 moves a weight by up to half an ulp of r (4e-6 at 224), and
// nothing would guarantee the two directions the same choice.
#pragma clang fp contract(off)
#include "common.h"
#include "head.h"

namespace {

// the interpolation of resize_kernel (pool.hip): two rounded operations per lerp level
__device__ __forceinline__ float bilerp(const Lerp& ly, const Lerp& lx, float v00, float v01, float v10, float v11) {
  return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

// sum |gen - gt| over this workgroup's share of sample n
template <int PX>
__device__ __forceinline__ double l1_share(const float* __restrict__ gen, const float* __restrict__ gt, bool hwc, int64_t n, int64_t hw) {
  double acc = 0.0;
  const int64_t per = hw / PX;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    float a[3][PX], b[3][PX];
    load_rgb_run<PX>(gen, hwc, n, hw, i * PX, a);
    load_rgb_run<PX>(gt, false, n, hw, i * PX, b);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < PX; ++j) acc += (double)fabsf(__fsub_rn(a[c][j], b[c][j]));
  }
  return acc;
}

// grid (gx, N).  per = work items of a sample's output: OH * OW / PX runs of PX pixels of a row.  part [N * gx] (NULL: l1 not wanted)
template <int PX>
__global__ void __launch_bounds__(256) gan_head_fwd_kernel(const float* __restrict__ gen, const float* __restrict__ gt, const float* __restrict__ src,
                                                           const float* __restrict__ ref, const float* __restrict__ mask, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, float* __restrict__ x_in, float* __restrict__ y_in,
                                                           double* __restrict__ part, int N, int H, int W, int OH, int OW, int64_t per, bool hwc,
                                                           bool l1_vec) {
  const int64_t n = blockIdx.y, hw = (int64_t)H * W, ohw = (int64_t)OH * OW;
  const int runs = OW / PX;
  float mu[3], sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) mu[c] = mean[c], sd[c] = stdv[c];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const int oy = (int)(i / runs), ox0 = (int)(i % runs) * PX;
    const Lerp ly = lerp_of(oy, H, OH);
    float o[6][3 * PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const Lerp lx = lerp_of(ox0 + j, W, OW);
      const int64_t p[4] = {(int64_t)ly.i0 * W + lx.i0, (int64_t)ly.i0 * W + lx.i1, (int64_t)ly.i1 * W + lx.i0, (int64_t)ly.i1 * W + lx.i1};
      float m[4], im[4], g[4][3], t[4][3], s[4][3], r[4][3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        m[k] = mask[n * hw + p[k]];
        im[k] = __fsub_rn(1.f, m[k]);
        load_rgb(gen, hwc, n, hw, p[k], g[k]);
        load_rgb(gt, false, n, hw, p[k], t[k]);
        load_rgb(src, false, n, hw, p[k], s[k]);
        load_rgb(ref, false, n, hw, p[k], r[k]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v0 = bilerp(ly, lx, g[0][c], g[1][c], g[2][c], g[3][c]);
        const float v1 = bilerp(ly, lx, __fmul_rn(g[0][c], im[0]), __fmul_rn(g[1][c], im[1]), __fmul_rn(g[2][c], im[2]), __fmul_rn(g[3][c], im[3]));
        const float v2 = bilerp(ly, lx, __fmul_rn(g[0][c], m[0]), __fmul_rn(g[1][c], m[1]), __fmul_rn(g[2][c], m[2]), __fmul_rn(g[3][c], m[3]));
        const float w0 = bilerp(ly, lx, t[0][c], t[1][c], t[2][c], t[3][c]);
        const float w1 = bilerp(ly, lx, s[0][c], s[1][c], s[2][c], s[3][c]);
        const float w2 = bilerp(ly, lx, __fmul_rn(r[0][c], m[0]), __fmul_rn(r[1][c], m[1]), __fmul_rn(r[2][c], m[2]), __fmul_rn(r[3][c], m[3]));
        o[0][j * 3 + c] = (v0 - mu[c]) / sd[c];
        o[1][j * 3 + c] = (v1 - mu[c]) / sd[c];
        o[2][j * 3 + c] = (v2 - mu[c]) / sd[c];
        o[3][j * 3 + c] = (w0 - mu[c]) / sd[c];
        o[4][j * 3 + c] = (w1 - mu[c]) / sd[c];
        o[5][j * 3 + c] = (w2 - mu[c]) / sd[c];
      }
    }
    const int64_t e = ((int64_t)oy * OW + ox0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      store_hwc<PX>(x_in, ((int64_t)k * N + n) * ohw * 3 + e, o[k]);
      store_hwc<PX>(y_in, ((int64_t)k * N + n) * ohw * 3 + e, o[3 + k]);
    }
  }
  if (part) {
    double acc = l1_vec ? l1_share<4>(gen, gt, hwc, n, hw) : l1_share<1>(gen, gt, hwc, n, hw);
    block_rows_out<1>(&acc, part, n * gridDim.x + blockIdx.x);
  }
}

// does output index o of an axis read input index i?  (its weights: l0 if i0 == i, l1 if i1 == i -- both at the clamped last index)
__device__ __forceinline__ bool touches(int o, int i, int in, int out) {
  const Lerp l = lerp_of(o, in, out);
  return l.i0 == i || l.i1 == i;
}
// the weight output l gives input index i: l0 if it is the first corner, l1 if the second, their sum at the clamped last index, where it
// is both; 0 if neither (only a candidate that contributors() could not exclude)
__device__ __forceinline__ float weight_on(const Lerp& l, int i) { return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f); }
// the contributors of input index i: the candidates of resize_cands narrowed to the outputs that read i (they are contiguous: i0 is
// monotonic in o).  lo > hi: none
__device__ __forceinline__ void contributors(int i, int in, int out, int& lo, int& hi) {
  resize_cands(i, in, out, lo, hi);
  while (lo <= hi && !touches(lo, i, in, out)) ++lo;
  while (hi >= lo && !touches(hi, i, in, out)) --hi;
}

// grid (gx, N); per = H * W / PX runs of PX input pixels of a row.  gx [3N][OH][OW][3] (NULL: zero); g_l1 a DEVICE scalar (NULL: zero)
template <int PX>
__global__ void __launch_bounds__(256) gan_head_bwd_kernel(const float* __restrict__ gen, const float* __restrict__ gt, const float* __restrict__ mask,
                                                           const float* __restrict__ stdv, const float* __restrict__ gx, const float* __restrict__ g_l1,
                                                           float* __restrict__ d_gen, int N, int H, int W, int OH, int OW, int64_t per, double count,
                                                           bool hwc) {
  const int64_t n = blockIdx.y, hw = (int64_t)H * W, ohw = (int64_t)OH * OW;
  const int runs = W / PX;
  const float t_l1 = g_l1 ? (float)((double)g_l1[0] / count) : 0.f;
  float sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) sd[c] = stdv[c];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const int iy = (int)(i / runs), ix0 = (int)(i % runs) * PX;
    const int64_t p = (int64_t)iy * W + ix0;
    float a[3][PX], b[3][PX], m[PX], d[3][PX];
    load_rgb_run<PX>(gen, hwc, n, hw, p, a);
    load_rgb_run<PX>(gt, false, n, hw, p, b);
    load_px<PX>(mask, n * hw + p, m);
    int ylo = 0, yhi = -1;
    if (gx) contributors(iy, H, OH, ylo, yhi);  // the rows: once for the run
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int ix = ix0 + j;
      float s[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[k][c] = 0.f;
      int xlo = 0, xhi = -1;
      if (gx) contributors(ix, W, OW, xlo, xhi);  // the columns: once for the three channels and the three streams
      for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = weight_on(lerp_of(oy, H, OH), iy);
        for (int ox = xlo; ox <= xhi; ++ox) {
          const float w = wy * weight_on(lerp_of(ox, W, OW), ix);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float* q = gx + ((((int64_t)k * N + n) * ohw) + (int64_t)oy * OW + ox) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[k][c] += w * (q[c] / sd[c]);
          }
        }
      }
      const float im = __fsub_rn(1.f, m[j]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float sgn = a[c][j] > b[c][j] ? 1.f : a[c][j] < b[c][j] ? -1.f : 0.f;
        d[c][j] = ((sgn * t_l1 + s[0][c]) + im * s[1][c]) + m[j] * s[2][c];
      }
    }
    store_rgb_run<PX>(d_gen, hwc, n, hw, p, d);  // the gradient in gen's own layout
  }
}

// workgroups per sample of the forward: enough for the larger of its two loops
inline int gan_fwd_gx(int64_t per_out, int64_t per_in) { return rows_for(per_out > per_in ? per_out : per_in, ROWS_PER_PLANE); }

}  // namespace

extern "C" int fmi_gan_image_head_fwd_f32(const float* gen, const float* gt, const float* src, const float* ref, const float* mask, const float* mean,
                                          const float* stdv, float* x_in, float* y_in, float* l1, int N, int H, int W, int OH, int OW, int gen_hwc,
                                          double* ws_part, int64_t ws_doubles, void* stream) {
  if (!gen || !gt || !src || !ref || !mask || !mean || !stdv || !x_in || !y_in || !l1 || !ws_part) return FMI_ERR_BAD_ARG;
  if ((gen_hwc != 0 && gen_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return FMI_ERR_BAD_ARG;
  const void* all[] = {gen, gt, src, ref, mask, mean, stdv, x_in, y_in, l1};
  for (const void* q : all)
    if (!al4(q)) return FMI_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(ws_part) & 7) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W, ohw = (int64_t)OH * OW;
  const bool vec_out = (OW & 3) == 0 && fmi_al16(x_in) && fmi_al16(y_in);
  const bool vec_in = (hw & 3) == 0 && fmi_al16(gen) && fmi_al16(gt);
  const int64_t per = vec_out ? ohw >> 2 : ohw;
  const int gx = gan_fwd_gx(per, vec_in ? hw >> 2 : hw);
  if (ws_doubles < (int64_t)N * gx) return FMI_ERR_BAD_ARG;  // one partial row per workgroup
  const dim3 grid(gx, N), block(256);
  if (vec_out)
    hipLaunchKernelGGL(gan_head_fwd_kernel<4>, grid, block, 0, (hipStream_t)stream, gen, gt, src, ref, mask, mean, stdv, x_in, y_in, ws_part, N, H, W, OH, OW,
                       per, gen_hwc != 0, vec_in);
  else
    hipLaunchKernelGGL(gan_head_fwd_kernel<1>, grid, block, 0, (hipStream_t)stream, gen, gt, src, ref, mask, mean, stdv, x_in, y_in, ws_part, N, H, W, OH, OW,
                       per, gen_hwc != 0, vec_in);
  hipLaunchKernelGGL(rows_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws_part, (int64_t)N * gx, 1, 3.0 * (double)N * (double)hw,
                     (double*)nullptr, l1);
  return fmi_launch_status();
}

extern "C" int fmi_gan_image_head_bwd_f32(const float* gen, const float* gt, const float* mask, const float* stdv, const float* gx, const float* g_l1,
                                          float* d_gen, int N, int H, int W, int OH, int OW, int gen_hwc, void* stream) {
  if (!gen || !gt || !mask || !stdv || !d_gen) return FMI_ERR_BAD_ARG;
  if ((gen_hwc != 0 && gen_hwc != 1) || N <= 0 || N > 65535 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return FMI_ERR_BAD_ARG;
  const void* all[] = {gen, gt, mask, stdv, gx, g_l1, d_gen};
  for (const void* q : all)
    if (!al4(q)) return FMI_ERR_BAD_ARG;
  const int64_t hw = (int64_t)H * W;
  const bool vec = (W & 3) == 0 && fmi_al16(gen) && fmi_al16(gt) && fmi_al16(mask) && fmi_al16(d_gen);
  const int64_t per = vec ? hw >> 2 : hw;
  const dim3 grid(rows_for(per, 1024), N), block(256);
  const double count = 3.0 * (double)N * (double)hw;
  if (vec)
    hipLaunchKernelGGL(gan_head_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, gen, gt, mask, stdv, gx, g_l1, d_gen, N, H, W, OH, OW, per, count, gen_hwc != 0);
  else
    hipLaunchKernelGGL(gan_head_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, gen, gt, mask, stdv, gx, g_l1, d_gen, N, H, W, OH, OW, per, count, gen_hwc != 0);
  return fmi_launch_status();
}
