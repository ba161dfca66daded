// StyleGAN2 decoder helpers on NHWC activations (stylegan2/model.py:187-369): the modulation is applied to the
// ACTIVATIONS (x * s[n,c] before the conv, * demod[n,o] after it), which is algebraically the reference's
// per-sample weight modulation (model.py:244-250) but lets every sample share one packed weight and one GEMM.
// All kernels are bandwidth-class.
#include "common.h"

// out[r] = sum_k x[r][k]^2  and its gradient gx[r][k] = 2 x[r][k] g[r]     (W^2 summed over the taps)
__global__ void __launch_bounds__(256) sqsum_last_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t rows, int k) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += x[r * k + j] * x[r * k + j];
    out[r] = s;
  }
}
extern "C" int fmi_sqsum_last_f32(const float* x, float* out, int64_t rows, int k, void* stream) {
  if (!x || !out || rows <= 0 || k <= 0) return FMI_ERR_BAD_ARG;
  hipLaunchKernelGGL(sqsum_last_kernel, dim3(fmi_bw_grid(rows, 256)), dim3(256), 0, (hipStream_t)stream, x, out, rows, k);
  return fmi_launch_status();
}
__global__ void __launch_bounds__(256) sqsum_last_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             float* __restrict__ gx, int64_t total, int k) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) gx[i] = 2.f * x[i] * g[i / k];
}
extern "C" int fmi_sqsum_last_bwd_f32(const float* x, const float* g, float* gx, int64_t rows, int k, void* stream) {
  if (!x || !g || !gx || rows <= 0 || k <= 0) return FMI_ERR_BAD_ARG;
  const int64_t total = rows * k;
  hipLaunchKernelGGL(sqsum_last_bwd_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, g, gx, total, k);
  return fmi_launch_status();
}

// backward of y = lrelu(x + bias[c] + nw*noise[p]) * scale:  gx = g * scale * (y > 0 ? 1 : alpha);  gnw += sum gx*noise
__global__ void __launch_bounds__(256) noise_bias_act_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                                 const float* __restrict__ noise, float* __restrict__ gx,
                                                                 float* __restrict__ gnw, int64_t total, int C, float alpha,
                                                                 float scale) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float v = g[i] * scale * (y[i] > 0.f ? 1.f : alpha);
    gx[i] = v;
    if (noise) acc += v * noise[i / C];
  }
  if (noise && gnw) {
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) atomicAdd(gnw, acc);
  }
}
__global__ void __launch_bounds__(256) noise_bias_act_bwd_vec_kernel(const float4* __restrict__ g, const float4* __restrict__ y,
                                                                     const float* __restrict__ noise, float4* __restrict__ gx,
                                                                     float* __restrict__ gnw, int64_t total4, int C4, float alpha,
                                                                     float scale) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    float4 v = g[i];
    const float4 o = y[i];
    v.x *= scale * (o.x > 0.f ? 1.f : alpha);
    v.y *= scale * (o.y > 0.f ? 1.f : alpha);
    v.z *= scale * (o.z > 0.f ? 1.f : alpha);
    v.w *= scale * (o.w > 0.f ? 1.f : alpha);
    gx[i] = v;
    if (noise) acc += ((v.x + v.y) + (v.z + v.w)) * noise[i / C4];
  }
  if (noise && gnw) {
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) atomicAdd(gnw, acc);
  }
}
extern "C" int fmi_noise_bias_act_bwd_f32(const float* g, const float* y, const float* noise, float* gx, float* gnw,
                                          int64_t pixels, int C, float alpha, float scale, void* stream) {
  if (!g || !y || !gx || pixels <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 4 == 0 && ((((uintptr_t)g) | ((uintptr_t)y) | ((uintptr_t)gx)) & 15) == 0) {
    const int64_t total4 = pixels * (C / 4);
    int grid = (fmi_det() && noise && gnw) ? 1 : fmi_bw_grid(total4, 256 * 4);  // reproducible mode: one block sums the noise-weight gradient
    if (grid > 1024) grid = 1024;  // one atomic per block on a single address
    hipLaunchKernelGGL(noise_bias_act_bwd_vec_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (const float4*)y,
                       noise, (float4*)gx, gnw, total4, C / 4, alpha, scale);
    return fmi_launch_status();
  }
  const int64_t total = pixels * C;
  hipLaunchKernelGGL(noise_bias_act_bwd_kernel, dim3((fmi_det() && noise && gnw) ? 1 : fmi_bw_grid(total, 256 * 4)), dim3(256), 0, (hipStream_t)stream, g, y, noise,
                     gx, gnw, total, C, alpha, scale);
  return fmi_launch_status();
}

// upfirdn2d on NHWC tensors (minor dimension = channels): same semantics as fmi_upfirdn2d_f32 per (n, c) plane
__device__ __forceinline__ int fdiv_i(int a, int b) {
  int q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}
__global__ void __launch_bounds__(256) upfirdn2d_nhwc_kernel(const float* __restrict__ in, const float* __restrict__ kernel,
                                                             float* __restrict__ out, int in_h, int in_w, int C, int out_h,
                                                             int out_w, int kh, int kw, int up_x, int up_y, int down_x,
                                                             int down_y, int pad_x0, int pad_y0, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int ox = (int)(r % out_w);
    r /= out_w;
    const int oy = (int)(r % out_h);
    const int n = (int)(r / out_h);
    const int uy0 = oy * down_y - pad_y0, ux0 = ox * down_x - pad_x0;
    int ky0 = (-uy0) % up_y, kx0 = (-ux0) % up_x;
    if (ky0 < 0) ky0 += up_y;
    if (kx0 < 0) kx0 += up_x;
    float acc = 0.f;
    for (int ky = ky0; ky < kh; ky += up_y) {
      const int iy = (uy0 + ky) / up_y;
      if ((unsigned)iy >= (unsigned)in_h) continue;
      for (int kx = kx0; kx < kw; kx += up_x) {
        const int ix = (ux0 + kx) / up_x;
        if ((unsigned)ix >= (unsigned)in_w) continue;
        acc += in[(((int64_t)n * in_h + iy) * in_w + ix) * C + c] * kernel[(kh - 1 - ky) * kw + (kw - 1 - kx)];
      }
    }
    out[i] = acc;
  }
}
// Vector form for the decoder's Blur (op/upfirdn2d.py:142-147 with up = down = 1: StyledConv up-convolutions, model.py:52-68, and
// their gradients): C % 4 == 0, one thread per (2 adjacent output pixels, 4 channels).  The KH x (KW+1) input window of the
// pair is read once as 16-byte loads (consecutive threads = consecutive channel chunks: coalesced), the taps are wave-uniform
// scalars.  Algorithmic traffic = in + out bytes; the window overlap between neighbouring threads is served by L1/L2.
template <int KH, int KW>
__global__ void __launch_bounds__(256) upfirdn2d_nhwc_fir_kernel(const float* __restrict__ in, const float* __restrict__ kernel,
                                                                 float* __restrict__ out, int in_h, int in_w, int C4, int out_h,
                                                                 int out_w, int pad_x0, int pad_y0, int total) {
  float kf[KH][KW];  // flipped taps: out[oy][ox] = sum_{a,b} in[oy - pad_y0 + a][ox - pad_x0 + b] * kernel[KH-1-a][KW-1-b]
#pragma unroll
  for (int a = 0; a < KH; ++a)
#pragma unroll
    for (int b = 0; b < KW; ++b) kf[a][b] = kernel[(KH - 1 - a) * KW + (KW - 1 - b)];
  const int pw = (out_w + 1) >> 1;  // pixel pairs per row
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c4 = i % C4;
    int r = i / C4;
    const int px = r % pw;
    r /= pw;
    const int oy = r % out_h, n = r / out_h;
    const int ox = 2 * px;
    const int iy0 = oy - pad_y0, ix0 = ox - pad_x0;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    const float4* base = reinterpret_cast<const float4*>(in) + (int64_t)n * in_h * in_w * C4 + c4;
#pragma unroll
    for (int a = 0; a < KH; ++a) {
      const int iy = iy0 + a;
      if ((unsigned)iy >= (unsigned)in_h) continue;
      const float4* row = base + (int64_t)iy * in_w * C4;
#pragma unroll
      for (int b = 0; b <= KW; ++b) {
        const int ix = ix0 + b;
        if ((unsigned)ix >= (unsigned)in_w) continue;
        const float4 v = row[(int64_t)ix * C4];
        if (b < KW) {
          const float k0 = kf[a][b];
          a0.x = fmaf(v.x, k0, a0.x), a0.y = fmaf(v.y, k0, a0.y), a0.z = fmaf(v.z, k0, a0.z), a0.w = fmaf(v.w, k0, a0.w);
        }
        if (b > 0) {
          const float k1 = kf[a][b - 1];
          a1.x = fmaf(v.x, k1, a1.x), a1.y = fmaf(v.y, k1, a1.y), a1.z = fmaf(v.z, k1, a1.z), a1.w = fmaf(v.w, k1, a1.w);
        }
      }
    }
    float4* o = reinterpret_cast<float4*>(out) + ((int64_t)(n * out_h + oy) * out_w + ox) * C4 + c4;
    o[0] = a0;
    if (ox + 1 < out_w) o[C4] = a1;
  }
}

// column-run FIR shared with the bf16 path (sg2_bf16.hip); returns 0 when it does not apply
extern "C" int fmi_internal_fir_run_launch(const void* in, const float* kernel, void* out, int N, int in_h, int in_w, int CV, int out_h,
                                           int out_w, int k, int pad_x0, int pad_y0, int bf16, void* stream);
extern "C" int fmi_upfirdn2d_nhwc_f32(const float* in, const float* kernel, float* out, int N, int in_h, int in_w, int C,
                                      int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                                      int pad_y0, int pad_y1, void* stream) {
  if (!in || !kernel || !out || N <= 0 || in_h <= 0 || in_w <= 0 || C <= 0 || kh <= 0 || kw <= 0) return FMI_ERR_BAD_ARG;
  if (up_x <= 0 || up_y <= 0 || down_x <= 0 || down_y <= 0) return FMI_ERR_BAD_ARG;
  const int fh = in_h * up_y + pad_y0 + pad_y1 - kh, fw = in_w * up_x + pad_x0 + pad_x1 - kw;
  if (fh < 0 || fw < 0) return FMI_ERR_BAD_ARG;
  const int out_h = fh / down_y + 1, out_w = fw / down_x + 1;
  const int64_t total = (int64_t)N * out_h * out_w * C;
  if (up_x == 1 && up_y == 1 && down_x == 1 && down_y == 1 && C % 4 == 0 && kh == kw && (kh == 4 || kh == 3 || kh == 2) &&
      (((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
    if (fmi_internal_fir_run_launch(in, kernel, out, N, in_h, in_w, C / 4, out_h, out_w, kh, pad_x0, pad_y0, 0, stream)) return fmi_launch_status();
    const int64_t tv = (int64_t)N * out_h * ((out_w + 1) / 2) * (C / 4);
    if (tv < (1ll << 31) && (int64_t)N * in_h * in_w * C < (1ll << 40)) {
      const int grid = fmi_bw_grid(tv, 256);
#define FIR_LAUNCH(K_)                                                                                                              \
  hipLaunchKernelGGL((upfirdn2d_nhwc_fir_kernel<K_, K_>), dim3(grid), dim3(256), 0, (hipStream_t)stream, in, kernel, out, in_h, in_w, \
                     C / 4, out_h, out_w, pad_x0, pad_y0, (int)tv)
      if (kh == 4) FIR_LAUNCH(4);
      else if (kh == 3) FIR_LAUNCH(3);
      else FIR_LAUNCH(2);
#undef FIR_LAUNCH
      return fmi_launch_status();
    }
  }
  hipLaunchKernelGGL(upfirdn2d_nhwc_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, in, kernel, out, in_h,
                     in_w, C, out_h, out_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, total);
  return fmi_launch_status();
}
