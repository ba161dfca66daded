// bf16 body of the UNet mask detector (modules/unet/unet_parts.py): the bandwidth kernels between the bf16 convolutions of conv_bf16.hip
// and the bf16 BatchNorm kernels of norm.hip -- 2 x 2 max pooling, the upsample / pad / concat of Up in one pass, and the 2-class head.
// NHWC bf16 tensors (uint16_t = raw bits), C % 8 == 0: one thread moves 8 channels (16 bytes), fp32 arithmetic, round-to-nearest-even
// stores.  Parameters, logits and every reduction result stay fp32.  No atomics anywhere: both modes of fmi_set_deterministic run the
// same code.
#include "bf16x8.h"
#include "head.h"


// ---- 2 x 2 stride-2 max pooling, H and W even; the FIRST maximum of the window in row-major order wins and a later NaN replaces the
// running maximum (ATen's rule, pool.hip's maxpool_kernel): a NaN reaches the output and takes the gradient ----
__device__ __forceinline__ bool u_takes(float v, float t) { return v > t || v != v; }
__global__ void __launch_bounds__(256) maxpool2_bf16_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int H, int W, int C8, int64_t total) {
  const int OH = H >> 1, OW = W >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C8);
    int64_t r = i / C8;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH);
    const int64_t n = r / OH;
    const uint4* p = x + ((n * H + oy * 2) * W + ox * 2) * C8 + c;
    float v0[8], v1[8], v2[8], v3[8], m[8];
    bf_unpack8(p[0], v0);
    bf_unpack8(p[C8], v1);
    bf_unpack8(p[(int64_t)W * C8], v2);
    bf_unpack8(p[(int64_t)W * C8 + C8], v3);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = v0[e];
      if (u_takes(v1[e], t)) t = v1[e];
      if (u_takes(v2[e], t)) t = v2[e];
      if (u_takes(v3[e], t)) t = v3[e];
      m[e] = t;
    }
    y[i] = bf_trunc8(m);
  }
}
// one thread per WINDOW: x and gy are read once, the four gx pixels of the window are written (the loser pixels as zeros)
__global__ void __launch_bounds__(256) maxpool2_bwd_bf16_kernel(const uint4* __restrict__ x, const uint4* __restrict__ gy, uint4* __restrict__ gx, int H,
                                                                int W, int C8, int64_t total) {
  const int OH = H >> 1, OW = W >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C8);
    int64_t r = i / C8;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH);
    const int64_t n = r / OH;
    const int64_t o = ((n * H + oy * 2) * W + ox * 2) * C8 + c;
    float v0[8], v1[8], v2[8], v3[8], g[8], q[4][8];
    bf_unpack8(x[o], v0);
    bf_unpack8(x[o + C8], v1);
    bf_unpack8(x[o + (int64_t)W * C8], v2);
    bf_unpack8(x[o + (int64_t)W * C8 + C8], v3);
    bf_unpack8(gy[i], g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int arg = 0;
      float t = v0[e];
      if (u_takes(v1[e], t)) { t = v1[e]; arg = 1; }
      if (u_takes(v2[e], t)) { t = v2[e]; arg = 2; }
      if (u_takes(v3[e], t)) { t = v3[e]; arg = 3; }
#pragma unroll
      for (int a = 0; a < 4; ++a) q[a][e] = arg == a ? g[e] : 0.f;
    }
    gx[o] = bf_trunc8(q[0]);
    gx[o + C8] = bf_trunc8(q[1]);
    gx[o + (int64_t)W * C8] = bf_trunc8(q[2]);
    gx[o + (int64_t)W * C8 + C8] = bf_trunc8(q[3]);
  }
}
static int pool_args(const void* a, const void* b, const void* c, int N, int H, int W, int C) {
  if (!a || !b || !c || N <= 0 || H <= 0 || W <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || (H & 1) || (W & 1) || !fmi_al16(a) || !fmi_al16(b) || !fmi_al16(c)) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
extern "C" int fmi_maxpool2_bf16(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, void* stream) {
  const int rc = pool_args(x, y, y, N, H, W, C);
  if (rc) return rc;
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
  hipLaunchKernelGGL(maxpool2_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)y, H, W, C / 8,
                     total);
  return fmi_launch_status();
}
extern "C" int fmi_maxpool2_bwd_bf16(const uint16_t* x, const uint16_t* gy, uint16_t* gx, int N, int H, int W, int C, void* stream) {
  const int rc = pool_args(x, gy, gx, N, H, W, C);
  if (rc) return rc;
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
  hipLaunchKernelGGL(maxpool2_bwd_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (const uint4*)gy,
                     (uint4*)gx, H, W, C / 8, total);
  return fmi_launch_status();
}

// ---- Up (unet_parts.py:45-72) in one pass: bilinear x2 (align_corners=True) of x1 [N,h,w,C1], a zero border up to the skip's size
// (dy // 2 rows on top, dy - dy // 2 below; the same split left and right) and cat([skip, up], C) -> [N,H,W,C2+C1] ----
// Source position of output o along an axis in -> out = 2 in: o (in - 1) / (out - 1), kept as an integer quotient and remainder, so the
// interpolation weight carries two roundings (1 / den, the product: at most 2^-23 relative) and the forward and its adjoint use identical
// weights.
struct Up2Lerp {
  int i0;
  float l0, l1;
};
__device__ __forceinline__ Up2Lerp up2_lerp(int o, int in, float inv_den) {  // den = 2 in - 1, inv_den = 1 / den
  const int den = 2 * in - 1, q = o * (in - 1);
  Up2Lerp l;
  l.i0 = q / den;
  l.l1 = (float)(q - l.i0 * den) * inv_den;
  l.l0 = 1.f - l.l1;
  return l;
}
__global__ void __launch_bounds__(256) up2_cat_bf16_kernel(const uint4* __restrict__ x1, const uint4* __restrict__ skip, uint4* __restrict__ y, int h,
                                                           int w, int C1_8, int H, int W, int C2_8, int py0, int px0, int64_t total) {
  const int CT = C1_8 + C2_8;
  const float idy = 1.f / (float)(2 * h - 1), idx = 1.f / (float)(2 * w - 1);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % CT);
    const int64_t pix = i / CT;
    if (c < C2_8) {
      y[i] = skip[pix * C2_8 + c];
      continue;
    }
    const int xx = (int)(pix % W);
    const int64_t r = pix / W;
    const int yy = (int)(r % H);
    const int64_t n = r / H;
    const int uy = yy - py0, ux = xx - px0;
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)uy < (unsigned)(2 * h) && (unsigned)ux < (unsigned)(2 * w)) {
      const Up2Lerp ly = up2_lerp(uy, h, idy), lx = up2_lerp(ux, w, idx);
      const int y1 = ly.i0 + (ly.i0 < h - 1 ? 1 : 0), x1i = lx.i0 + (lx.i0 < w - 1 ? 1 : 0);
      const uint4* b = x1 + n * h * w * C1_8 + (c - C2_8);
      float v00[8], v01[8], v10[8], v11[8], o[8];
      bf_unpack8(b[((int64_t)ly.i0 * w + lx.i0) * C1_8], v00);
      bf_unpack8(b[((int64_t)ly.i0 * w + x1i) * C1_8], v01);
      bf_unpack8(b[((int64_t)y1 * w + lx.i0) * C1_8], v10);
      bf_unpack8(b[((int64_t)y1 * w + x1i) * C1_8], v11);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = ly.l0 * (lx.l0 * v00[e] + lx.l1 * v01[e]) + ly.l1 * (lx.l0 * v10[e] + lx.l1 * v11[e]);
      out = bf_pack8(o);
    }
    y[i] = out;
  }
}
// outputs o of an axis whose footprint {i0, i0 + 1} can contain input i: i0 in {i - 1, i}
__device__ __forceinline__ void up2_cands(int i, int in, int& lo, int& hi) {
  const int out = 2 * in;
  if (in == 1) {
    lo = 0, hi = out - 1;
    return;
  }
  lo = i > 0 ? ((i - 1) * (out - 1) + in - 2) / (in - 1) : 0;
  hi = ((i + 1) * (out - 1) - 1) / (in - 1);
  if (hi > out - 1) hi = out - 1;
}
// gskip = the first C2 channels of g (a copy); gx1 = the adjoint of the interpolation as a GATHER per input pixel: fp32 accumulation
// in a fixed order (rows of the footprint, each row's columns first), one bf16 store, nothing to zero
__global__ void __launch_bounds__(256) up2_cat_bwd_bf16_kernel(const uint4* __restrict__ g, uint4* __restrict__ gskip, uint4* __restrict__ gx1, int h,
                                                               int w, int C1_8, int H, int W, int C2_8, int py0, int px0, int64_t nskip,
                                                               int64_t total) {
  const int CT = C1_8 + C2_8;
  const float idy = 1.f / (float)(2 * h - 1), idx = 1.f / (float)(2 * w - 1);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (i < nskip) {
      gskip[i] = g[(i / C2_8) * CT + (i % C2_8)];
      continue;
    }
    const int64_t j = i - nskip;
    const int c = (int)(j % C1_8);
    int64_t r = j / C1_8;
    const int ix = (int)(r % w);
    r /= w;
    const int iy = (int)(r % h);
    const int64_t n = r / h;
    int ylo, yhi, xlo, xhi;
    up2_cands(iy, h, ylo, yhi);
    up2_cands(ix, w, xlo, xhi);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; ++oy) {
      const Up2Lerp ly = up2_lerp(oy, h, idy);
      const float wy = ly.i0 == iy ? ly.l0 : (ly.i0 + 1 == iy ? ly.l1 : 0.f);
      if (wy == 0.f) continue;
      float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const uint4* row = g + ((n * H + (oy + py0)) * W + px0) * CT + C2_8 + c;
      for (int ox = xlo; ox <= xhi; ++ox) {
        const Up2Lerp lx = up2_lerp(ox, w, idx);
        const float wx = lx.i0 == ix ? lx.l0 : (lx.i0 + 1 == ix ? lx.l1 : 0.f);
        if (wx == 0.f) continue;
        float gv[8];
        bf_unpack8(row[(int64_t)ox * CT], gv);
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = fmaf(wx, gv[e], t[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = fmaf(wy, t[e], s[e]);
    }
    gx1[j] = bf_pack8(s);
  }
}
static int up2_args(const void* a, const void* b, const void* c, int N, int h, int w, int C1, int H, int W, int C2) {
  if (!a || !b || !c || N <= 0 || h <= 0 || w <= 0 || C1 <= 0 || H <= 0 || W <= 0 || C2 <= 0) return FMI_ERR_BAD_ARG;
  if (H < 2 * h || W < 2 * w) return FMI_ERR_BAD_ARG;  // the border is never negative (unet_parts.py pads up to the skip's size)
  if (C1 % 8 != 0 || C2 % 8 != 0 || !fmi_al16(a) || !fmi_al16(b) || !fmi_al16(c)) return FMI_ERR_UNSUPPORTED;
  if (h > 16384 || w > 16384) return FMI_ERR_UNSUPPORTED;  // o (in - 1) stays an int
  return FMI_OK;
}
extern "C" int fmi_up2_cat_bf16(const uint16_t* x1, const uint16_t* skip, uint16_t* y, int N, int h, int w, int C1, int H, int W, int C2, void* stream) {
  const int rc = up2_args(x1, skip, y, N, h, w, C1, H, W, C2);
  if (rc) return rc;
  const int64_t total = (int64_t)N * H * W * ((C1 + C2) / 8);
  hipLaunchKernelGGL(up2_cat_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x1, (const uint4*)skip,
                     (uint4*)y, h, w, C1 / 8, H, W, C2 / 8, (H - 2 * h) / 2, (W - 2 * w) / 2, total);
  return fmi_launch_status();
}
extern "C" int fmi_up2_cat_bwd_bf16(const uint16_t* g, uint16_t* gskip, uint16_t* gx1, int N, int h, int w, int C1, int H, int W, int C2, void* stream) {
  const int rc = up2_args(g, gskip, gx1, N, h, w, C1, H, W, C2);
  if (rc) return rc;
  const int64_t nskip = (int64_t)N * H * W * (C2 / 8), total = nskip + (int64_t)N * h * w * (C1 / 8);
  hipLaunchKernelGGL(up2_cat_bwd_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)g, (uint4*)gskip,
                     (uint4*)gx1, h, w, C1 / 8, H, W, C2 / 8, (H - 2 * h) / 2, (W - 2 * w) / 2, nskip, total);
  return fmi_launch_status();
}

// ---- OutConv (1 x 1, C -> K <= 4): bf16 x [P,C], fp32 w [K][C] and b [K] -> fp32 logits [P,K] ----
// Eight lanes share a pixel: lane j adds channel chunks j, j + 8, ... in order (16-byte loads, consecutive lanes = consecutive chunks), the
// eight partial sums meet through three shuffles in a fixed order, the bias is added last.  The weights sit in LDS.
constexpr int HEAD_KMAX = 4, HEAD_CMAX = 1024;
template <int K>
__device__ __forceinline__ void head_logits(const uint4* __restrict__ x, const float* wl, const float* __restrict__ b, int64_t p, int C8, int sub,
                                            float (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  for (int c = sub; c < C8; c += 8) {
    float f[8];
    bf_unpack8(x[p * C8 + c], f);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[k] = fmaf(f[e], wl[(k * C8 + c) * 8 + e], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc[k] += __shfl_xor(acc[k], 1, 64);
    acc[k] += __shfl_xor(acc[k], 2, 64);
    acc[k] += __shfl_xor(acc[k], 4, 64);
    acc[k] += b[k];
  }
}
template <int K, bool ARGMAX>
__global__ void __launch_bounds__(256) head1x1_bf16_kernel(const uint4* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                           float* __restrict__ y, int64_t P, int C8) {
  __shared__ float wl[HEAD_KMAX * HEAD_CMAX];
  for (int i = threadIdx.x; i < K * C8 * 8; i += 256) wl[i] = w[i];
  __syncthreads();
  const int sub = threadIdx.x & 7;
  const int64_t groups = (P + 31) / 32;  // 32 pixels per workgroup and round; whole groups keep the shuffles uniform
  for (int64_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
    const int64_t p = gi * 32 + (threadIdx.x >> 3);
    const int64_t pc = p < P ? p : P - 1;
    float acc[K];
    head_logits<K>(x, wl, b, pc, C8, sub, acc);
    if (sub == 0 && p < P) {
      if (ARGMAX) {
        float best = acc[0];
        int bi = 0;
#pragma unroll
        for (int k = 1; k < K; ++k)
          if (acc[k] > best || (acc[k] != acc[k] && best == best)) best = acc[k], bi = k;  // fmi_argmax_channels_f32's rule
        y[p] = (float)bi;
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) y[p * K + k] = acc[k];
      }
    }
  }
}
static int head_args(const void* x, const void* w, const void* b, const void* y, int64_t P, int C, int K) {
  if (!x || !w || !b || !y || P <= 0 || C <= 0 || K <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || C > HEAD_CMAX || K > HEAD_KMAX || !fmi_al16(x) || !al4(w) || !al4(b) || !al4(y)) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
template <bool ARGMAX>
static int head_launch(const uint16_t* x, const float* w, const float* b, float* y, int64_t P, int C, int K, void* stream) {
  const int rc = head_args(x, w, b, y, P, C, K);
  if (rc) return rc;
  const dim3 grid(fmi_bw_grid((P + 31) / 32, 1)), blk(256);
  hipStream_t st = (hipStream_t)stream;
  const uint4* xv = (const uint4*)x;
  switch (K) {
    case 1: hipLaunchKernelGGL((head1x1_bf16_kernel<1, ARGMAX>), grid, blk, 0, st, xv, w, b, y, P, C / 8); break;
    case 2: hipLaunchKernelGGL((head1x1_bf16_kernel<2, ARGMAX>), grid, blk, 0, st, xv, w, b, y, P, C / 8); break;
    case 3: hipLaunchKernelGGL((head1x1_bf16_kernel<3, ARGMAX>), grid, blk, 0, st, xv, w, b, y, P, C / 8); break;
    default: hipLaunchKernelGGL((head1x1_bf16_kernel<4, ARGMAX>), grid, blk, 0, st, xv, w, b, y, P, C / 8); break;
  }
  return fmi_launch_status();
}
extern "C" int fmi_head1x1_bf16(const uint16_t* x, const float* w, const float* b, float* y, int64_t P, int C, int K, void* stream) {
  return head_launch<false>(x, w, b, y, P, C, K, stream);
}
extern "C" int fmi_head1x1_argmax_bf16(const uint16_t* x, const float* w, const float* b, float* mask, int64_t P, int C, int K, void* stream) {
  return head_launch<true>(x, w, b, mask, P, C, K, stream);
}

// gx[p][c] = sum_k g[p][k] w[k][c] (bf16);  gw[k][c] = sum_p g[p][k] x[p][c],  gb[k] = sum_p g[p][k] (fp32).  A thread keeps ONE channel
// chunk and walks the pixels of its workgroup's slice; the workgroup adds its threads in a fixed order and stores one partial row
// (doubles); head.h's finishing kernel adds the rows in order.
template <int K>
__global__ void __launch_bounds__(256) head1x1_bwd_bf16_kernel(const float* __restrict__ g, const uint4* __restrict__ x, const float* __restrict__ w,
                                                               uint4* __restrict__ gx, double* __restrict__ part_w, double* __restrict__ part_b,
                                                               int64_t P, int C8, int64_t rows_per_block) {
  __shared__ float lw[256][K * 8 + 1];  // +1: the column walk below strides by whole rows
  __shared__ float lb[256][K];
  const int cg = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > P) r1 = P;
  float aw[K][8], ab[K], wc[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ab[k] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) aw[k][e] = 0.f, wc[k][e] = rl < RL ? w[(k * C8 + cg) * 8 + e] : 0.f;
  }
  if (rl < RL) {
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      float xv[8], o[8], gk[K];
      bf_unpack8(x[r * C8 + cg], xv);
#pragma unroll
      for (int k = 0; k < K; ++k) gk[k] = g[r * K + k];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        ab[k] += gk[k];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          o[e] = fmaf(gk[k], wc[k][e], o[e]);
          aw[k][e] = fmaf(gk[k], xv[e], aw[k][e]);
        }
      }
      gx[r * C8 + cg] = bf_pack8(o);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    lb[threadIdx.x][k] = ab[k];
#pragma unroll
    for (int e = 0; e < 8; ++e) lw[threadIdx.x][k * 8 + e] = aw[k][e];
  }
  __syncthreads();
  const int nvw = K * C8 * 8;
  for (int i = threadIdx.x; i < nvw; i += 256) {  // i = k * C + channel
    const int k = i / (C8 * 8), ch = i - k * C8 * 8, c8 = ch >> 3, e = ch & 7;
    double t = 0.0;
    for (int l = 0; l < RL; ++l) t += (double)lw[l * C8 + c8][k * 8 + e];
    part_w[(int64_t)blockIdx.x * nvw + i] = t;
  }
  if ((int)threadIdx.x < K) {
    double t = 0.0;
    for (int l = 0; l < RL; ++l) t += (double)lb[l * C8][threadIdx.x];  // the cg = 0 thread of every pixel lane
    part_b[(int64_t)blockIdx.x * K + threadIdx.x] = t;
  }
}
extern "C" int fmi_head1x1_bwd_bf16(const float* g, const uint16_t* x, const float* w, uint16_t* gx, float* gw, float* gb, double* ws,
                                    int64_t ws_doubles, int64_t P, int C, int K, void* stream) {
  if (!g || !x || !w || !gx || !gw || !gb || !ws || P <= 0 || C <= 0 || K <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || C > HEAD_CMAX || K > HEAD_KMAX || !fmi_al16(x) || !fmi_al16(gx) || !al4(g) || !al4(w) || !al4(gw) || !al4(gb) ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return FMI_ERR_UNSUPPORTED;
  const int C8 = C / 8, nv = K * C + K;
  if (C8 > 256 || ws_doubles < nv) return FMI_ERR_UNSUPPORTED;
  int64_t blocks = ceil_div64(P, 256);
  const int64_t cap = ws_doubles / nv < 512 ? ws_doubles / nv : 512;
  if (blocks > cap) blocks = cap;
  const int64_t rpb = ceil_div64(P, blocks);
  blocks = ceil_div64(P, rpb);
  double* part_w = ws;
  double* part_b = ws + blocks * (int64_t)K * C;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), blk(256);
  const uint4* xv = (const uint4*)x;
  uint4* gxv = (uint4*)gx;
  switch (K) {
    case 1: hipLaunchKernelGGL(head1x1_bwd_bf16_kernel<1>, grid, blk, 0, st, g, xv, w, gxv, part_w, part_b, P, C8, rpb); break;
    case 2: hipLaunchKernelGGL(head1x1_bwd_bf16_kernel<2>, grid, blk, 0, st, g, xv, w, gxv, part_w, part_b, P, C8, rpb); break;
    case 3: hipLaunchKernelGGL(head1x1_bwd_bf16_kernel<3>, grid, blk, 0, st, g, xv, w, gxv, part_w, part_b, P, C8, rpb); break;
    default: hipLaunchKernelGGL(head1x1_bwd_bf16_kernel<4>, grid, blk, 0, st, g, xv, w, gxv, part_w, part_b, P, C8, rpb); break;
  }
  hipLaunchKernelGGL(plane_rows_finish_kernel<float>, dim3((K * C + 255) / 256), dim3(256), 0, st, (const double*)part_w, (int)blocks, 1, K * C, 1.0, gw);
  hipLaunchKernelGGL(plane_rows_finish_kernel<float>, dim3(1), dim3(256), 0, st, (const double*)part_b, (int)blocks, 1, K, 1.0, gb);
  return fmi_launch_status();
}
