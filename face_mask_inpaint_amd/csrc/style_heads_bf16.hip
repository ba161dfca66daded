// Inference form of the map2style heads of the pSp encoder (modules/psp/encoders/psp_encoders.py:13-37, :97-98, :140-151 and
// stylegan2/model.py EqualLinear of the reference) on bf16 NHWC activations.  The G heads of one pyramid level run together, one launch
// per layer:
//   * fmi_conv2d_grouped_fwd_bf16: G convolutions (3x3 stride 2 + LeakyReLU, or the 1x1 that is the heads' EqualLinear) in one call.
//     Calls with many output rows go to the tile kernel of conv_bf16.hip with its grouped output stage; calls with at most
//     FMI_STYLE_SKINNY_ROWS rows -- at batch 8 the layers that produce 4^2, 2^2 and 1^2 maps and the linear: 128, 32, 8 and 8 rows --
//     cost what reading each head's weights costs, and take the weight-streaming kernel below.
//   * fmi_fpn_merge_bf16: _upsample_add and the fp32 -> bf16 hand-over of a level map in one pass.
//   * fmi_fpn_merge_in_bf16 and fmi_mask_blend_bf16: _upsample_add from bf16 maps and the mask blend of the pyramid levels
//     (psp_encoders.py:135-138) for the bf16 neck (psp_encoders.neck_bf16), which hands the heads bf16 level maps.
// Parameters and accumulation are fp32, every bf16 value is rounded once, nothing is accumulated through atomics.
#include "bf16x8.h"

typedef __bf16 sh_bf16x8 __attribute__((ext_vector_type(8)));
typedef float sh_f32x4 __attribute__((ext_vector_type(4)));

// conv_bf16.hip: the tile path (conv_bf16_kernel with the grouped output stage EpGroupB); the arguments are checked here
int fmi_conv_bf16_grouped_tiles(const fmi_conv_desc* d, int G, int64_t x_off, int64_t w_off, const uint16_t* x, const uint16_t* wnk,
                                const float* bias, float slope, uint16_t* y, void* stream);

// ---- weight-streaming kernel ----------------------------------------------------------------------------------------------------------
// grid (K / 16, G, ceil(rows / 64)), four waves.  A workgroup owns 16 output columns of one group and up to 64 output rows (= pixels, in
// [n][oy][ox] order).  The reduction over (tap, channel) is cut into slices of 32; wave w takes slices w, w + 4, ... and multiplies each
// with v_mfma_f32_16x16x32_bf16, whose operand layout is what lies in memory: lane l supplies 8 consecutive reduction elements of row /
// column l & 15 starting at 8 (l >> 4) -- 8 consecutive channels of one NHWC pixel and 8 consecutive elements of wnk[k][tap][:], one
// 16-byte load each, no LDS staging.  Padding taps and rows beyond `rows` supply zeros.  The four partial accumulators meet through LDS
// and wave 0 adds them in wave order, applies bias and activation and stores.
struct SkinnyArgs {
  const bf16_t* x;
  const bf16_t* w;
  const float* bias;
  bf16_t* y16;
  float* y32;
  int rows, H, W, OH, OW, C, K, kk, stride, pad, xcs, ycs;
  int64_t x_off;
  float slope;
};
constexpr int SK_UNROLL = 4;  // slices in flight per wave: 4 weight loads and up to 16 activation loads before the first MFMA

__global__ void __launch_bounds__(256) style_skinny_kernel(SkinnyArgs a) {
  __shared__ float red[3][4][4][64];  // [wave 1..3][row block][register][lane]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int k0 = blockIdx.x * 16, g = blockIdx.y, r0 = blockIdx.z * 64;
  const int left = a.rows - r0;
  const int nrb = left >= 64 ? 4 : (left + 15) >> 4;  // 16-row blocks of this workgroup (uniform)
  const int taps = a.kk * a.kk, spt = a.C >> 5, nsl = taps * spt;

  int iy0[4], ix0[4];
  int64_t pix0[4];
  bool rv[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int row = r0 + rb * 16 + l15;
    rv[rb] = rb < nrb && row < a.rows;
    const int rr = rv[rb] ? row : 0;
    const int n = rr / (a.OH * a.OW), rem = rr - n * (a.OH * a.OW);
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    iy0[rb] = oy * a.stride - a.pad;
    ix0[rb] = ox * a.stride - a.pad;
    pix0[rb] = (int64_t)n * a.H * a.W;
  }
  const bf16_t* const wp = a.w + ((int64_t)g * a.K + k0 + l15) * taps * a.C + lq * 8;
  const bf16_t* const xp = a.x + (int64_t)g * a.x_off + lq * 8;

  sh_f32x4 acc[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) acc[rb] = sh_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s0 = wid; s0 < nsl; s0 += 4 * SK_UNROLL) {
    sh_bf16x8 fb[SK_UNROLL], fa[SK_UNROLL][4];
    bool live[SK_UNROLL];
#pragma unroll
    for (int u = 0; u < SK_UNROLL; ++u) {
      const int s = s0 + 4 * u;
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      live[u] = false;
      fb[u] = *reinterpret_cast<const sh_bf16x8*>(&z);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) fa[u][rb] = *reinterpret_cast<const sh_bf16x8*>(&z);
      if (s >= nsl) continue;  // uniform
      const int tap = s / spt, c0 = (s - tap * spt) << 5;
      const int ty = tap / a.kk, tx = tap - ty * a.kk;
      bool ok[4], any = false;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const int iy = iy0[rb] + ty, ix = ix0[rb] + tx;
        ok[rb] = rv[rb] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        any = any || ok[rb];
      }
      if (__ballot(any) == 0ull) continue;  // a tap that is padding for every row of the workgroup: its weights are not read (uniform)
      live[u] = true;
      fb[u] = *reinterpret_cast<const sh_bf16x8*>(wp + (int64_t)tap * a.C + c0);
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        if (ok[rb]) {
          const int64_t pix = pix0[rb] + (int64_t)(iy0[rb] + ty) * a.W + (ix0[rb] + tx);
          fa[u][rb] = *reinterpret_cast<const sh_bf16x8*>(xp + pix * a.xcs + c0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < SK_UNROLL; ++u) {
      if (!live[u]) continue;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
        if (rb < nrb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[u][rb], fb[u], acc[rb], 0, 0, 0);
    }
  }

  if (wid > 0) {
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wid - 1][rb][e][lane] = acc[rb][e];
  }
  __syncthreads();
  if (wid != 0) return;
  const int col = k0 + l15;  // of the group
  const float b = a.bias ? a.bias[(int64_t)g * a.K + col] : 0.f;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    if (rb >= nrb) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = r0 + rb * 16 + lq * 4 + e;  // accumulator register e of lane l: row 4 (l >> 4) + e, column l & 15
      if (row >= a.rows) continue;
      float v = ((acc[rb][e] + red[0][rb][e][lane]) + red[1][rb][e][lane]) + red[2][rb][e][lane];
      v += b;
      v = v > 0.f ? v : a.slope * v;
      const int64_t o = (int64_t)row * a.ycs + (int64_t)g * a.K + col;
      if (a.y32) a.y32[o] = v;
      else a.y16[o] = (bf16_t)bf_round(v);
    }
  }
}

extern "C" int fmi_conv2d_grouped_fwd_bf16(const fmi_conv_desc* d, int G, int64_t x_group_off, const uint16_t* x, const uint16_t* wnk,
                                           const float* bias, float slope, uint16_t* y16, float* y32, void* stream) {
  if (!d || !x || !wnk || G <= 0 || (y16 != nullptr) == (y32 != nullptr)) return FMI_ERR_BAD_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0) return FMI_ERR_BAD_ARG;
  if (x_group_off != 0 && x_group_off != d->C) return FMI_ERR_BAD_ARG;
  if (d->OH != (d->H + 2 * d->pad - d->kh) / d->stride + 1 || d->OW != (d->W + 2 * d->pad - d->kw) / d->stride + 1 || d->OH <= 0 || d->OW <= 0)
    return FMI_ERR_BAD_ARG;
  if ((int64_t)d->x_cstride < (int64_t)(G - 1) * x_group_off + d->C || (int64_t)d->y_cstride < (int64_t)G * d->K) return FMI_ERR_BAD_ARG;
  const bool k3 = d->kh == 3 && d->kw == 3 && d->pad == 1 && d->stride == 2, k1 = d->kh == 1 && d->kw == 1 && d->pad == 0 && d->stride == 1;
  if (!(k3 || k1) || d->dil > 1 || d->pad_mode != 0 || d->C % 64 != 0 || d->K % 64 != 0 || (y32 && !k1)) return FMI_ERR_UNSUPPORTED;
  if (d->x_cstride % 8 != 0 || d->y_cstride % 8 != 0 || !fmi_al16(x) || !fmi_al16(wnk) || !fmi_al16(bias) || !fmi_al16(y16) || !fmi_al16(y32))
    return FMI_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)d->N * d->OH * d->OW;
  if ((int64_t)d->N * d->H * d->W > 0x7fffffffLL / 2 || rows > 0x7fffffffLL / 2 || (int64_t)G * d->K > 0x3fffffffLL || G > 65535 ||
      (int64_t)d->kh * d->kw * d->C > 0x3fffffffLL)
    return FMI_ERR_UNSUPPORTED;
  const int64_t w_off = (int64_t)d->K * d->kh * d->kw * d->C;
  if (rows > FMI_STYLE_SKINNY_ROWS && y16) {
    if (x_group_off == 0) {  // one convolution with G*K output columns: the stacked packs are its weight as they lie
      fmi_conv_desc one = *d;
      one.K = G * d->K;
      return fmi_conv_bf16_grouped_tiles(&one, 1, 0, 0, x, wnk, bias, slope, y16, stream);
    }
    return fmi_conv_bf16_grouped_tiles(d, G, x_group_off, w_off, x, wnk, bias, slope, y16, stream);
  }
  const int64_t zb = (rows + 63) / 64;
  if (zb > 65535) return FMI_ERR_UNSUPPORTED;
  SkinnyArgs a{x, wnk, bias, y16, y32, (int)rows, d->H, d->W, d->OH, d->OW, d->C, d->K, d->kh, d->stride, d->pad, d->x_cstride, d->y_cstride,
               x_group_off, slope};
  hipLaunchKernelGGL(style_skinny_kernel, dim3((unsigned)(d->K / 16), (unsigned)G, (unsigned)zb), dim3(256), 0, (hipStream_t)stream, a);
  return fmi_launch_status();
}

// ---- FPN merge --------------------------------------------------------------------------------------------------------------------------
// one thread = 8 channels of one output pixel.  align_corners=True: source coordinate y (CH - 1) / (H - 1), split into its integer part
// and the two weights by integer arithmetic -- rem / (H - 1) and (H - 1 - rem) / (H - 1), one rounding each -- so the weights carry no
// error that grows with the coordinate.
// TIN is the element type of lateral and coarse: float (fmi_fpn_merge_bf16) or bf16 bits (fmi_fpn_merge_in_bf16, widened exactly).
__device__ __forceinline__ void fpn_load8(const float* p, float (&f)[8]) { bf_load8f(p, f); }
__device__ __forceinline__ void fpn_load8(const uint16_t* p, float (&f)[8]) { bf_unpack8(*reinterpret_cast<const uint4*>(p), f); }
template <typename TIN>
__global__ void __launch_bounds__(256) fpn_merge_kernel(const TIN* __restrict__ lat, const TIN* __restrict__ coarse, float* __restrict__ p32,
                                                        uint4* __restrict__ p16, int H, int W, int CH, int CW, int C8, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    const int64_t pix = i / C8;
    float f[8];
    fpn_load8(lat + i * 8, f);
    if (coarse) {
      const int ox = (int)(pix % W);
      const int64_t t = pix / W;
      const int oy = (int)(t % H);
      const int64_t n = t / H;
      const int dy = H > 1 ? H - 1 : 1, dx = W > 1 ? W - 1 : 1;
      const int ny = oy * (CH - 1), nx = ox * (CW - 1);
      const int y0 = ny / dy, x0 = nx / dx, ry = ny - y0 * dy, rx = nx - x0 * dx;
      const int y1 = y0 + 1 < CH ? y0 + 1 : CH - 1, x1 = x0 + 1 < CW ? x0 + 1 : CW - 1;
      const float fy = (float)ry / (float)dy, gy = (float)(dy - ry) / (float)dy, fx = (float)rx / (float)dx, gx = (float)(dx - rx) / (float)dx;
      const TIN* base = coarse + (n * CH * CW) * (int64_t)C8 * 8 + c8 * 8;
      float a00[8], a01[8], a10[8], a11[8];
      fpn_load8(base + ((int64_t)y0 * CW + x0) * C8 * 8, a00);
      fpn_load8(base + ((int64_t)y0 * CW + x1) * C8 * 8, a01);
      fpn_load8(base + ((int64_t)y1 * CW + x0) * C8 * 8, a10);
      fpn_load8(base + ((int64_t)y1 * CW + x1) * C8 * 8, a11);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += gy * (gx * a00[e] + fx * a01[e]) + fy * (gx * a10[e] + fx * a11[e]);
    }
    if (p32) {
      float4* o = reinterpret_cast<float4*>(p32 + i * 8);
      o[0] = make_float4(f[0], f[1], f[2], f[3]);
      o[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
    p16[i] = bf_pack8(f);
  }
}

extern "C" int fmi_fpn_merge_bf16(const float* lateral, const float* coarse, float* p32, uint16_t* p16, int N, int H, int W, int CH, int CW, int C,
                                  void* stream) {
  if (!lateral || !p16 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (coarse && (CH <= 0 || CW <= 0))) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(lateral) || !fmi_al16(coarse) || !fmi_al16(p32) || !fmi_al16(p16)) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)H * CH > 0x7fffffffLL || (int64_t)W * CW > 0x7fffffffLL) return FMI_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)N * H * W * (C / 8);
  hipLaunchKernelGGL(fpn_merge_kernel<float>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, lateral, coarse, p32, (uint4*)p16, H, W,
                     CH, CW, C / 8, total);
  return fmi_launch_status();
}

// the same merge from bf16 lateral and coarse maps (the lateral convolution's and the level above's bf16 outputs): same integer bilinear
// weights, fp32 arithmetic, one rounding; there is no fp32 output and no plain-conversion form (a bf16 map needs no hand-over)
extern "C" int fmi_fpn_merge_in_bf16(const uint16_t* lateral, const uint16_t* coarse, uint16_t* p16, int N, int H, int W, int CH, int CW, int C,
                                     void* stream) {
  if (!lateral || !coarse || !p16 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || CH <= 0 || CW <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(lateral) || !fmi_al16(coarse) || !fmi_al16(p16)) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)H * CH > 0x7fffffffLL || (int64_t)W * CW > 0x7fffffffLL) return FMI_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)N * H * W * (C / 8);
  hipLaunchKernelGGL(fpn_merge_kernel<uint16_t>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, lateral, coarse, (float*)nullptr,
                     (uint4*)p16, H, W, CH, CW, C / 8, total);
  return fmi_launch_status();
}

// ---- mask blend (psp_encoders.py:135-138) -----------------------------------------------------------------------------------------------
// y = bf16(m r + (1 - m) c) from bf16 r, c [rows][C] and fp32 m [rows], one thread = 8 channels of one pixel.  fma(m, r, (1 - m) c) in
// fp32: m == 1 leaves r and m == 0 leaves c, and a bf16 value survives its own rounding, so both return their operand bit for bit.
__global__ void __launch_bounds__(256) mask_blend_kernel(const uint4* __restrict__ r, const uint4* __restrict__ c, const float* __restrict__ m,
                                                         uint4* __restrict__ y, int C8, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float mk = m[i / C8], om = 1.f - mk;
    float a[8], b[8];
    bf_unpack8(r[i], a);
    bf_unpack8(c[i], b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = mk == 1.f ? a[e] : (mk == 0.f ? b[e] : fmaf(mk, a[e], om * b[e]));  // the selects keep a -0's sign
    y[i] = bf_pack8(a);
  }
}
extern "C" int fmi_mask_blend_bf16(const uint16_t* r, const uint16_t* c, const float* m, uint16_t* y, int64_t rows, int C, void* stream) {
  if (!r || !c || !m || !y || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(r) || !fmi_al16(c) || !fmi_al16(y) || ((uintptr_t)m & 3) != 0 || rows > 0x7fffffffffffLL / C) return FMI_ERR_UNSUPPORTED;
  const int64_t total = rows * (C / 8);
  hipLaunchKernelGGL(mask_blend_kernel, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const uint4*)r, (const uint4*)c, m, (uint4*)y,
                     C / 8, total);
  return fmi_launch_status();
}
