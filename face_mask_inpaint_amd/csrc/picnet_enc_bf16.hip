// Inference form of the PICNet ResEncoder (base_function.py:242-305 of the reference: ResBlock with norm 'none' and
// ResBlockEncoderOptimized) on bf16 NHWC activations: the layers fmi_conv2d_fwd_chan_bf16 does not take, and what lies between the
// convolutions of a block.
//   * the stem's first convolution: fp32 image with C <= 4 -> bf16, bias + LeakyReLU in the output stage (fp32 FMAs);
//   * the 32-channel layers (3x3 pad 1 or 1x1 pad 0, K = 32 or 64): one bf16 MFMA pair per tap, the whole weight set in registers;
//   * the block tail: main + shortcut [, 2x2 mean], written raw, LeakyReLU'd and / or in fp32 in one pass;
//   * the stem's tail: pool2(h) + bypass1x1(pool2(img)) + bias, the three-term 1x1 convolution evaluated in the tail itself.
// Parameters and arithmetic are fp32, every stored bf16 value is rounded once (to nearest even), nothing is accumulated through atomics:
// every result is bit-reproducible.  One thread of the element-wise kernels moves 8 channels (16-byte loads and stores).
#include "bf16x8.h"
#include "x6.h"

__device__ __forceinline__ float enc_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

static int enc_check_desc(const fmi_conv_desc* d) {
  if (!d) return FMI_ERR_BAD_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0)
    return FMI_ERR_BAD_ARG;
  if (d->stride != 1 || d->dil > 1 || d->pad_mode != 0 || d->kh != d->kw) return FMI_ERR_UNSUPPORTED;
  if (d->OH != d->H + 2 * d->pad - d->kh + 1 || d->OW != d->W + 2 * d->pad - d->kw + 1) return FMI_ERR_BAD_ARG;
  if (d->OH != d->H || d->OW != d->W) return FMI_ERR_UNSUPPORTED;  // 3x3 pad 1 or 1x1 pad 0: the map keeps its extent
  if (d->x_cstride != d->C || d->y_cstride != d->K) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)d->N * d->H * d->W > 0x7fffffffLL / 2) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}

// ---- the stem's conv1: y = lrelu(conv3x3(x) + b, slope), x fp32 [N,H,W,C <= 4], wf fp32 [9][C][K], y bf16 [N,H,W,K] --------------
// One thread = 8 output channels of one pixel; the weights sit in LDS padded to 4 input channels, the 27 (36) taps are one fma chain.
template <int K>
__global__ void __launch_bounds__(256) enc_thin_in_kernel(const float* __restrict__ x, const float* __restrict__ wf, const float* __restrict__ bias,
                                                          uint4* __restrict__ y, int H, int W, int C, float slope, int64_t total) {
  __shared__ __attribute__((aligned(16))) float wl[9 * 4 * K];
  __shared__ __attribute__((aligned(16))) float bl[K];
  for (int i = threadIdx.x; i < 9 * 4 * K; i += 256) {
    const int k = i % K, c = (i / K) & 3, t = i / (4 * K);
    wl[i] = c < C ? wf[((int64_t)t * C + c) * K + k] : 0.f;
  }
  for (int i = threadIdx.x; i < K; i += 256) bl[i] = bias ? bias[i] : 0.f;
  __syncthreads();
  constexpr int K8 = K / 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % K8);
    const int64_t pix = i / K8;
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;  // zero padding
      const float* xp = x + (pix + (int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * C;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        const float xv = xp[c];
        float w[8];
        bf_load8f(wl + (t * 4 + c) * K + c8 * 8, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(xv, w[e], acc[e]);
      }
    }
    float b[8];
    bf_load8f(bl + c8 * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = enc_lrelu(acc[e] + b[e], slope);
    y[i] = bf_pack8(acc);
  }
}
extern "C" int fmi_conv2d_thin_in_fwd_bf16(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias, float slope, uint16_t* y,
                                           void* stream) {
  int rc = enc_check_desc(d);
  if (rc) return rc;
  if (!x || !wf || !y) return FMI_ERR_BAD_ARG;
  if (d->C > 4 || (d->K != 32 && d->K != 64) || d->kh != 3 || d->pad != 1) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)wf | (uintptr_t)bias) & 3) != 0 || !fmi_al16(y)) return FMI_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)d->N * d->H * d->W * (d->K / 8);
  const dim3 grid(fmi_bw_grid(total, 256 * 2)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (d->K == 32) hipLaunchKernelGGL(enc_thin_in_kernel<32>, grid, block, 0, st, x, wf, bias, (uint4*)y, d->H, d->W, d->C, slope, total);
  else hipLaunchKernelGGL(enc_thin_in_kernel<64>, grid, block, 0, st, x, wf, bias, (uint4*)y, d->H, d->W, d->C, slope, total);
  return fmi_launch_status();
}

// ---- the pSp encoder's stem in one launch (psp_encoders.py:59-61 and block 0's first BatchNorm, helpers.py:86 / :108) ----------------
// a = prelu(conv3x3(x) * scale + shift, slope), y = bf16(a), z = bf16(a * scale0 + shift0).  enc_thin_in_kernel's layout -- the weights in
// LDS padded to 4 input channels, the five per-channel vectors beside them ((36 + 5) K floats, dynamic: K is a run-time value), one
// thread = 8 output channels, one fma chain over the 27 (36) taps, 16-byte stores -- but a thread carries P pixels through the chain: at
// one pixel per thread the kernel is bound by its LDS reads (two ds_read_b128 per 8 fmas, 864 bytes read per 32 bytes written), with P
// pixels a weight fragment is read once for all of them.  A workgroup takes chunks of 256 P items (item = pixel * K/8 + channel group);
// thread t has items t + 256 j, so with K/8 a divisor of 256 the channel group is the same for every j (the host gives P = 1
// otherwise), the pixels of one j are consecutive across a wave (1 KB stores at K = 64) and P 2048 / K apart within a thread.  A tap
// outside the map contributes fma(0, w, acc): the sum of the taps inside, in the order the one-pixel form adds them.  Both stores of a
// pixel leave from the same fp32 a; a32 (debug, may be NULL) receives it.  What is left after that is VALU work, so the chain runs on
// packed fp32 fmas (two channels per instruction, the same two roundings), x is addressed by 32-bit byte offsets from the uniform base
// (one add per load; the host refuses an image of 4 GiB or more) and the roundings are v_cvt_pk_bf16_f32 (round to nearest even).
typedef float stem_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stem_load4(const float* p, stem_f2 (&f)[4]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = stem_f2{a.x, a.y}, f[1] = stem_f2{a.z, a.w}, f[2] = stem_f2{b.x, b.y}, f[3] = stem_f2{b.z, b.w};
}
template <int P>
__global__ void __launch_bounds__(256) irse_stem_fused_kernel(const float* __restrict__ x, const float* __restrict__ wf, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* __restrict__ slope,
                                                              const float* __restrict__ scale0, const float* __restrict__ shift0, uint4* __restrict__ y,
                                                              uint4* __restrict__ z, float* __restrict__ a32, int H, int W, int C, int K, int64_t total,
                                                              int64_t chunks) {
  extern __shared__ __attribute__((aligned(16))) float stem_lds[];  // [9][4][K] weights, then scale, shift, slope, scale0, shift0 [K] each
  float* wl = stem_lds;
  float* pl = stem_lds + 36 * K;
  for (int i = threadIdx.x; i < 36 * K; i += 256) {
    const int k = i % K, c = (i / K) & 3, t = i / (4 * K);
    wl[i] = c < C ? wf[((int64_t)t * C + c) * K + k] : 0.f;
  }
  for (int i = threadIdx.x; i < K; i += 256) {
    pl[i] = scale[i], pl[K + i] = shift[i], pl[2 * K + i] = slope[i], pl[3 * K + i] = scale0[i], pl[4 * K + i] = shift0[i];
  }
  __syncthreads();
  const int K8 = K / 8;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t i0 = ch * (256 * P) + threadIdx.x;  // this thread's items: i0 + 256 j
    const int c8 = (int)(i0 % K8);
    uint32_t xoff[P];  // byte offset of the pixel in x
    int xx[P], yy[P];
    bool live[P];
    stem_f2 acc[P][4];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int64_t i = i0 + 256 * j;
      live[j] = i < total;
      const int64_t pix = i / K8;
      xx[j] = (int)(pix % W), yy[j] = (int)((pix / W) % H);
      xoff[j] = (uint32_t)(pix * C) * 4u;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] = stem_f2{0.f, 0.f};
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3 - 1, dx = t % 3 - 1;
      const uint32_t toff = (uint32_t)((dy * W + dx) * C) * 4u;  // uniform; wraps for the taps before the pixel, as the sum below does
      // zero padding: a tap outside the map (and a dead item) reads x[0] and counts as 0 -- every load is unconditional, so the loads of
      // a tap leave together instead of one exec-masked block, with a wait of its own, per load
      bool ok[P];
      uint32_t off[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        ok[j] = live[j] & ((unsigned)(yy[j] + dy) < (unsigned)H) & ((unsigned)(xx[j] + dx) < (unsigned)W);
        off[j] = ok[j] ? xoff[j] + toff : 0u;
      }
      float xv[4][P];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (uint32_t)(off[j] + 4u * c));
          xv[c][j] = ok[j] ? v : 0.f;
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        stem_f2 w[4];
        stem_load4(wl + (t * 4 + c) * K + c8 * 8, w);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const stem_f2 x2 = stem_f2{xv[c][j], xv[c][j]};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = __builtin_elementwise_fma(x2, w[e], acc[j][e]);
        }
      }
    }
    stem_f2 sc[4], sh[4], sl[4], sc0[4], sh0[4];
    stem_load4(pl + c8 * 8, sc);
    stem_load4(pl + K + c8 * 8, sh);
    stem_load4(pl + 2 * K + c8 * 8, sl);
    stem_load4(pl + 3 * K + c8 * 8, sc0);
    stem_load4(pl + 4 * K + c8 * 8, sh0);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (!live[j]) continue;
      const int64_t i = i0 + 256 * j;
      float a[8], b[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const stem_f2 v = __builtin_elementwise_fma(acc[j][e], sc[e], sh[e]), n = sl[e] * v;
        a[2 * e] = v.x > 0.f ? v.x : n.x, a[2 * e + 1] = v.y > 0.f ? v.y : n.y;
        const stem_f2 zz = stem_f2{a[2 * e], a[2 * e + 1]} * sc0[e] + sh0[e];  // fmi_irse_stem_bf16's expression on the same fp32 a
        b[2 * e] = zz.x, b[2 * e + 1] = zz.y;
      }
      y[i] = bf_pack8_hw(a);
      if (a32) {
        float4* o = reinterpret_cast<float4*>(a32 + i * 8);
        o[0] = make_float4(a[0], a[1], a[2], a[3]);
        o[1] = make_float4(a[4], a[5], a[6], a[7]);
      }
      z[i] = bf_pack8_hw(b);
    }
  }
}
#define FMI_STEM_PIXELS 4 /* pixels a thread of the fused stem carries where K / 8 divides 256 (16 x 256^2 x 3 -> 64: 1, 2, 4, 8 measured) */
extern "C" int fmi_irse_stem_fwd_bf16(const fmi_conv_desc* d, const float* x, const float* wf, const float* scale, const float* shift,
                                      const float* slope, const float* scale0, const float* shift0, uint16_t* y, uint16_t* z, float* a32,
                                      void* stream) {
  int rc = enc_check_desc(d);
  if (rc) return rc;
  if (!x || !wf || !scale || !shift || !slope || !scale0 || !shift0 || !y || !z) return FMI_ERR_BAD_ARG;
  if (d->C > 4 || d->K % 8 != 0 || d->K > 256 || d->kh != 3 || d->pad != 1) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)d->N * d->H * d->W * d->C * 4 > 0xffffffffLL) return FMI_ERR_UNSUPPORTED;  // x is addressed by 32-bit byte offsets
  if ((((uintptr_t)x | (uintptr_t)wf | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)slope | (uintptr_t)scale0 | (uintptr_t)shift0) & 3) != 0 ||
      !fmi_al16(y) || !fmi_al16(z) || !fmi_al16(a32))
    return FMI_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)d->N * d->H * d->W * (d->K / 8);
  const int pp = 256 % (d->K / 8) == 0 ? FMI_STEM_PIXELS : 1;
  const int64_t chunks = ceil_div64(total, 256 * pp);
  const dim3 grid((unsigned)(chunks < 2048 ? chunks : 2048)), block(256);
  const size_t lds = (size_t)(41 * d->K) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define STEM_LAUNCH(PP) \
  hipLaunchKernelGGL(irse_stem_fused_kernel<PP>, grid, block, lds, st, x, wf, scale, shift, slope, scale0, shift0, (uint4*)y, (uint4*)z, a32, d->H, d->W, \
                     d->C, d->K, total, chunks)
  if (pp == FMI_STEM_PIXELS) STEM_LAUNCH(FMI_STEM_PIXELS);
  else STEM_LAUNCH(1);
#undef STEM_LAUNCH
  return fmi_launch_status();
}

// ---- the 32-channel layers: y = lrelu(conv(x) + b, slope), x bf16 [N,H,W,32], wnk bf16 [K][taps][32], y bf16 [N,H,W,K] -------------
// O^T[k][pixel] = sum_tap W_tap[k][c] X_tap^T[c][pixel] on v_mfma_f32_32x32x16_bf16: a wave owns tiles of 32 consecutive pixels (rows of
// the flattened N H W index, so any W), the A fragments of ALL taps and output channels stay in its registers for the launch
// (TAPS x 2 k-steps x KT tiles of 4 VGPRs: 144 for 3x3 into 64 channels), and the B fragment of a tap is two 16-byte loads per lane
// straight from the map -- lane (pixel p, half lh) reads channels 16 kk + 8 lh .. + 7 of pixel p + tap offset, or zeros outside the map.
// A pixel's 64 bytes are read by the nine taps of its neighbours out of the cache; memory sees x once and y once.  No LDS, no barrier.
// Register r of output tile kt is channel 32 kt + (r & 3) + 8 (r >> 2) + 4 lh of pixel l31: four consecutive channels per 8-byte store.
#define ENC_C32_TILES_PER_WAVE 2
#define ENC_C32_MAX_BLOCKS 512
template <int KT, int TAPS>
__global__ void __launch_bounds__(256) enc_c32_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wnk, const float* __restrict__ bias,
                                                      uint16_t* __restrict__ y, int H, int W, float slope, int64_t P, int64_t tiles) {
  constexpr int K = KT * 32, R = TAPS == 9 ? 1 : 0;  // R: the tap radius
  const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  bf16x8_t wa[KT][TAPS][2];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        wa[kt][t][kk] = __builtin_bit_cast(
            bf16x8_t, *reinterpret_cast<const u32x4_t*>(wnk + ((int64_t)(kt * 32 + l31) * TAPS + t) * 32 + 16 * kk + 8 * lh));
  float bv[KT][4][4];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[kt][g][e] = bias ? bias[kt * 32 + 8 * g + 4 * lh + e] : 0.f;

  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t tile = wave0; tile < tiles; tile += nwaves) {
    const int64_t p = tile * 32 + l31;
    const bool valid = p < P;
    const int xx = (int)(p % W), yy = (int)((p / W) % H);
    f32x16 acc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int dy = TAPS == 9 ? t / 3 - R : 0, dx = TAPS == 9 ? t % 3 - R : 0;
      const int iy = yy + dy, ix = xx + dx;
      const bool in = valid && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const uint16_t* xp = x + (p + (int64_t)dy * W + dx) * 32 + 8 * lh;
      u32x4_t b0 = {0u, 0u, 0u, 0u}, b1 = {0u, 0u, 0u, 0u};
      if (in) {
        b0 = *reinterpret_cast<const u32x4_t*>(xp);
        b1 = *reinterpret_cast<const u32x4_t*>(xp + 16);
      }
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[kt][t][0], __builtin_bit_cast(bf16x8_t, b0), acc[kt], 0, 0, 0);
        acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[kt][t][1], __builtin_bit_cast(bf16x8_t, b1), acc[kt], 0, 0, 0);
      }
    }
    if (valid) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float f[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = enc_lrelu(acc[kt][4 * g + e] + bv[kt][g][e], slope);
          *reinterpret_cast<uint2*>(y + p * K + kt * 32 + 8 * g + 4 * lh) = make_uint2(bf_pack2(f[0], f[1]), bf_pack2(f[2], f[3]));
        }
    }
  }
}
extern "C" int fmi_conv2d_c32_fwd_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* bias, float slope, uint16_t* y,
                                       void* stream) {
  int rc = enc_check_desc(d);
  if (rc) return rc;
  if (!x || !wnk || !y) return FMI_ERR_BAD_ARG;
  const bool k3 = d->kh == 3 && d->pad == 1, k1 = d->kh == 1 && d->pad == 0;
  if (d->C != 32 || (d->K != 32 && d->K != 64) || !(k3 || k1)) return FMI_ERR_UNSUPPORTED;
  if (!fmi_al16(x) || !fmi_al16(wnk) || !fmi_al16(y) || !fmi_al16(bias)) return FMI_ERR_UNSUPPORTED;
  const int64_t P = (int64_t)d->N * d->H * d->W, tiles = ceil_div64(P, 32);
  int64_t nb = ceil_div64(tiles, 4 * ENC_C32_TILES_PER_WAVE);
  if (nb > ENC_C32_MAX_BLOCKS) nb = ENC_C32_MAX_BLOCKS;
  const dim3 grid((unsigned)nb), block(256);
  hipStream_t st = (hipStream_t)stream;
#define ENC_C32_LAUNCH(KT, TAPS) hipLaunchKernelGGL((enc_c32_kernel<KT, TAPS>), grid, block, 0, st, x, wnk, bias, y, d->H, d->W, slope, P, tiles)
  if (d->K == 32) {
    if (k3) ENC_C32_LAUNCH(1, 9);
    else ENC_C32_LAUNCH(1, 1);
  } else {
    if (k3) ENC_C32_LAUNCH(2, 9);
    else ENC_C32_LAUNCH(2, 1);
  }
#undef ENC_C32_LAUNCH
  return fmi_launch_status();
}

// ---- block tail: v = main + shortcut [2x2 mean of the sum]; y_raw = bf16(v), y_act = bf16(lrelu(v)), y_f32 = v ----------------------
// The eight (two) addends are summed as a tree: every term passes at most three roundings.
__global__ void __launch_bounds__(256) enc_tail_kernel(const uint4* __restrict__ a, const uint4* __restrict__ s, uint4* __restrict__ y_raw,
                                                       uint4* __restrict__ y_act, float* __restrict__ y_f32, int OH, int OW, int C8, int pool,
                                                       float slope, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float v[8];
    if (!pool) {
      float f[8], g[8];
      bf_unpack8(a[i], f);
      bf_unpack8(s[i], g);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = f[e] + g[e];
    } else {
      const int c8 = (int)(i % C8);
      const int64_t pix = i / C8;
      const int ox = (int)(pix % OW);
      const int64_t row = pix / OW;  // n * OH + oy; the input has 2 OH rows of 2 OW pixels per sample
      const int64_t i00 = ((row * 2) * (2 * (int64_t)OW) + 2 * ox) * C8 + c8, i10 = i00 + 2 * (int64_t)OW * C8;
      float t[4][8];
      const int64_t idx[4] = {i00, i00 + C8, i10, i10 + C8};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float f[8], g[8];
        bf_unpack8(a[idx[q]], f);
        bf_unpack8(s[idx[q]], g);
#pragma unroll
        for (int e = 0; e < 8; ++e) t[q][e] = f[e] + g[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ((t[0][e] + t[1][e]) + (t[2][e] + t[3][e])) * 0.25f;
    }
    if (y_raw) y_raw[i] = bf_pack8(v);
    if (y_f32) {
      float4* o = reinterpret_cast<float4*>(y_f32 + i * 8);
      o[0] = make_float4(v[0], v[1], v[2], v[3]);
      o[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    if (y_act) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = enc_lrelu(v[e], slope);
      y_act[i] = bf_pack8(v);
    }
  }
}
extern "C" int fmi_resblock_tail_bf16(const uint16_t* main_, const uint16_t* shortcut, uint16_t* y_raw, uint16_t* y_act, float* y_f32, int N, int H,
                                      int W, int C, int pool, float slope, void* stream) {
  if (!main_ || !shortcut || (!y_raw && !y_act && !y_f32) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (pool != 0 && pool != 1)) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || (pool && (H % 2 != 0 || W % 2 != 0))) return FMI_ERR_UNSUPPORTED;
  if (!fmi_al16(main_) || !fmi_al16(shortcut) || !fmi_al16(y_raw) || !fmi_al16(y_act) || !fmi_al16(y_f32)) return FMI_ERR_UNSUPPORTED;
  const int OH = pool ? H / 2 : H, OW = pool ? W / 2 : W;
  const int64_t total = (int64_t)N * OH * OW * (C / 8);
  hipLaunchKernelGGL(enc_tail_kernel, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const uint4*)main_, (const uint4*)shortcut,
                     (uint4*)y_raw, (uint4*)y_act, y_f32, OH, OW, C / 8, pool, slope, total);
  return fmi_launch_status();
}

// ---- the stem's tail: v = pool2(h) + sum_c wb[c][k] pool2(img)[c] + bias[k]; h bf16 [N,H,W,K], img fp32 [N,H,W,C <= 4] ---------------
// Two fma chains, a = fma(w0, p0, pool(h)) [, w3] and b = fma(w2, p2, fma(w1, p1, bias)), v = a + b: no term passes more than five
// roundings (two of them in its 2x2 mean).
__global__ void __launch_bounds__(256) enc_stem_tail_kernel(const uint4* __restrict__ h, const float* __restrict__ img, const float* __restrict__ wb,
                                                            const float* __restrict__ bias, uint4* __restrict__ y_raw, uint4* __restrict__ y_act,
                                                            int OH, int OW, int C, int K8, float slope, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % K8);
    const int64_t pix = i / K8;
    const int ox = (int)(pix % OW);
    const int64_t row = pix / OW;
    const int64_t p00 = (row * 2) * (2 * (int64_t)OW) + 2 * ox, p10 = p00 + 2 * (int64_t)OW;
    const int64_t pidx[4] = {p00, p00 + 1, p10, p10 + 1};
    float t[4][8], pc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bf_unpack8(h[pidx[q] * K8 + c8], t[q]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      pc[c] = c < C ? ((img[pidx[0] * C + c] + img[pidx[1] * C + c]) + (img[pidx[2] * C + c] + img[pidx[3] * C + c])) * 0.25f : 0.f;
    float w[4][8], b[8], v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) bf_load8f(wb + (int64_t)c * K8 * 8 + c8 * 8, w[c]);
      else
#pragma unroll
        for (int e = 0; e < 8; ++e) w[c][e] = 0.f;
    }
    if (bias) bf_load8f(bias + c8 * 8, b);
    else
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float ph = ((t[0][e] + t[1][e]) + (t[2][e] + t[3][e])) * 0.25f;
      const float a = fmaf(w[3][e], pc[3], fmaf(w[0][e], pc[0], ph));
      const float bb = fmaf(w[2][e], pc[2], fmaf(w[1][e], pc[1], b[e]));
      v[e] = a + bb;
    }
    if (y_raw) y_raw[i] = bf_pack8(v);
    if (y_act) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = enc_lrelu(v[e], slope);
      y_act[i] = bf_pack8(v);
    }
  }
}
extern "C" int fmi_picnet_stem_tail_bf16(const uint16_t* h, const float* img, const float* wb, const float* bias, uint16_t* y_raw, uint16_t* y_act,
                                         int N, int H, int W, int C, int K, float slope, void* stream) {
  if (!h || !img || !wb || (!y_raw && !y_act) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0) return FMI_ERR_BAD_ARG;
  if (C > 4 || K % 8 != 0 || H % 2 != 0 || W % 2 != 0) return FMI_ERR_UNSUPPORTED;
  if (!fmi_al16(h) || !fmi_al16(wb) || !fmi_al16(bias) || !fmi_al16(y_raw) || !fmi_al16(y_act) || ((uintptr_t)img & 3) != 0) return FMI_ERR_UNSUPPORTED;
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)N * OH * OW * (K / 8);
  hipLaunchKernelGGL(enc_stem_tail_kernel, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const uint4*)h, img, wb, bias,
                     (uint4*)y_raw, (uint4*)y_act, OH, OW, C, K / 8, slope, total);
  return fmi_launch_status();
}
