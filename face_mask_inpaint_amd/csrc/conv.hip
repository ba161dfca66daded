// Implicit-GEMM convolution family: forward, adjoint (= ConvTranspose2d forward / conv input gradient)
// and weight gradient.  See include/fmi_hip.h for the contract and gemm_core.h for the machine mapping.
#include "gemm_core.h"
#include "conv3x3.h"
#include "conv_p3.h"
#include "convt3x3.h"

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the 16-byte epilogue: Nout % 4 == 0, 16-byte rows, every tensor it touches 16-byte aligned
static int ep_vec(const ConvEp& ep, int Nout) {
  return Nout % 4 == 0 && ep.cstride % 4 == 0 && aligned16(ep.y) && aligned16(ep.bias) && aligned16(ep.res) && aligned16(ep.mask);
}

static int check_desc(const fmi_conv_desc* d) {
  if (!d) return FMI_ERR_BAD_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 ||
      d->pad < 0 || d->x_cstride < d->C || d->y_cstride < d->K)
    return FMI_ERR_BAD_ARG;
  const int pe = d->pad, dl = d->dil > 1 ? d->dil : 1;
  if (d->dil < 0 || (dl > 1 && d->pad_mode)) return FMI_ERR_BAD_ARG;
  if (d->OH != (d->H + 2 * pe - dl * (d->kh - 1) - 1) / d->stride + 1 || d->OW != (d->W + 2 * pe - dl * (d->kw - 1) - 1) / d->stride + 1)
    return FMI_ERR_BAD_ARG;
  if (d->OH <= 0 || d->OW <= 0) return FMI_ERR_BAD_ARG;
  if (d->pad_mode == 1 && (d->pad >= d->H || d->pad >= d->W)) return FMI_ERR_UNSUPPORTED;
  if (d->pad_mode != 0 && d->pad_mode != 1) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)d->N * d->H * d->W > 0x7fffffffLL / 2 || (int64_t)d->kh * d->kw * d->C > 0x3fffffffLL) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}

// the fields the shared builders (gemm_core.h) leave to the family, as the fp32 gathers read them; img = the gathered tensor
static ConvGeom f32_geom(ConvGeom g, const fmi_conv_desc* d, const float* img) {
  const int dl = d->dil > 1 ? d->dil : 1;  // dilation = the tap step of the gather (modules/drn.py); adjoint: only with stride 1 (the caller checks)
  g.ystep *= dl; g.xstep *= dl;
  g.vec = (g.C % 4 == 0) && (g.cstride % 4 == 0) && aligned16(img);  // 1 = four channels are one float4 load
  g.dC = make_fastdiv(g.C);                                          // reduction index -> tap
  g.img_bs = (int64_t)g.IH * g.IW * g.cstride;                       // per-sample weight mode: one sample of the image
  return g;
}

#ifndef FMI_HOST_EMU
// y[pixel][k] = bias[k] + bias2[k] + residual[pixel][k] (each may be null): first pass of a split-reduction convolution; bias2 = the second
// convolution's bias of a pair (conv_pair.h)
__global__ void __launch_bounds__(256) conv_split_init_kernel(float* __restrict__ y, const float* __restrict__ bias, const float* __restrict__ bias2,
                                                             const float* __restrict__ res, int K, int cstride, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % K);
    const int64_t o = (i / K) * cstride + k;
    float v = bias ? bias[k] : 0.f;
    if (bias2) v += bias2[k];
    if (res) v += res[o];
    y[o] = v;
  }
}
#endif

// Small feature maps with deep reductions (the 128-channel residual stacks at 32x32 and below, and the discriminator) give
// the implicit GEMM only a handful of output tiles: split the (tap, channel) reduction over several workgroups per tile.
static int conv_ksplit(int64_t M, int N, int K) {
#ifdef FMI_HOST_EMU
  return 1;
#else
  // keep the 128-wide tiles (operand reuse) and fill the chip by splitting the reduction instead of shrinking the tile
  const int64_t tiles = ceil_div64(M, 128) * ceil_div64(N, N <= 32 ? 32 : (N <= 64 ? 64 : 128));
  if (K < 512 || fmi_det()) return 1;  // reproducible mode: no split reduction (partial sums would meet through atomics)
  if (tiles >= 320) {
    // between one and two "waves" of workgroups (3 per CU x 256 CUs) the CUs that got 3 tiles set the time while the others idle
    // (VGG 28^2: 588 tiles = 2.3 per CU): splitting the work unit lets the dispatcher even it out.  Measured (TFLOP/s, split 1 / 2 / 3):
    // 588 tiles K 4608: 102 / 111 / 118;  588 tiles K 2304: 101 / 107 / 109;  512 tiles K 2304: 111 / 116 / 111;
    // 1024 tiles K 2304: 125 / 118 / 114;  1176 tiles K 2304: 101 / 97 / 100  ->  no split from ~800 tiles up
    if (tiles >= 800 || K < 2304) return 1;
    return tiles <= 520 ? 2 : 3;
  }
  // 192 .. 319 tiles: unsplit wins up to K = 2304 (256 tiles: 8 x 64^2 128 -> 128 92 vs 81 TFLOP/s split in two; the IR-SE50 stage
  // 16 x 32^2 256 -> 256 94.5 vs 89)
  if (tiles >= 192 && K < 4608) return 1;
  int64_t ks = ceil_div64(384, tiles);
  // at least 16 k-tiles per split; a handful of output tiles (M <= 128 rows: the pSp style heads at 4^2 .. 1^2) only stream the
  // weights, so more, shorter splits put more loads in flight: 4 k-tiles there
  const int64_t kmin = (M <= 128 && tiles <= 16) ? 64 : 256;
  if (ks > K / kmin) ks = K / kmin;
  return ks < 2 ? 1 : (int)(ks > (kmin == 64 ? 64 : 16) ? (kmin == 64 ? 64 : 16) : ks);
#endif
}

// One output phase: the forward convolution, or one sub-pixel phase of the adjoint (flip = 1: the 3x3 tap-reuse kernels take the
// flipped taps of the adjoint's weight pack).  g gathers x (g.C channels at pitch g.cstride; x3 = its bf16 piece image or null); w / w3 =
// the weights packed for this direction and their piece image (null where it cannot be used); ep writes Nout channels.  may_split: the
// reduction may be split over workgroups, whose partial sums meet through atomics in an output initialised first; shared_init: the caller
// has initialised the output once for all phases (the adjoint's strided split) and this phase only adds to it.
static int conv_phase(const fmi_conv_desc* d, const ConvGeom& g, const float* x, const void* x3, const float* w, const void* w3p,
                      int64_t w_bstride, int Nout, int flip, ConvEp ep, int batch_w, bool may_split, bool shared_init, hipStream_t st) {
  ConvK la{x, g};
  ConvWX lb{w, g, w_bstride, Nout, (Nout % 4 == 0) && aligned16(w) && (w_bstride % 4 == 0)};
  const int ks = may_split ? conv_ksplit(g.Mdim(), Nout, g.Kdim()) : 1;
#ifndef FMI_HOST_EMU
  if (shared_init || ks > 1) {
    if (!shared_init) {
      const int64_t total = (int64_t)g.N * ep.OHt * ep.OWt * Nout;
      hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, ep.y, ep.bias, (const float*)nullptr, ep.res, Nout, ep.cstride,
                         total);
    }
    ep.bias = nullptr;
    ep.res = nullptr;
    ep.act = 3;
    ep.vec = 0;
  }
  const uint16_t* w3 = (const uint16_t*)w3p;
  const int64_t w3_stride = (int64_t)d->kh * d->kw * d->C * d->K;
  const int64_t pixels = (int64_t)g.N * g.IH * g.IW;
  const bool tap3 = d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->dil <= 1 && g.pad_mode == 0;
  // both operands as bf16 piece images (conv_p3.h): the activation pieces of x came from x's producer
  const bool p3 = batch_w == 1 && g.cstride == g.C && g.Kdim() > 0 && p3_generic_ok(g, x3, w3, Nout);
  if (p3 && tap3 && conv3x3_p3_eligible(x3, w3, g.C, Nout, pixels)) {
    const C3P3Args ca{(const uint16_t*)x3, w3, g.N, g.IH, g.IW, g.C, Nout, flip, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW)};
    return launch_conv3x3_p3(ca, ep, g.Mdim(), ks, st);
  }
  if (p3)
    return launch_gemm_p3(ConvK3{(const uint16_t*)x3, g, make_fastdiv(g.ntaps())}, ConvWX3{w3, g, w3_stride, Nout}, ep, g.Mdim(), Nout,
                          g.Kdim(), ks, st);
  if (batch_w == 1 && tap3 && conv3x3_eligible(x, w, g.C, g.cstride, Nout, pixels)) {
    const C3Args ca{x, w, g.N, g.IH, g.IW, g.C, g.cstride, Nout, flip, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW), w3};
    return launch_conv3x3(ca, ep, g.Mdim(), ks, st);
  }
  if (w3 && la.dma_ok()) return launch_gemm(la, ConvWX3{w3, g, w3_stride, Nout}, ep, g.Mdim(), Nout, g.Kdim(), 1, ks, st);
#endif
  return launch_gemm(la, lb, ep, g.Mdim(), Nout, g.Kdim(), batch_w, ks, st);
}

// d->w3, the bf16 piece image of the weights, where the kernels can read it: shared weights, 16-channel groups of the reduction
static const void* weight_pieces(const fmi_conv_desc* d, int batch_w, int red_c) {
#ifndef FMI_HOST_EMU
  if (batch_w == 1 && red_c % 16 == 0 && aligned16(d->w3)) return d->w3;
#endif
  return nullptr;
}

static int check_y3(const fmi_conv_desc* d, int out_c, int out_cs) {
  if (!d->y3) return FMI_OK;
  return (out_c % 16 == 0 && out_cs == out_c && aligned16(d->y3)) ? FMI_OK : FMI_ERR_BAD_ARG;
}

extern "C" int fmi_conv2d_fwd_f32(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias,
                                  const float* residual, float* y, int act, int batch_w, int64_t w_bstride,
                                  void* stream) {
  if (!d) return FMI_ERR_BAD_ARG;
  int rc = check_y3(d, d->K, d->y_cstride);
  if (rc) return rc;
  rc = check_desc(d);
  if (rc) return rc;
  if (!x || !wf || !y || batch_w < 1 || act < 0 || act > 2) return FMI_ERR_BAD_ARG;
  if (batch_w > 1 && batch_w != d->N) return FMI_ERR_BAD_ARG;
  auto finish = [&](int rc) {  // the piece image of y, if one is requested
#ifndef FMI_HOST_EMU
    if (rc == FMI_OK && d->y3) rc = fmi_split3_f32(y, d->y3, nullptr, (int64_t)d->N * d->OH * d->OW, d->K, 0, 0.f, stream);
#endif
    return rc;
  };
#ifndef FMI_HOST_EMU
  if (batch_w == 1 && fmi_conv2d_thin_supported(d) && aligned16(x))
    return finish(fmi_conv2d_thin_fwd_f32(d, x, wf, bias, residual, y, act, stream));
  // thin INPUT (C <= 4: the image-facing first layers), 3x3 on a large map: streaming FMA kernel (thinin.hip).  The 1x1 form is a 9 - 13 us
  // launch either way and did not clear the keep-only-if-faster rule (profiles/thin_in.txt): it stays on the generic path
  if (batch_w == 1 && d->kh == 3 && fmi_conv2d_thin_in_routed(d) && aligned16(y) && aligned16(residual))
    return finish(fmi_conv2d_thin_in_fwd_f32(d, x, wf, bias, residual, y, act, stream));
#endif
  const ConvGeom g = f32_geom(fwd_geom(d, batch_w > 1 ? 1 : d->N), d, x);
  // bf16 piece images of the weights (fmi_weight_prepare_f32 writes them): [3][taps][C / 8][K][8]
  const void* w3 = weight_pieces(d, batch_w, d->C);
  ConvEp ep{y, bias, residual, d->OH, d->OW, 1, 0, 0, d->OH, d->OW, d->y_cstride, act, g.dGW, g.dG, (int64_t)d->OH * d->OW * d->y_cstride};
  ep.vec = ep_vec(ep, d->K);
  return finish(conv_phase(d, g, x, d->x3, wf, w3, w_bstride, d->K, 0, ep, batch_w, act == 0 && batch_w == 1, false, (hipStream_t)stream));
}

static int dgrad_impl(const fmi_conv_desc* d, const float* dy, const float* wt, const float* bias, const float* residual,
                      const float* mask, float mslope, float* dx, int batch_w, int64_t w_bstride, void* stream) {
  if (!d) return FMI_ERR_BAD_ARG;
  int rc = check_y3(d, d->C, d->x_cstride);
  if (rc) return rc;
  rc = check_desc(d);
  if (rc) return rc;
  if (!dy || !wt || !dx || batch_w < 1) return FMI_ERR_BAD_ARG;
  if (d->pad_mode != 0) return FMI_ERR_UNSUPPORTED;  // reflect: run on the padded extent, then fmi_reflect_pad_fold_f32
  if (batch_w > 1 && batch_w != d->N) return FMI_ERR_BAD_ARG;
  if (mask && bias) return FMI_ERR_UNSUPPORTED;  // the mask applies to the bare adjoint; a residual is added AFTER it (ConvEp: v * mask + res)
  auto finish = [&](int rc) {  // the piece image of dx, if one is requested
#ifndef FMI_HOST_EMU
    if (rc == FMI_OK && d->y3) rc = fmi_split3_f32(dx, d->y3, nullptr, (int64_t)d->N * d->H * d->W, d->C, 0, 0.f, stream);
#endif
    return rc;
  };
#ifndef FMI_HOST_EMU
  if (batch_w == 1 && !bias && !residual && !mask && fmi_conv2d_thin_supported(d) && aligned16(dx))
    return finish(fmi_conv2d_thin_dgrad_f32(d, dy, wt, dx, stream));
  // thin INPUT: VGG16's first layer (the entry's 1x1 form is not routed here: see the forward)
  if (batch_w == 1 && !bias && !residual && !mask && d->C <= 4 && d->x_cstride == d->C && d->kh == 3) {
    const int rc_thin = fmi_conv2d_thin_input_dgrad_f32(d, dy, wt, dx, stream);
    if (rc_thin != FMI_ERR_UNSUPPORTED) return finish(rc_thin);
  }
#endif
  const int n_eff = batch_w > 1 ? 1 : d->N;
  const int s = d->stride;
  // bf16 piece images of the adjoint's weights: [3][taps][K / 8][C][8]
  const void* w3 = weight_pieces(d, batch_w, d->K);
  if (d->dil > 1 && s != 1) return FMI_ERR_UNSUPPORTED;  // adjoint of a dilated AND strided convolution: not needed by modules/drn.py
  bool strided_split = false;
#ifndef FMI_HOST_EMU
  // Strided adjoints of small feature maps (the stride-2 style heads of the pSp encoder: 512 -> 512 at 16^2 .. 2^2) are a few
  // output tiles per sub-pixel phase with up to 128 reduction tiles each -- 0.25 ms of pure load latency per call.  If any phase
  // wants a split reduction, dx is initialised once and EVERY phase adds its (partial) sums atomically.
  if (s > 1 && batch_w == 1) {
    for (int py = 0; py < s && !strided_split; ++py)
      for (int px = 0; px < s && !strided_split; ++px) {
        const ConvGeom g = adj_geom(d, n_eff, py, px);
        if (g.GH > 0 && g.GW > 0 && conv_ksplit(g.Mdim(), d->C, g.Kdim()) > 1) strided_split = true;
      }
    if (strided_split) {
      const int64_t total = (int64_t)d->N * d->H * d->W * d->C;
      hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, dx, bias, (const float*)nullptr, residual, d->C,
                         d->x_cstride, total);
    }
  }
  // thin ConvTranspose2d(3, stride 2) on a large map: all four sub-pixel phases in one tap-reuse launch (convt3x3.h)
  if (batch_w == 1 && !strided_split && !d->x3 && convt3x3_eligible(d, dy, (const uint16_t*)w3)) {
    CT3Args ca{};
    ca.x = dy; ca.w3 = (const uint16_t*)w3; ca.N = d->N; ca.H = d->OH; ca.W = d->OW; ca.Cred = d->K; ca.cs = d->y_cstride; ca.Nout = d->C;
    ca.dW = make_fastdiv(d->OW); ca.dHW = make_fastdiv(d->OH * d->OW);
    ConvEp ep{dx, bias, residual, d->OH, d->OW, 2, 0, 0, d->H, d->W, d->x_cstride, 0, ca.dW, ca.dHW, (int64_t)d->H * d->W * d->x_cstride};
    ep.mask = mask;
    ep.mslope = mslope;
    ep.vec = ep_vec(ep, d->C);
    ca.ep = ep;
    return finish(launch_convt3x3(ca, d->N * d->OH * d->OW, (hipStream_t)stream));
  }
#endif
  for (int py = 0; py < s; ++py) {
    for (int px = 0; px < s; ++px) {
      const ConvGeom g = f32_geom(adj_geom(d, n_eff, py, px), d, dy);
      if (g.GH <= 0 || g.GW <= 0) continue;
      ConvEp ep{dx, bias, residual, g.GH, g.GW, s, py, px, d->H, d->W, d->x_cstride, 0, g.dGW, g.dG,
                (int64_t)d->H * d->W * d->x_cstride};
      ep.mask = mask;
      ep.mslope = mslope;
      ep.vec = ep_vec(ep, d->C);
      rc = conv_phase(d, g, dy, d->x3, wt, w3, w_bstride, d->C, 1, ep, batch_w, batch_w == 1 && (s == 1 || strided_split), strided_split,
                      (hipStream_t)stream);
      if (rc) return rc;
    }
  }
  return finish(FMI_OK);
}
extern "C" int fmi_conv2d_dgrad_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* bias,
                                    const float* residual, float* dx, int batch_w, int64_t w_bstride, void* stream) {
  return dgrad_impl(d, dy, wt, bias, residual, nullptr, 0.f, dx, batch_w, w_bstride, stream);
}
// y = ConvTranspose2d(x1, W1) + ConvTranspose2d(x2, W2) + bias for two 3x3 stride-2 transposed convolutions of the same geometry (the main
// path and the bypass of ResBlockDecoder, base_function.py:297-305) in ONE launch of convt3x3.h: the reduction runs over x1's channels,
// then over x2's.  d describes the first one as for fmi_conv2d_dgrad_f32 (d->K = channels of x1, d->C = output channels, d->H x d->W the
// output, d->w3 = the piece image of its adjoint pack); K2 = channels of the dense tensor x2, w3b its piece image.
extern "C" int fmi_conv_transpose2d_pair_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int K2, const void* w3b,
                                             const float* bias, float* y, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!x1 || !x2 || !w3b || !d->w3 || !y || K2 <= 0) return FMI_ERR_BAD_ARG;
#ifndef FMI_HOST_EMU
  const uint16_t* w3 = (d->K % 16 == 0 && aligned16(d->w3)) ? (const uint16_t*)d->w3 : nullptr;
  if (!convt3x3_eligible(d, x1, w3) || (K2 & 15) || !aligned16(x2) || !aligned16(w3b) || d->pad_mode != 0 || d->x3) return FMI_ERR_UNSUPPORTED;
  CT3Args ca{};
  ca.x = x1; ca.w3 = w3; ca.x2 = x2; ca.w3b = (const uint16_t*)w3b; ca.Cred2 = K2; ca.cs2 = K2;
  ca.N = d->N; ca.H = d->OH; ca.W = d->OW; ca.Cred = d->K; ca.cs = d->y_cstride; ca.Nout = d->C;
  ca.dW = make_fastdiv(d->OW); ca.dHW = make_fastdiv(d->OH * d->OW);
  ConvEp ep{y, bias, nullptr, d->OH, d->OW, 2, 0, 0, d->H, d->W, d->x_cstride, 0, ca.dW, ca.dHW, (int64_t)d->H * d->W * d->x_cstride};
  ep.vec = ep_vec(ep, d->C);
  ca.ep = ep;
  return launch_convt3x3(ca, d->N * d->OH * d->OW, (hipStream_t)stream);
#else
  return FMI_ERR_UNSUPPORTED;
#endif
}
extern "C" int fmi_conv2d_dgrad_masked_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* mask, float mask_slope,
                                           float* dx, void* stream) {
  if (!mask) return FMI_ERR_BAD_ARG;
  return dgrad_impl(d, dy, wt, nullptr, nullptr, mask, mask_slope, dx, 1, 0, stream);
}

extern "C" int fmi_conv2d_dgrad_masked_add_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* mask, float mask_slope,
                                               const float* gadd, float* dx, void* stream) {
  if (!mask || !gadd) return FMI_ERR_BAD_ARG;
  return dgrad_impl(d, dy, wt, nullptr, gadd, mask, mask_slope, dx, 1, 0, stream);
}

extern "C" int fmi_conv2d_wgrad_f32(const fmi_conv_desc* d, const float* x, const float* dy, float* dwf, float* dbias,
                                    int batch_w, int64_t w_bstride, void* stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!x || !dy || !dwf || batch_w < 1) return FMI_ERR_BAD_ARG;
  if (batch_w > 1 && batch_w != d->N) return FMI_ERR_BAD_ARG;
#ifndef FMI_HOST_EMU
  if (batch_w == 1 && fmi_conv2d_thin_supported(d) && aligned16(x)) return fmi_conv2d_thin_wgrad_f32(d, x, dy, dwf, dbias, stream);
#endif
#ifndef FMI_HOST_EMU
  // both operands as bf16 piece images (d->x3 = pieces of x, d->y3 = pieces of dy, INPUTS here): no split arithmetic, transposed LDS reads.
  // The bias gradient does not ride along on this path (the caller runs fmi_bias_grad_f32).
  if (batch_w == 1 && !dbias && wgrad_p3_ok(d, d->x3, d->y3))
    return launch_wgrad_p3(d, (const uint16_t*)d->x3, (const uint16_t*)d->y3, dwf, (hipStream_t)stream);
#endif
  const int n_eff = batch_w > 1 ? 1 : d->N;
  ConvGeom g = f32_geom(fwd_geom(d, n_eff), d, x);
  // the bias gradient rides along as one extra output row (needs a float4-aligned row index and shared weights)
  const bool fuse_bias = dbias && batch_w == 1 && (g.Kdim() % 4 == 0);
  if (dbias && !fuse_bias) return FMI_ERR_UNSUPPORTED;
  const int ones_row = fuse_bias ? g.Kdim() : -1;
  const int Mg = g.Kdim() + (fuse_bias ? 1 : 0), Ng = d->K, Kg = g.Mdim();
  WgradAX la{x, g, ones_row};
  DenseX lb{dy, (int64_t)d->y_cstride, (int64_t)d->OH * d->OW * d->y_cstride, Ng, Kg,
            (d->K % 4 == 0) && (d->y_cstride % 4 == 0) && aligned16(dy)};
  WgradEp ep{dwf, g, d->K, w_bstride, dbias, ones_row};
  // split the (long) pixel reduction over workgroups; partial sums meet through fp32 atomics
  const int64_t tiles = ceil_div64(Mg, 128) * ceil_div64(Ng, Ng <= 32 ? 32 : (Ng <= 64 ? 64 : 128));
  int64_t ksplit = 2048 / (tiles * batch_w);
  const int64_t kmax = Kg / 512;
  if (ksplit > kmax) ksplit = kmax;
  if (ksplit < 1) ksplit = 1;
  if (fmi_det()) ksplit = 1;  // reproducible mode: one workgroup per tile walks the whole pixel reduction
  if (ksplit * batch_w > 65535) ksplit = 65535 / batch_w;
  return launch_gemm(la, lb, ep, Mg, Ng, Kg, batch_w, (int)ksplit, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// The stride-1 ResBlock pair (conv_pair.h): y = act(conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2) as one reduction over 9 * C + C2 elements,
// and dW1, dW2 and the gradient of both biases from one walk over dy.  d describes the 3x3 convolution (d->w3 = the piece image of its
// forward pack or null); x2 is dense [N][H][W][C2].
// ---------------------------------------------------------------------------------------------
static int pair_check(const fmi_conv_desc* d, int C2) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (C2 <= 0) return FMI_ERR_BAD_ARG;
  if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1 || d->pad_mode != 0 || d->dil > 1) return FMI_ERR_UNSUPPORTED;
  if ((d->C & 15) || (C2 & 15) || (d->K & 3) || d->x_cstride != d->C || d->y_cstride != d->K) return FMI_ERR_UNSUPPORTED;
  if (9ll * d->C + C2 > 0x3fffffffLL || (int64_t)d->N * d->H * d->W >= (1ll << 30)) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
// reduction splits of the pair's forward, as the launch takes them (1: unsplit)
static int pair_ksplit(const fmi_conv_desc* d, int C2, int act, bool tap_reuse) {
  const int M = d->N * d->H * d->W, Kd = 9 * d->C + C2;
  int ks = act == 0 ? conv_ksplit(M, d->K, Kd) : 1;
  if (tap_reuse) {  // launch_conv3x3: whole (ky, 16 channels) steps per split
    const int nit = 3 * (d->C >> 4) + (C2 >> 4);
    if (ks > nit) ks = nit;
    const int it_chunk = (nit + ks - 1) / ks;
    return (nit + it_chunk - 1) / it_chunk;
  }
  const int kchunk = (int)ceil_div64(ceil_div64(Kd, ks), 16) * 16;  // launch_gemm: 16-deep tiles per split
  return (int)ceil_div64(Kd, kchunk);
}
static bool pair_tap_reuse(const fmi_conv_desc* d) {
#ifndef FMI_HOST_EMU
  return (d->C >= 64 || d->K <= 32);  // conv3x3_eligible's channel rule; alignment is checked at the call
#else
  return false;
#endif
}
extern "C" int fmi_conv2d_pair_supported(const fmi_conv_desc* d, int C2) { return d && pair_check(d, C2) == FMI_OK; }
extern "C" int fmi_conv2d_pair_ksplit(const fmi_conv_desc* d, int C2, int act) {
  if (!d || pair_check(d, C2) != FMI_OK) return 0;
  return pair_ksplit(d, C2, act, pair_tap_reuse(d));
}
// Which passes of a supported shape the ResBlock routes here: bit 0 the forward, bit 1 the weight gradient.  A pass is routed only where the
// fused launch was faster than conv2 + bypass in EVERY alternated round of tools/bench_tools/resblock_pair_time.py
// (profiles/resblock_pair.txt): the weight gradient at every measured shape (8 x 8^2 .. 8 x 128^2); the forward at all of them but
// 8 x 32^2 128 -> 128, a tie (39.6 against 39.5 us, lower in 2 rounds of 5).  Where conv2 runs from piece images of x1 today
// (functional.p3_wanted: >= 16384 pixels, C >= 64, K >= 128) only the measured shape, 8 x 64^2 64 -> 128, is routed.  Below 32 channels
// (nothing measured: the step has no such block) the two launches stay.
extern "C" int fmi_conv2d_pair_routed(const fmi_conv_desc* d, int C2) {
  if (!fmi_conv2d_pair_supported(d, C2) || d->C < 32) return 0;
  const int64_t px = (int64_t)d->N * d->H * d->W;
  if (px >= 16384 && d->C >= 64 && d->K >= 128) return (d->C == 64 && d->K == 128 && px <= 32768) ? 3 : 0;
  const bool fwd_tie = d->C == 128 && d->K == 128 && px > 2048 && px < 16384;
  return fwd_tie ? 2 : 3;
}

extern "C" int fmi_conv2d_pair_fwd_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int C2, const float* wf1, const float* wf2,
                                       const void* w3b, const float* b1, const float* b2, float* y, int act, void* stream) {
  if (!d) return FMI_ERR_BAD_ARG;
  int rc = pair_check(d, C2);
  if (rc) return rc;
  if (!x1 || !x2 || !wf1 || !wf2 || !y || act < 0 || act > 2) return FMI_ERR_BAD_ARG;
  if (!aligned16(x1) || !aligned16(x2) || !aligned16(wf1) || !aligned16(wf2) || !aligned16(y) || !aligned16(b1) || !aligned16(b2)) return FMI_ERR_BAD_ARG;
  if (!b1) { b1 = b2; b2 = nullptr; }
  const ConvGeom g = f32_geom(fwd_geom(d, d->N), d, x1);
  const int K1 = g.Kdim(), Kd = K1 + C2, M = g.Mdim();
  ConvEp2 ep;
  static_cast<ConvEp&>(ep) = ConvEp{y, b1, nullptr, d->OH, d->OW, 1, 0, 0, d->OH, d->OW, d->y_cstride, act, g.dGW, g.dG, (int64_t)d->OH * d->OW * d->y_cstride};
  ep.bias2 = b2;
  ep.vec = ep_vec(ep, d->K);
  const bool tap_reuse = pair_tap_reuse(d);
  const int ks = pair_ksplit(d, C2, act, tap_reuse);
#ifndef FMI_HOST_EMU
  hipStream_t st = (hipStream_t)stream;
  if (ks > 1) {  // y = b1 + b2 first; the partial sums meet in it through atomics
    const int64_t total = (int64_t)M * d->K;
    hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, y, b1, b2, (const float*)nullptr, d->K, d->y_cstride, total);
    ep.bias = nullptr;
    ep.bias2 = nullptr;
    ep.act = 3;
    ep.vec = 0;
  }
  const uint16_t* w3 = (const uint16_t*)weight_pieces(d, 1, d->C);
  const uint16_t* w32 = aligned16(w3b) ? (const uint16_t*)w3b : nullptr;
  if (!w3 || !w32) w3 = w32 = nullptr;  // the piece images of BOTH packs, or the fp32 packs
  if (tap_reuse) {
    C3Args2 ca;
    static_cast<C3Args&>(ca) = C3Args{x1, wf1, g.N, g.IH, g.IW, g.C, g.cstride, d->K, 0, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW), w3};
    ca.x2 = x2; ca.w2 = wf2; ca.w3b = w32; ca.C2 = C2; ca.cs2 = C2;
    return launch_conv3x3(ca, ep, M, ks, st);
  }
  const ConvK2 la{ConvK{x1, g}, x2, C2, C2, K1};
  if (w3) {
    const int64_t w3_stride = 9ll * d->C * d->K;
    return launch_gemm(la, ConvWX32{ConvWX3{w3, g, w3_stride, d->K}, w32, C2, K1}, ep, M, d->K, Kd, 1, ks, st);
  }
  return launch_gemm(la, ConvWX2{ConvWX{wf1, g, 0, d->K, 1}, wf2, C2, K1}, ep, M, d->K, Kd, 1, ks, st);
#else
  (void)w3b;
  return launch_gemm(ConvK2{ConvK{x1, g}, x2, C2, C2, K1}, ConvWX2{ConvWX{wf1, g, 0, d->K, 1}, wf2, C2, K1}, ep, M, d->K, Kd, 1, ks, (hipStream_t)stream);
#endif
}

// dw1 [9][C][K], dw2 [C2][K] and dbias [K] (may be null) are ACCUMULATED into: the caller zeroes them, as for fmi_conv2d_wgrad_f32
extern "C" int fmi_conv2d_pair_wgrad_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int C2, const float* dy, float* dw1, float* dw2,
                                         float* dbias, void* stream) {
  if (!d) return FMI_ERR_BAD_ARG;
  int rc = pair_check(d, C2);
  if (rc) return rc;
  if (!x1 || !x2 || !dy || !dw1 || !dw2) return FMI_ERR_BAD_ARG;
  if (!aligned16(x1) || !aligned16(x2) || !aligned16(dy)) return FMI_ERR_BAD_ARG;
  const ConvGeom g = f32_geom(fwd_geom(d, d->N), d, x1);
  const int R1 = g.Kdim(), ones_row = dbias ? R1 + C2 : -1;
  const int Mg = R1 + C2 + (dbias ? 1 : 0), Ng = d->K, Kg = g.Mdim();
  const WgradAX2 la{WgradAX{x1, g, -1}, x2, C2, C2, R1, ones_row};
  const DenseX lb{dy, (int64_t)d->y_cstride, (int64_t)d->OH * d->OW * d->y_cstride, Ng, Kg, 1};
  const WgradEp2 ep{WgradEp{dw1, g, d->K, 0, dbias, ones_row}, dw2, R1};
  // the pixel split of fmi_conv2d_wgrad_f32, over the taller row range
  const int64_t tiles = ceil_div64(Mg, 128) * ceil_div64(Ng, Ng <= 32 ? 32 : (Ng <= 64 ? 64 : 128));
  int64_t ksplit = 2048 / tiles;
  const int64_t kmax = Kg / 512;
  if (ksplit > kmax) ksplit = kmax;
  if (ksplit < 1) ksplit = 1;
  if (fmi_det()) ksplit = 1;
  if (ksplit > 65535) ksplit = 65535;
  return launch_gemm(la, lb, ep, Mg, Ng, Kg, 1, (int)ksplit, (hipStream_t)stream);
}

#ifndef FMI_HOST_EMU
// ---------------------------------------------------------------------------------------------
// dbias[k] += sum_rows g[row*cstride + k]
// vector form (K % 4 == 0, K/4 divides 256): the tensor is streamed as float4, 256 threads cover 256/(K/4) rows per
// pass with fully coalesced 16-byte loads; threads owning the same 4 channels are combined through LDS.
// ---------------------------------------------------------------------------------------------
// reproducible mode runs ONE workgroup over all rows: its threads then add tens of thousands of terms each, so they carry fp64 sums (the
// default mode's many short fp32 chains are more accurate than one long one: measured on the whole-pSp fixture)
__global__ void __launch_bounds__(256) bias_grad_vec_f64_kernel(const float* __restrict__ g, int64_t rows, int K4, float* __restrict__ dbias) {
  __shared__ double part[256][4];
  const int cg = threadIdx.x % K4, rl = threadIdx.x / K4, RL = 256 / K4;
  double s[4] = {0, 0, 0, 0};
  for (int64_t r = rl; r < rows; r += RL) {
    const float4 v = reinterpret_cast<const float4*>(g)[r * K4 + cg];
    s[0] += v.x, s[1] += v.y, s[2] += v.z, s[3] += v.w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[threadIdx.x][e] = s[e];
  __syncthreads();
  if (threadIdx.x < K4) {
    double t[4] = {0, 0, 0, 0};
    for (int l = 0; l < RL; ++l)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += part[l * K4 + threadIdx.x][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(dbias + 4 * threadIdx.x + e, (float)t[e]);
  }
}
__global__ void __launch_bounds__(256) bias_grad_vec_kernel(const float* __restrict__ g, int64_t rows, int K4,
                                                            float* __restrict__ dbias, int64_t rows_per_block) {
  __shared__ float4 part[256];
  const int cg = threadIdx.x % K4, rl = threadIdx.x / K4, RL = 256 / K4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t r = r0 + rl;
  for (; r + 3 * RL < r1; r += 4 * RL) {  // four independent 16-byte loads in flight per thread
    const float4 v0 = reinterpret_cast<const float4*>(g)[r * K4 + cg];
    const float4 v1 = reinterpret_cast<const float4*>(g)[(r + RL) * K4 + cg];
    const float4 v2 = reinterpret_cast<const float4*>(g)[(r + 2 * RL) * K4 + cg];
    const float4 v3 = reinterpret_cast<const float4*>(g)[(r + 3 * RL) * K4 + cg];
    s.x += (v0.x + v1.x) + (v2.x + v3.x);
    s.y += (v0.y + v1.y) + (v2.y + v3.y);
    s.z += (v0.z + v1.z) + (v2.z + v3.z);
    s.w += (v0.w + v1.w) + (v2.w + v3.w);
  }
  for (; r < r1; r += RL) {
    const float4 v = reinterpret_cast<const float4*>(g)[r * K4 + cg];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < K4) {
    float4 t = part[threadIdx.x];
    for (int l = 1; l < RL; ++l) {
      const float4 v = part[l * K4 + threadIdx.x];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    atomicAdd(dbias + 4 * threadIdx.x + 0, t.x);
    atomicAdd(dbias + 4 * threadIdx.x + 1, t.y);
    atomicAdd(dbias + 4 * threadIdx.x + 2, t.z);
    atomicAdd(dbias + 4 * threadIdx.x + 3, t.w);
  }
}
__global__ void __launch_bounds__(256) bias_grad_kernel(const float* __restrict__ g, int64_t rows, int K, int cstride,
                                                        float* __restrict__ dbias, int64_t rows_per_block) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int cg = 0; cg < K; cg += 64) {
    const int c = cg + tx;
    float s = 0.f;
    if (c < K)
      for (int64_t r = r0 + ty; r < r1; r += 4) s += g[r * cstride + c];
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < K) atomicAdd(dbias + c, part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx]);
    __syncthreads();
  }
}

extern "C" int fmi_bias_grad_f32(const float* g, int64_t rows, int K, int cstride, float* dbias, void* stream) {
  if (!g || !dbias || rows <= 0 || K <= 0 || cstride < K) return FMI_ERR_BAD_ARG;
  int64_t blocks = ceil_div64(rows, 256);
  // every workgroup ends with K atomics onto the same K addresses and those serialise: per training step (13 calls, up to 1 GB each)
  // 2048 workgroups took 1.31 ms, 512: 0.73, 256: 0.58 (the 1 GB tensor streams at 5.5 TB/s either way)
  if (blocks > 256) blocks = 256;
  if (fmi_det()) blocks = 1;  // reproducible mode: one workgroup, one contribution per channel
  const int64_t rpb = ceil_div64(rows, blocks);
  blocks = ceil_div64(rows, rpb);
  const int K4 = K / 4;
  if (fmi_det() && K % 4 == 0 && cstride == K && K4 <= 256 && (K4 & (K4 - 1)) == 0 && (((uintptr_t)g) & 15) == 0)
    hipLaunchKernelGGL(bias_grad_vec_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, g, rows, K4, dbias);
  else if (K % 4 == 0 && cstride == K && K4 <= 256 && (K4 & (K4 - 1)) == 0 && (((uintptr_t)g) & 15) == 0)
    hipLaunchKernelGGL(bias_grad_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, rows, K4, dbias, rpb);
  else
    hipLaunchKernelGGL(bias_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, rows, K, cstride, dbias, rpb);
  return fmi_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Gradient of nn.ReflectionPad2d(pad): gx[y][x] = sum of gpad over every padded position mirroring (y, x)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) reflect_fold_kernel(const float* __restrict__ gp, float* __restrict__ gx, int N,
                                                           int H, int W, int C, int pad, int64_t total) {
  const int HP = H + 2 * pad, WP = W + 2 * pad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int x = (int)(r % W);
    r /= W;
    const int y = (int)(r % H);
    const int n = (int)(r / H);
    // padded rows that map onto y: y+pad, and the mirrors pad-y (y in 1..pad), 2H-2-y+pad (y in H-1-pad..H-2)
    int ys[3], xs[3], ny = 0, nx = 0;
    ys[ny++] = y + pad;
    if (y >= 1 && y <= pad) ys[ny++] = pad - y;
    if (y <= H - 2 && y >= H - 1 - pad) ys[ny++] = 2 * H - 2 - y + pad;
    xs[nx++] = x + pad;
    if (x >= 1 && x <= pad) xs[nx++] = pad - x;
    if (x <= W - 2 && x >= W - 1 - pad) xs[nx++] = 2 * W - 2 - x + pad;
    float s = 0.f;
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) s += gp[(((int64_t)n * HP + ys[a]) * WP + xs[b]) * C + c];
    gx[i] = s;
  }
}

extern "C" int fmi_reflect_pad_fold_f32(const float* gpad, float* gx, int N, int H, int W, int C, int pad, void* stream) {
  if (!gpad || !gx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || pad < 0 || pad >= H || pad >= W) return FMI_ERR_BAD_ARG;
  const int64_t total = (int64_t)N * H * W * C;
  hipLaunchKernelGGL(reflect_fold_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, gpad, gx, N,
                     H, W, C, pad, total);
  return fmi_launch_status();
}
#endif  // FMI_HOST_EMU
