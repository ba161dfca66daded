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
static ConvGeom f32_geom_al(ConvGeom g, const fmi_conv_desc* d, bool img_al16) {
  const int dl = d->dil > 1 ? d->dil : 1;  // dilation = the tap step of the gather (modules/drn.py); adjoint: only with stride 1 (the caller checks)
  g.ystep *= dl; g.xstep *= dl;
  g.vec = (g.C % 4 == 0) && (g.cstride % 4 == 0) && img_al16;  // 1 = four channels are one float4 load
  g.dC = make_fastdiv(g.C);                                          // reduction index -> tap
  g.img_bs = (int64_t)g.IH * g.IW * g.cstride;                       // per-sample weight mode: one sample of the image
  return g;
}
static ConvGeom f32_geom(ConvGeom g, const fmi_conv_desc* d, const float* img) { return f32_geom_al(g, d, aligned16(img)); }

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

// Every routing decision below is conv_f32_plan.h's: this file gathers the facts a plan reads (ConvCallF, ConvPhaseInF), launches what
// comes back, and answers fmi_conv2d_f32_plan from the same functions.
extern "C" int fmi_debug_f32_last_plan(void) { return __atomic_load_n(&fmi_f32_last_plan_code, __ATOMIC_RELAXED); }

// what an entry learns from its pointers and the process.  x: the gathered tensor; w: the second operand (weights; the weight gradient's dy)
static ConvCallF call_facts(const fmi_conv_desc* d, const void* x, const void* w, const void* out, const void* bias, const void* res,
                            const void* mask, int act, int batch_w) {
  ConvCallF c{};
  c.x_al16 = aligned16(x); c.w_al16 = aligned16(w); c.out_al16 = aligned16(out); c.res_al16 = aligned16(res);
  c.x3 = d->x3 != nullptr; c.x3_al16 = aligned16(d->x3); c.w3 = d->w3 != nullptr; c.w3_al16 = aligned16(d->w3);
  c.y3 = d->y3 != nullptr; c.y3_al16 = aligned16(d->y3);
  c.bias = bias != nullptr; c.res = res != nullptr; c.mask = mask != nullptr;
  c.act = act; c.batch_w = batch_w;
  c.det = fmi_det();
#ifndef FMI_HOST_EMU
  c.dma_off = fmi_dma_off_env();
  if (batch_w == 1) {  // every thin exit needs shared weights: the predicates are not asked otherwise
    c.thin_out = fmi_conv2d_thin_supported(d) != 0;
    c.thin_in = d->kh == 3 && fmi_conv2d_thin_in_routed(d) != 0;  // only the forward's 3x3 exit reads it (fwd_early_f)
  }
#else  // the emulation has no thin kernels and reads no piece images
  c.x3 = c.w3 = c.y3 = false;
#endif
  return c;
}

// the plan's inputs of one output phase: the forward convolution, or one sub-pixel phase of the adjoint.  g gathers the image (g.C channels
// at pitch g.cstride); w3: the weights' piece image can be used (weight_pieces_f); w_vec: ConvWX's float4 loads are legal
static ConvPhaseInF phase_in(const fmi_conv_desc* d, const ConvGeom& g, int Nout, const ConvCallF& c, bool w3, bool w_vec, bool may_split,
                             bool shared_init) {
  ConvPhaseInF in{};
  in.M = g.Mdim(); in.Nout = Nout; in.Kdim = g.Kdim(); in.C = g.C; in.cstride = g.cstride;
  in.pixels = (int64_t)g.N * g.IH * g.IW;
  in.pad_mode = g.pad_mode;
  in.tap3 = d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->dil <= 1 && g.pad_mode == 0;
  in.batch_w = c.batch_w;
  in.x3 = c.x3 && c.x3_al16; in.w3 = w3;
  in.x_al16 = c.x_al16; in.w_al16 = c.w_al16;
  in.la_dma = ConvK{nullptr, g}.dma_ok();
  in.lb_dma = ConvWX{nullptr, g, 0, Nout, w_vec}.dma_ok();
  in.may_split = may_split; in.shared_init = shared_init;
  in.det = c.det; in.dma_off = c.dma_off;
  return in;
}
static bool w_vec_of(const ConvCallF& c, int Nout, int64_t w_bstride) { return (Nout % 4 == 0) && c.w_al16 && (w_bstride % 4 == 0); }
// bf16 piece images of the weights (fmi_weight_prepare_f32 writes them): forward [3][taps][C / 8][K][8], adjoint [3][taps][K / 8][C][8]
static ConvPhaseInF fwd_phase_in(const fmi_conv_desc* d, const ConvGeom& g, const ConvCallF& c, bool w_vec) {
  return phase_in(d, g, d->K, c, weight_pieces_f(c.w3 && c.w3_al16, c.batch_w, d->C), w_vec, c.act == 0 && c.batch_w == 1, false);
}
static ConvPhaseInF adj_phase_in(const fmi_conv_desc* d, const ConvGeom& g, const ConvCallF& c, bool w_vec, bool strided_split) {
  return phase_in(d, g, d->C, c, weight_pieces_f(c.w3 && c.w3_al16, c.batch_w, d->K), w_vec, dgrad_may_split_f(d, c, strided_split), strided_split);
}
// does any sub-pixel phase of a strided adjoint want a split reduction (dgrad_phase_wants_split_f)?
static bool adj_strided_split(const fmi_conv_desc* d, const ConvCallF& c, int n_eff) {
  if (d->stride == 1 || c.batch_w != 1) return false;  // dgrad_phase_wants_split_f's first two terms: no geometry is built for them
  for (int py = 0; py < d->stride; ++py)
    for (int px = 0; px < d->stride; ++px) {
      const ConvGeom g = adj_geom(d, n_eff, py, px);
      if (dgrad_phase_wants_split_f(d, c, g.GH, g.GW, g.Mdim(), g.Kdim())) return true;
    }
  return false;
}

// One output phase (flip = 1: the 3x3 tap-reuse kernels take the flipped taps of the adjoint's weight pack).  x3 = the piece image of the
// gathered tensor; w / w3 = the weights packed for this direction and their piece image; ep writes in.Nout channels.
static int conv_phase(const fmi_conv_desc* d, const ConvGeom& g, const ConvPhaseInF& in, const float* x, const void* x3, const float* w,
                      const void* w3p, int64_t w_bstride, bool w_vec, int flip, ConvEp ep, hipStream_t st) {
  const int Nout = in.Nout;
  ConvK la{x, g};
  ConvWX lb{w, g, w_bstride, Nout, w_vec};
#ifdef FMI_HOST_EMU  // every convolution through the emulated launch_gemm, unsplit
  (void)d; (void)x3; (void)w3p; (void)flip;
  return launch_gemm(la, lb, ep, in.M, Nout, in.Kdim, in.batch_w, 1, st);
#else
  const LaunchPlanF pl = conv_phase_plan_f(in);
  if (pl.init) {
    const int64_t total = (int64_t)g.N * ep.OHt * ep.OWt * Nout;
    hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, ep.y, ep.bias, (const float*)nullptr, ep.res, Nout, ep.cstride,
                       total);
  }
  if (phase_adds_f(in, pl)) {
    ep.bias = nullptr;
    ep.res = nullptr;
    ep.act = 3;
    ep.vec = 0;
  }
  const uint16_t* w3 = in.w3 ? (const uint16_t*)w3p : nullptr;
  const int64_t w3_stride = (int64_t)d->kh * d->kw * d->C * d->K;
  switch (pl.route) {
    case ROUTE_C3_P3_F:
      return launch_conv3x3_p3(C3P3Args{(const uint16_t*)x3, w3, g.N, g.IH, g.IW, g.C, Nout, flip, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW)}, ep, in.M, pl, st);
    case ROUTE_GEMM_P3_F:
      return launch_gemm_p3(ConvK3{(const uint16_t*)x3, g, make_fastdiv(g.ntaps())}, ConvWX3{w3, g, w3_stride, Nout}, ep, in.M, Nout, in.Kdim, pl, st);
    case ROUTE_C3_F:
    case ROUTE_C3_W3_F:
      return launch_conv3x3(C3Args{x, w, g.N, g.IH, g.IW, g.C, g.cstride, Nout, flip, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW), w3}, ep, in.M, pl, st);
    case ROUTE_GEMM_W3_F: return launch_gemm_plan(la, ConvWX3{w3, g, w3_stride, Nout}, ep, in.M, Nout, in.Kdim, 1, pl, st);
    case ROUTE_GEMM_F: return launch_gemm_plan(la, lb, ep, in.M, Nout, in.Kdim, in.batch_w, pl, st);
  }
  return pl.status ? pl.status : FMI_ERR_BAD_ARG;
#endif
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
  const ConvCallF c = call_facts(d, x, wf, y, bias, residual, nullptr, act, batch_w);
#ifndef FMI_HOST_EMU
  switch (fwd_early_f(d, c)) {
    case ROUTE_THIN_OUT_F: return finish(fmi_conv2d_thin_fwd_f32(d, x, wf, bias, residual, y, act, stream));
    case ROUTE_THIN_IN_F: return finish(fmi_conv2d_thin_in_fwd_f32(d, x, wf, bias, residual, y, act, stream));
  }
#endif
  const ConvGeom g = f32_geom(fwd_geom(d, batch_w > 1 ? 1 : d->N), d, x);
  const bool w_vec = w_vec_of(c, d->K, w_bstride);
  ConvEp ep{y, bias, residual, d->OH, d->OW, 1, 0, 0, d->OH, d->OW, d->y_cstride, act, g.dGW, g.dG, (int64_t)d->OH * d->OW * d->y_cstride};
  ep.vec = ep_vec(ep, d->K);
  return finish(conv_phase(d, g, fwd_phase_in(d, g, c, w_vec), x, d->x3, wf, d->w3, w_bstride, w_vec, 0, ep, (hipStream_t)stream));
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
  const ConvCallF c = call_facts(d, dy, wt, dx, bias, residual, mask, 0, batch_w);
#ifndef FMI_HOST_EMU
  if (dgrad_thin_out_f(c)) return finish(fmi_conv2d_thin_dgrad_f32(d, dy, wt, dx, stream));
  if (dgrad_thin_in_tried_f(d, c)) {
    const int rc_thin = fmi_conv2d_thin_input_dgrad_f32(d, dy, wt, dx, stream);
    if (rc_thin != FMI_ERR_UNSUPPORTED) return finish(rc_thin);
  }
#endif
  const int n_eff = batch_w > 1 ? 1 : d->N;
  const int s = d->stride;
  if (d->dil > 1 && s != 1) return FMI_ERR_UNSUPPORTED;  // adjoint of a dilated AND strided convolution: not needed by modules/drn.py
  bool strided_split = false;
#ifndef FMI_HOST_EMU
  strided_split = adj_strided_split(d, c, n_eff);
  if (strided_split) {  // dx is initialised once and EVERY phase adds its (partial) sums atomically
    const int64_t total = (int64_t)d->N * d->H * d->W * d->C;
    hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, dx, bias, (const float*)nullptr, residual, d->C,
                       d->x_cstride, total);
  }
  if (dgrad_convt3x3_f(d, c, strided_split)) {
    CT3Args ca{};
    ca.x = dy; ca.w3 = (const uint16_t*)d->w3; ca.N = d->N; ca.H = d->OH; ca.W = d->OW; ca.Cred = d->K; ca.cs = d->y_cstride; ca.Nout = d->C;
    ca.dW = make_fastdiv(d->OW); ca.dHW = make_fastdiv(d->OH * d->OW);
    ConvEp ep{dx, bias, residual, d->OH, d->OW, 2, 0, 0, d->H, d->W, d->x_cstride, 0, ca.dW, ca.dHW, (int64_t)d->H * d->W * d->x_cstride};
    ep.mask = mask;
    ep.mslope = mslope;
    ep.vec = ep_vec(ep, d->C);
    ca.ep = ep;
    return finish(launch_convt3x3(ca, d->N * d->OH * d->OW, convt3x3_plan_f(d->N * d->OH * d->OW, d->C), (hipStream_t)stream));
  }
#endif
  const bool w_vec = w_vec_of(c, d->C, w_bstride);
  for (int py = 0; py < s; ++py) {
    for (int px = 0; px < s; ++px) {
      const ConvGeom g = f32_geom(adj_geom(d, n_eff, py, px), d, dy);
      if (g.GH <= 0 || g.GW <= 0) continue;
      ConvEp ep{dx, bias, residual, g.GH, g.GW, s, py, px, d->H, d->W, d->x_cstride, 0, g.dGW, g.dG,
                (int64_t)d->H * d->W * d->x_cstride};
      ep.mask = mask;
      ep.mslope = mslope;
      ep.vec = ep_vec(ep, d->C);
      rc = conv_phase(d, g, adj_phase_in(d, g, c, w_vec, strided_split), dy, d->x3, wt, d->w3, w_bstride, w_vec, 1, ep, (hipStream_t)stream);
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
  const uint16_t* w3 = (const uint16_t*)d->w3;
  if (!convt3x3_eligible_f(d, aligned16(x1), weight_pieces_f(aligned16(d->w3), 1, d->K)) || (K2 & 15) || !aligned16(x2) || !aligned16(w3b) || d->pad_mode != 0 || d->x3) return FMI_ERR_UNSUPPORTED;
  CT3Args ca{};
  ca.x = x1; ca.w3 = w3; ca.x2 = x2; ca.w3b = (const uint16_t*)w3b; ca.Cred2 = K2; ca.cs2 = K2;
  ca.N = d->N; ca.H = d->OH; ca.W = d->OW; ca.Cred = d->K; ca.cs = d->y_cstride; ca.Nout = d->C;
  ca.dW = make_fastdiv(d->OW); ca.dHW = make_fastdiv(d->OH * d->OW);
  ConvEp ep{y, bias, nullptr, d->OH, d->OW, 2, 0, 0, d->H, d->W, d->x_cstride, 0, ca.dW, ca.dHW, (int64_t)d->H * d->W * d->x_cstride};
  ep.vec = ep_vec(ep, d->C);
  ca.ep = ep;
  return launch_convt3x3(ca, d->N * d->OH * d->OW, convt3x3_plan_f(d->N * d->OH * d->OW, d->C), (hipStream_t)stream);
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
  const ConvCallF c = call_facts(d, x, dy, dwf, dbias, nullptr, nullptr, 0, batch_w);
#ifndef FMI_HOST_EMU
  if (wgrad_thin_out_f(c)) return fmi_conv2d_thin_wgrad_f32(d, x, dy, dwf, dbias, stream);
#endif
  const int n_eff = batch_w > 1 ? 1 : d->N;
  ConvGeom g = f32_geom(fwd_geom(d, n_eff), d, x);
  const bool dy_vec = (d->K % 4 == 0) && (d->y_cstride % 4 == 0) && c.w_al16;
  const WgradPlanF w = wgrad_plan_f(d, c, g.Kdim(), g.Mdim(), g.vec != 0, dy_vec);
  if (w.pl.status) return w.pl.status;
#ifndef FMI_HOST_EMU
  if (w.pl.route != ROUTE_WGRAD_GEMM_F) return launch_wgrad_p3(d, (const uint16_t*)d->x3, (const uint16_t*)d->y3, dwf, w.pl, (hipStream_t)stream);
#endif
  const int ones_row = w.fuse_bias ? g.Kdim() : -1;
  const int Mg = g.Kdim() + (w.fuse_bias ? 1 : 0), Ng = d->K, Kg = g.Mdim();
  WgradAX la{x, g, ones_row};
  DenseX lb{dy, (int64_t)d->y_cstride, (int64_t)d->OH * d->OW * d->y_cstride, Ng, Kg, dy_vec};
  WgradEp ep{dwf, g, d->K, w_bstride, dbias, ones_row};
#ifndef FMI_HOST_EMU
  return launch_gemm_plan(la, lb, ep, Mg, Ng, Kg, batch_w, w.pl, (hipStream_t)stream);
#else
  return launch_gemm(la, lb, ep, Mg, Ng, Kg, batch_w, 1, (hipStream_t)stream);
#endif
}

// ---------------------------------------------------------------------------------------------
// The stride-1 ResBlock pair (conv_pair.h): y = act(conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2) as one reduction over 9 * C + C2 elements,
// and dW1, dW2 and the gradient of both biases from one walk over dy.  d describes the 3x3 convolution (d->w3 = the piece image of its
// forward pack or null); x2 is dense [N][H][W][C2].
// ---------------------------------------------------------------------------------------------
static int pair_check(const fmi_conv_desc* d, int C2) {
  const int rc = check_desc(d);
  return rc ? rc : pair_shape_check_f(d, C2);
}
#ifdef FMI_HOST_EMU  // the emulation runs the pair on the plain GEMM loop, unsplit
static bool pair_tap_reuse(const fmi_conv_desc*) { return false; }
static int pair_ksplit(const fmi_conv_desc*, int, int, bool) { return 1; }
#else
static bool pair_tap_reuse(const fmi_conv_desc* d) { return pair_tap_reuse_f(d); }
static int pair_ksplit(const fmi_conv_desc* d, int C2, int act, bool tap_reuse) { return pair_ksplit_f(d, C2, act, tap_reuse, fmi_det()); }
#endif
extern "C" int fmi_conv2d_pair_supported(const fmi_conv_desc* d, int C2) { return d && pair_check(d, C2) == FMI_OK; }
extern "C" int fmi_conv2d_pair_ksplit(const fmi_conv_desc* d, int C2, int act) {
  if (!d || pair_check(d, C2) != FMI_OK) return 0;
  return pair_ksplit(d, C2, act, pair_tap_reuse(d));
}
// The pair's two launches as plans, shared by the entries and by fmi_conv2d_f32_plan.  dma_ok: both loaders stage through LDS-DMA -- true
// for every call the entries accept (they refuse a misaligned operand, and pair_check leaves C, C2 % 16 == 0 and K % 4 == 0).  The pair's
// loaders are not ConvK / WgradAX, so FMI_DMA_OFF reads them under its dense bit (gemm_family_f).
static LaunchPlanF pair_fwd_plan(const fmi_conv_desc* d, int C2, int act, bool w3_both, bool dma_ok, bool det, int dma_off) {
  const int M = d->N * d->H * d->W, Kd = 9 * d->C + C2;
  const bool tap_reuse = pair_tap_reuse_f(d);
  const int ks = pair_ksplit_f(d, C2, act, tap_reuse, det);
  LaunchPlanF pl = tap_reuse ? c3_plan_f(M, d->K, 3 * (d->C >> 4) + (C2 >> 4), ks, w3_both, det)
                             : gemm_plan_f(w3_both ? ROUTE_GEMM_W3_F : ROUTE_GEMM_F, M, d->K, Kd, 1, ks, dma_ok, DMA_FAMILY_DENSE_F, dma_off, det);
  pl.init = ks > 1;  // y = b1 + b2 first; the partial sums meet in it through atomics
  return pl;
}
static LaunchPlanF pair_wgrad_plan(const fmi_conv_desc* d, int C2, bool bias, bool dma_ok, bool det, int dma_off) {
  const int Mg = 9 * d->C + C2 + (bias ? 1 : 0), P = d->N * d->H * d->W;
  return gemm_plan_f(ROUTE_WGRAD_GEMM_F, Mg, d->K, P, 1, (int)pair_wgrad_split_f(Mg, d->K, P, det), dma_ok, DMA_FAMILY_DENSE_F, dma_off, det);
}
// which passes of a supported shape the ResBlock routes here (pair_routed_f): bit 0 the forward, bit 1 the weight gradient
extern "C" int fmi_conv2d_pair_routed(const fmi_conv_desc* d, int C2) { return fmi_conv2d_pair_supported(d, C2) ? pair_routed_f(d) : 0; }

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
#ifndef FMI_HOST_EMU
  hipStream_t st = (hipStream_t)stream;
  const uint16_t* w3 = weight_pieces_f(aligned16(d->w3), 1, d->C) ? (const uint16_t*)d->w3 : nullptr;
  const uint16_t* w32 = aligned16(w3b) ? (const uint16_t*)w3b : nullptr;
  if (!w3 || !w32) w3 = w32 = nullptr;  // the piece images of BOTH packs, or the fp32 packs
  const ConvK2 la{ConvK{x1, g}, x2, C2, C2, K1};
  const ConvWX32 lb3{ConvWX3{w3, g, 9ll * d->C * d->K, d->K}, w32, C2, K1};
  const ConvWX2 lb{ConvWX{wf1, g, 0, d->K, 1}, wf2, C2, K1};
  const LaunchPlanF pl = pair_fwd_plan(d, C2, act, w3 != nullptr, la.dma_ok() && (w3 ? lb3.dma_ok() : lb.dma_ok()), fmi_det(), fmi_dma_off_env());
  if (pl.init) {
    const int64_t total = (int64_t)M * d->K;
    hipLaunchKernelGGL(conv_split_init_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, st, y, b1, b2, (const float*)nullptr, d->K, d->y_cstride, total);
    ep.bias = nullptr;
    ep.bias2 = nullptr;
    ep.act = 3;
    ep.vec = 0;
  }
  if (pl.route == ROUTE_C3_F || pl.route == ROUTE_C3_W3_F) {
    C3Args2 ca;
    static_cast<C3Args&>(ca) = C3Args{x1, wf1, g.N, g.IH, g.IW, g.C, g.cstride, d->K, 0, make_fastdiv(g.IW), make_fastdiv(g.IH * g.IW), w3};
    ca.x2 = x2; ca.w2 = wf2; ca.w3b = w32; ca.C2 = C2; ca.cs2 = C2;
    return launch_conv3x3(ca, ep, M, pl, st);
  }
  if (w3) return launch_gemm_plan(la, lb3, ep, M, d->K, Kd, 1, pl, st);
  return launch_gemm_plan(la, lb, ep, M, d->K, Kd, 1, pl, st);
#else
  (void)w3b;
  return launch_gemm(ConvK2{ConvK{x1, g}, x2, C2, C2, K1}, ConvWX2{ConvWX{wf1, g, 0, d->K, 1}, wf2, C2, K1}, ep, M, d->K, Kd, 1, 1, (hipStream_t)stream);
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
#ifndef FMI_HOST_EMU
  return launch_gemm_plan(la, lb, ep, Mg, Ng, Kg, 1, pair_wgrad_plan(d, C2, dbias != nullptr, la.dma_ok() && lb.dma_ok(), fmi_det(), fmi_dma_off_env()), (hipStream_t)stream);
#else
  return launch_gemm(la, lb, ep, Mg, Ng, Kg, 1, 1, (hipStream_t)stream);
#endif
}

// ---------------------------------------------------------------------------------------------
// fmi_conv2d_f32_plan: what the entries above would launch, from the functions they decide with, without a launch (include/fmi_hip.h)
// ---------------------------------------------------------------------------------------------
static ConvCallF call_facts_of_flags(const fmi_conv_desc* d, int flags) {
  ConvCallF c{};
  c.x_al16 = flags & FMI_F32_PLAN_X_AL16; c.w_al16 = flags & FMI_F32_PLAN_W_AL16; c.out_al16 = flags & FMI_F32_PLAN_OUT_AL16;
  c.res = flags & FMI_F32_PLAN_RES; c.res_al16 = !c.res || (flags & FMI_F32_PLAN_RES_AL16);
  c.x3 = flags & FMI_F32_PLAN_X3; c.x3_al16 = !c.x3 || (flags & FMI_F32_PLAN_X3_AL16);
  c.w3 = flags & FMI_F32_PLAN_W3; c.w3_al16 = !c.w3 || (flags & FMI_F32_PLAN_W3_AL16);
  c.y3 = flags & FMI_F32_PLAN_Y3; c.y3_al16 = !c.y3 || (flags & FMI_F32_PLAN_Y3_AL16);
  c.bias = flags & FMI_F32_PLAN_BIAS; c.mask = flags & FMI_F32_PLAN_MASK;
  c.act = flags & FMI_F32_PLAN_ACT ? 1 : 0;
  c.batch_w = flags & FMI_F32_PLAN_BATCH_W ? d->N : 1;
  const bool modes = flags & FMI_F32_PLAN_MODES;
  c.det = modes ? (flags & FMI_F32_PLAN_DET) != 0 : fmi_det();
  c.thin_out = flags & FMI_F32_PLAN_THIN_OUT; c.thin_in = flags & FMI_F32_PLAN_THIN_IN;
#ifndef FMI_HOST_EMU  // this build has the predicates of thinconv.hip / thinin.hip: their answers, not the caller's
  c.dma_off = modes ? (flags >> FMI_F32_PLAN_DMA_OFF_SHIFT) & 7 : fmi_dma_off_env();
  c.thin_out = fmi_conv2d_thin_supported(d) != 0;
  c.thin_in = fmi_conv2d_thin_in_routed(d) != 0;
#else
  c.dma_off = modes ? (flags >> FMI_F32_PLAN_DMA_OFF_SHIFT) & 7 : 0;
#endif
  return c;
}
static int plan_out(int* out, int& n, const LaunchPlanF& pl) {
  if (n < 4) {
    int* o = out + 4 + 10 * n;
    o[0] = pl.route; o[1] = pl.tile; o[2] = pl.dma; o[3] = pl.fl; o[4] = pl.init; o[5] = pl.ksplit; o[6] = pl.chunk;
    o[7] = (int)pl.grid[0]; o[8] = (int)pl.grid[1]; o[9] = pl.code();
  }
  ++n;
  return pl.status;
}
extern "C" int fmi_conv2d_f32_plan(const fmi_conv_desc* d, int pass, int flags, int* out) {
  if (!d || !out) return FMI_ERR_BAD_ARG;
  for (int i = 0; i < FMI_CONV_F32_PLAN_INTS; ++i) out[i] = 0;
  const int C2 = pass >> 8;
  pass &= 255;
  auto done = [&](int rc) {  // the rest is zero when refused
    if (rc) for (int i = 1; i < FMI_CONV_F32_PLAN_INTS; ++i) out[i] = 0;
    return out[0] = rc;
  };
  if (pass < 0 || pass > 3) return done(FMI_ERR_BAD_ARG);
  int rc = pass == 3 ? pair_check(d, C2) : check_desc(d);
  if (rc) return done(rc);
  ConvCallF c = call_facts_of_flags(d, flags);
  const int n_eff = c.batch_w > 1 ? 1 : d->N;
  int n = 0;
  if (pass == 0) {
    if (c.y3 && !(d->K % 16 == 0 && d->y_cstride == d->K && c.y3_al16)) return done(FMI_ERR_BAD_ARG);
    if ((out[2] = fwd_early_f(d, c))) return done(FMI_OK);
    const ConvGeom g = f32_geom_al(fwd_geom(d, n_eff), d, c.x_al16);
    rc = plan_out(out, n, conv_phase_plan_f(fwd_phase_in(d, g, c, w_vec_of(c, d->K, 0))));
  } else if (pass == 1) {
    if (c.y3 && !(d->C % 16 == 0 && d->x_cstride == d->C && c.y3_al16)) return done(FMI_ERR_BAD_ARG);
    if (d->pad_mode != 0 || (c.mask && c.bias)) return done(FMI_ERR_UNSUPPORTED);
    // the thin-input adjoint has no predicate: whether fmi_conv2d_thin_input_dgrad_f32 takes what is tried on it is the caller's THIN_IN bit
    if (dgrad_thin_out_f(c)) out[2] = ROUTE_THIN_OUT_F;
    else if (dgrad_thin_in_tried_f(d, c) && (flags & FMI_F32_PLAN_THIN_IN)) out[2] = ROUTE_THIN_IN_F;
    if (out[2]) return done(FMI_OK);
    if (d->dil > 1 && d->stride != 1) return done(FMI_ERR_UNSUPPORTED);
    const bool strided_split = adj_strided_split(d, c, n_eff);
    out[3] = strided_split ? 1 : 0;
    if (dgrad_convt3x3_f(d, c, strided_split)) {
      rc = plan_out(out, n, convt3x3_plan_f(d->N * d->OH * d->OW, d->C));
    } else {
      for (int py = 0; py < d->stride; ++py)
        for (int px = 0; px < d->stride; ++px) {
          const ConvGeom g = f32_geom_al(adj_geom(d, n_eff, py, px), d, c.x_al16);
          if (g.GH <= 0 || g.GW <= 0) continue;
          if (!rc) rc = plan_out(out, n, conv_phase_plan_f(adj_phase_in(d, g, c, w_vec_of(c, d->C, 0), strided_split)));
        }
    }
  } else if (pass == 2) {
    if ((out[2] = wgrad_thin_out_f(c) ? ROUTE_THIN_OUT_F : 0)) return done(FMI_OK);
    const ConvGeom g = f32_geom_al(fwd_geom(d, n_eff), d, c.x_al16);
    const WgradPlanF w = wgrad_plan_f(d, c, g.Kdim(), g.Mdim(), g.vec != 0, (d->K % 4 == 0) && (d->y_cstride % 4 == 0) && c.w_al16);
    out[3] = (w.fuse_bias ? 2 : 0) | (w.pl.xcd_splits ? 4 : 0);
    rc = plan_out(out, n, w.pl);
  } else {  // the ResBlock pair (C2 = pass >> 8): which passes are routed to it, its forward, its weight gradient (BIAS: with a bias gradient)
    out[3] = pair_routed_f(d) << 4;
    // the entries refuse a misaligned operand: x1 / x2 (X_AL16), the packs or dy (W_AL16), y (OUT_AL16, the forward only)
    if (!c.x_al16 || !c.w_al16) return done(FMI_ERR_BAD_ARG);
    rc = c.out_al16 ? plan_out(out, n, pair_fwd_plan(d, C2, c.act, c.w3 && c.w3_al16, true, c.det, c.dma_off)) : FMI_ERR_BAD_ARG;
    if (!rc) rc = plan_out(out, n, pair_wgrad_plan(d, C2, c.bias, true, c.det, c.dma_off));
  }
  out[1] = n;
  return done(rc);
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
