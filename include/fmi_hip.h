/*
 * fmi_hip.h -- C ABI of libfmi_hip.so: MI355X (gfx950) kernels for the
 * reference-guided inpainting training hot path of syncdoth/face_mask_inpaint.
 *
 * Conventions
 *  - every entry point is extern "C", takes raw DEVICE pointers + sizes, an
 *    explicit hipStream_t (passed as void*), launches asynchronously and
 *    returns an fmi_status (0 = ok).  Nothing is allocated or retained.
 *  - activations are NHWC fp32 (channels contiguous) unless stated; "cstride"
 *    arguments are the distance in floats between consecutive pixels so that
 *    channel slices of a wider tensor can be read / written in place.
 *  - unsupported arguments fail loudly (FMI_ERR_*); the reference's CUDA
 *    upfirdn2d silently returns uninitialised memory for them
 *    (modules/psp/stylegan2/op/upfirdn2d_kernel.cu:172-268).
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *  - fmi_upfirdn2d_f32      <- upfirdn2d_op.upfirdn2d, op/upfirdn2d.cpp:12-23,
 *                              kernel op/upfirdn2d_kernel.cu:52-272
 *  - fmi_fused_bias_act_f32 <- fused.fused_bias_act, op/fused_bias_act.cpp:11-20,
 *                              kernel op/fused_bias_act_kernel.cu:18-99
 *  - everything else replaces stock ATen calls made by the nn.Modules on the
 *    path (F.conv2d / conv_transpose2d / bmm / softmax / instance_norm /
 *    interpolate / avg_pool / Adam ...); each prototype cites its call site.
 */
#ifndef FMI_HIP_H
#define FMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  FMI_OK = 0,
  FMI_ERR_BAD_ARG = 1,      /* null pointer, non-positive size, misaligned view */
  FMI_ERR_UNSUPPORTED = 2,  /* shape / mode outside what the kernels implement */
  FMI_ERR_LAUNCH = 3        /* hipGetLastError() != hipSuccess after the launch */
} fmi_status;

const char* fmi_status_string(int status);
int fmi_version(void);
/* Reproducible mode (also FMI_DETERMINISTIC=1 in the environment at load time).  Default off: split reductions meet through fp32 atomics,
 * whose arrival order changes the rounding from run to run.  On: every entry picks a decomposition with ONE contributing workgroup per
 * accumulated address (no split reductions, one-block reduction tails, gather-form adjoints), and fmi_attention_bwd_det_f32 replaces the
 * atomic dQ by per-key-block partial tiles added in a fixed order: two runs are bit-identical.  Slower; a checking mode.
 * fmi_set_deterministic returns the previous setting. */
int fmi_set_deterministic(int on);
int fmi_get_deterministic(void);

/* ------------------------------------------------------------------------
 * Dense batched GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 *   C[b] = alpha * A[b] . B[b] (+ bias[n]) + beta * C[b]
 * A is M x K with element strides (sa_m, sa_k), one of which must be 1;
 * B is K x N with (sb_k, sb_n), one of which must be 1; C has (sc_m, sc_n).
 * Replaces torch.bmm / @ at example_guided_att.py:17,31, base_function.py:433,437,
 * external_function.py:184,253 and F.linear at stylegan2/model.py:160-165.
 * ---------------------------------------------------------------------- */
int fmi_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K,
                 int64_t sa_m, int64_t sa_k, int64_t sb_k, int64_t sb_n, int64_t sc_m, int64_t sc_n,
                 int batch, int64_t sa_b, int64_t sb_b, int64_t sc_b,
                 float alpha, float beta, const float* bias, void* stream);

/* ------------------------------------------------------------------------
 * Convolution family as implicit GEMM (im2col gather -> LDS -> fp32 MFMA).
 * All three entry points are described by the FORWARD convolution
 *      y[N,OH,OW,K] = conv(x[N,H,W,C], w[K,C,kh,kw], stride, pad)
 *      OH = (H + 2*pad - kh)/stride + 1
 * A ConvTranspose2d (base_function.py:326-341) is the adjoint of that conv:
 * its forward is fmi_conv2d_dgrad_f32, its input-gradient fmi_conv2d_fwd_f32
 * and its weight-gradient fmi_conv2d_wgrad_f32 with x/dy exchanged.
 * Weights are consumed in two packed layouts produced by fmi_weight_prepare:
 *      wf[tap][C][K]   (tap = kh_i*kw + kw_i)  used by fwd, produced by wgrad
 *      wt[tap][K][C]                            used by dgrad
 * batch_w > 1 selects per-sample weights (ModulatedConv2d, stylegan2/model.py:
 * 241-279): sample n uses w + n*w_bstride and N must equal batch_w.
 * ---------------------------------------------------------------------- */
typedef struct {
  int N, H, W, C;    /* x: conv input (the larger image for stride > 1) */
  int OH, OW, K;     /* y: conv output */
  int x_cstride;     /* floats between consecutive pixels of x (>= C) */
  int y_cstride;     /* floats between consecutive pixels of y (>= K) */
  int kh, kw, stride, pad;
  int pad_mode;      /* 0 = zeros, 1 = reflect (nn.ReflectionPad2d, base_function.py:390) */
  int dil;           /* dilation (modules/drn.py: 2 / 4 in the dilated stages); 0 or 1 = none.  fp32 family only, stride 1 for the adjoint */
  const void* w3;    /* optional (NULL = none): the weight operand of THIS call -- wf for fwd, wt for dgrad -- once more as the three bf16
                        piece images fmi_weight_prepare_f32 writes (entry.wf3 / entry.wt3).  fp32 products run as six bf16 MFMAs on exact
                        three-way splits of both operands; with the pieces at hand only the activations are split inside the kernel.
                        Results do not depend on whether it is given. */
  const void* x3;    /* optional (NULL = none): the ACTIVATION operand of this call -- x for fwd, dy for dgrad -- once more as a bf16 piece
                        image x3[pixel][C/16][piece 0..2][16] (fmi_split3_f32, or the y3 output of the call that produced the tensor).
                        Needs a dense tensor (pixel pitch == channels), channels % 16 == 0, zero padding and w3; the convolution then
                        runs without any split arithmetic (csrc/conv_p3.h).  Results do not depend on whether it is given. */
  void* y3;          /* optional (NULL = none): OUT, the result of this call -- y for fwd, dx for dgrad -- once more as such a piece image
                        (result channels % 16 == 0, dense rows), for the convolution that will consume it (today: a fmi_split3_f32 pass
                        behind the convolution launch) */
} fmi_conv_desc;

/* ------------------------------------------------------------------------
 * GPU side of the data path (dataloader.py:76-93,169-170: PIL resize, HWC -> CHW, / 255, Normalize), csrc/preproc.hip.
 * The host decodes files and computes Pillow's O(W + H) resampling tables; the pixels are produced here in integer arithmetic and
 * equal Pillow's bit for bit.
 *   fmi_resample_u8: one pass of Pillow's 8-bit resampling, out = clip8((2^21 + sum in * kk) >> 22).  axis 0 (along x):
 *     in [N][in_h][in_w][C] -> out [N][rows][out_len][C], output row y reads input row row0 + y; axis 1 (along y):
 *     in [N][in_h][in_w][C] -> out [N][out_len][in_w][C].  bounds[out_len][2] = (first input index, count), kk[out_len][ksize] int32.
 *   fmi_gather_u8_i64: NEAREST resize through index tables, out[n][y][x] = (int64) in[n][ytab[y]][xtab[x]]  (the mask, dataloader.py:80-91)
 *   fmi_u8_lut_chw_f32: out[n][c][p] = lut256[in[n][p][c]]  (v / 255 and the optional Normalize as a 256-entry table)
 * ---------------------------------------------------------------------- */
int fmi_resample_u8(const uint8_t* in, uint8_t* out, int N, int in_h, int in_w, int C, int out_len, int axis, int row0, int rows,
                    const int32_t* bounds, const int32_t* kk, int ksize, void* stream);
int fmi_gather_u8_i64(const uint8_t* in, int64_t* out, int N, int in_h, int in_w, int out_h, int out_w, const int32_t* ytab,
                      const int32_t* xtab, void* stream);
int fmi_u8_lut_chw_f32(const uint8_t* in, const float* lut256, float* out, int N, int H, int W, int C, void* stream);

/* bf16 piece image of a dense NHWC fp32 tensor (C % 16 == 0): x3[pixel][C/16][piece][16], x = x0 + x1 + x2 exactly, x0 = rn_bf16(x),
 * x1 = rn_bf16(x - x0), x2 = x - x0 - x1.  op 0: pieces of x; op 1: pieces of lrelu(x, p0) (the LeakyReLU -> conv pairs of
 * base_function.py:207-305).  y (may be NULL): also receives the fp32 value the pieces were cut from.  fmi_merge3_f32 is the inverse. */
int fmi_split3_f32(const float* x, void* x3, float* y, int64_t pixels, int C, int op, float p0, void* stream);
int fmi_merge3_f32(const void* x3, float* y, int64_t pixels, int C, void* stream);
/* pieces of a gradient tensor dy AND its bias gradient in the same pass: colsum[c] += sum over pixels dy[pixel][c] (fp32 atomics; the
 * reproducible mode takes fmi_bias_grad_f32 instead).  C <= 512 and 256 % (C / 8) == 0, else FMI_ERR_UNSUPPORTED.  Replaces the bias
 * term of Conv2d's backward (torch.nn.Conv2d in base_function.py:207-305) when the weight gradient reads dy as pieces. */
int fmi_split3_colsum_f32(const float* x, void* x3, float* colsum, int64_t pixels, int C, void* stream);

/* y = conv(x, wf) + bias[k] + residual ; bias/residual may be NULL.
 * act: 0 none, 1 tanh, 2 relu, applied last. residual has y's layout. */
int fmi_conv2d_fwd_f32(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias,
                       const float* residual, float* y, int act, int batch_w, int64_t w_bstride, void* stream);
/* dx = conv_adjoint(dy, wt) + bias[c] + residual (dx layout = x's).  With
 * pad_mode = reflect the caller passes H,W of the PADDED input (see
 * fmi_reflect_pad_fold_f32). */
/* y = ConvTranspose2d(x1, W1) + ConvTranspose2d(x2, W2) + bias: the main path and the bypass of ResBlockDecoder (base_function.py:297-305:
 * two nn.ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1) whose results are added) in one launch -- the reduction runs over
 * x1's channels and continues over x2's, so the 1 GB intermediate is neither written nor re-read.  d describes the FIRST transposed
 * convolution exactly as for fmi_conv2d_dgrad_f32 (d->K = channels of x1, d->C = output channels, d->H x d->W = the output, d->w3 = piece
 * image of its adjoint pack, entry.wt3 of fmi_weight_prepare_f32); x2 is dense with K2 channels, w3b its piece image.  Thin outputs on large
 * maps only (d->C <= 64, >= 32 768 input pixels, channels % 16 == 0); FMI_ERR_UNSUPPORTED otherwise: the caller then issues the two
 * fmi_conv2d_dgrad_f32 calls (the second with the first's result as residual). */
int fmi_conv_transpose2d_pair_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int K2, const void* w3b, const float* bias,
                                  float* y, void* stream);
/* Whole backward of fmi_conv_transpose2d_pair_f32 from one read of dy (csrc/convt3x3_bwd.hip): dx1 / dx2 (layouts of x1 / x2),
 * dwf1 [9][C][K] / dwf2 [9][C][K2] and dbias [C] are WRITTEN (no atomics, nothing to zero, bit-identical from run to run in either
 * reproducibility mode); each of the five may be NULL.  d as for the forward (d->C = 32 output channels, d->K = x1's channels), dense
 * tensors, K and K2 in {32, 64}; wf3a / wf3b: the packs' wf3 piece images.  ws: device memory of
 * fmi_conv_transpose2d_pair_bwd_ws_bytes(d, K, K2) bytes, contents irrelevant.  Null descriptor or required pointer, a short workspace
 * or a pointer off 16-byte alignment: FMI_ERR_BAD_ARG; any other geometry: FMI_ERR_UNSUPPORTED (_supported says 0). */
int fmi_conv_transpose2d_pair_bwd_supported(const fmi_conv_desc* d, int K, int K2);
int fmi_conv_transpose2d_pair_bwd_ws_bytes(const fmi_conv_desc* d, int K, int K2);
int fmi_conv_transpose2d_pair_bwd_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int K2, const float* dy, const void* wf3a,
                                      const void* wf3b, float* dx1, float* dx2, float* dwf1, float* dwf2, float* dbias, void* ws,
                                      int64_t ws_bytes, void* stream);
int fmi_conv2d_dgrad_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* bias,
                         const float* residual, float* dx, int batch_w, int64_t w_bstride, void* stream);
/* The stride-1 ResBlock's  y = act(conv3x3(x1, W1) + conv1x1(x2, W2) + b1 + b2)  in one launch (csrc/conv_pair.h): after the 9 * C (tap,
 * channel) reduction steps over x1 the reduction goes on over the C2 channels of x2 at the centre tap.  d describes the 3x3 convolution
 * (kernel 3, stride 1, pad 1, zero padding, dense NHWC, d->C % 16 == 0, d->K % 4 == 0; d->w3 = the piece image of its forward pack or
 * NULL); x2 is dense [N][H][W][C2], C2 % 16 == 0; wf1 [9][C][K], wf2 [C2][K] the forward packs and w3b wf2's piece image (NULL: the fp32
 * packs are read); b1 / b2 may be NULL.  A split reduction (fmi_conv2d_pair_ksplit(d, C2, act) > 1; never with an activation nor in
 * reproducible mode) starts from y = b1 + b2 and adds partial sums atomically.  Any other geometry: FMI_ERR_UNSUPPORTED (_supported says
 * 0); a NULL required pointer or one off 16-byte alignment: FMI_ERR_BAD_ARG; both before any launch.  _routed: which passes of a supported
 * shape were measured faster than the single launches in every round (profiles/resblock_pair.txt): bit 0 the forward, bit 1 the weight
 * gradient; 0: keep the two-launch form.
 * fmi_conv2d_pair_wgrad_f32: dw1 [9][C][K], dw2 [C2][K] and dbias [K] (the gradient of b1 AND of b2; may be NULL) from one walk over dy,
 * ACCUMULATED into zeroed destinations with the pixel split, atomics and reproducible-mode rule of fmi_conv2d_wgrad_f32.  The two input
 * gradients are two fmi_conv2d_dgrad_*_f32 calls. */
int fmi_conv2d_pair_supported(const fmi_conv_desc* d, int C2);
int fmi_conv2d_pair_routed(const fmi_conv_desc* d, int C2);
int fmi_conv2d_pair_ksplit(const fmi_conv_desc* d, int C2, int act);
/* What fmi_conv2d_fwd_f32 (pass 0), fmi_conv2d_dgrad_f32 and its masked forms (1), fmi_conv2d_wgrad_f32 (2) or the ResBlock pair (3 with
 * C2 in pass >> 8) would launch for d -- decided by the code the entries run (csrc/conv_f32_plan.h), without a launch and without a GPU.
 * flags: what the decision reads of a call's pointers and of the process (below).  out[FMI_CONV_F32_PLAN_INTS]:
 *   [0] status as the entry returns it   [1] planned launches of the convolution kernels (0 for an early exit; the phases of a strided
 *   adjoint, at most the first four are listed)   [2] early exit: 11 the thin-output kernels, 12 the thin-input kernels
 *   [3] bit 0 a strided adjoint initialises dx once for all phases, bit 1 the weight gradient fuses the bias gradient, bit 2 its splits are
 *       dealt to the XCDs in groups of 8, bits 4..5 (pair) fmi_conv2d_pair_routed
 *   [4 + 10 p ...] launch p: route (1 GEMM, 2 GEMM on weight pieces, 3 GEMM on piece images, 4 tap-reuse 3x3, 5 tap-reuse 3x3 on weight
 *       pieces, 6 tap-reuse 3x3 on piece images, 7 one-launch ConvTranspose 3x3, 8 / 9 / 10 weight gradient as GEMM / from piece images /
 *       3x3 from piece images), tile (1000 rows + columns), LDS-DMA kernel, blocked accumulation, an initialising launch precedes it,
 *       splits, reduction per split, grid x, grid y, and the code fmi_debug_f32_last_plan reports after that launch.
 *   Pair: launch 0 is its forward, launch 1 its weight gradient (FMI_F32_PLAN_BIAS: with the bias gradient; _W3: both piece images), from
 *   the functions its two entries launch with; X_AL16 (x1, x2), W_AL16 (both packs, dy) and OUT_AL16 must be set, as the entries refuse
 *   a misaligned operand (FMI_ERR_BAD_ARG).
 * The thin kernels' files decide for themselves: in the device build THIN_OUT / THIN_IN are ignored for what fmi_conv2d_thin_supported and
 * fmi_conv2d_thin_in_routed answer; a build without those files (g++ -DFMI_HOST_EMU) is told.  Whether the thin-input ADJOINT takes a call
 * has no predicate: pass 1 reads THIN_IN in both builds.  Returns out[0]; FMI_ERR_BAD_ARG for a null d or out or an unknown pass. */
#define FMI_CONV_F32_PLAN_INTS 44
#define FMI_F32_PLAN_X_AL16 0x1      /* the gathered tensor (x; the adjoint's dy) is 16-byte aligned */
#define FMI_F32_PLAN_W_AL16 0x2      /* the second operand (weights; the weight gradient's dy) is */
#define FMI_F32_PLAN_OUT_AL16 0x4    /* the output is */
#define FMI_F32_PLAN_RES 0x8         /* a residual is given ... */
#define FMI_F32_PLAN_RES_AL16 0x10   /* ... and 16-byte aligned */
#define FMI_F32_PLAN_X3 0x20         /* d->x3 ... */
#define FMI_F32_PLAN_X3_AL16 0x40
#define FMI_F32_PLAN_W3 0x80         /* d->w3 ... */
#define FMI_F32_PLAN_W3_AL16 0x100
#define FMI_F32_PLAN_Y3 0x200        /* d->y3 ... */
#define FMI_F32_PLAN_Y3_AL16 0x400
#define FMI_F32_PLAN_BIAS 0x800      /* bias (weight gradient: dbias) given */
#define FMI_F32_PLAN_MASK 0x1000
#define FMI_F32_PLAN_ACT 0x2000      /* act != 0 */
#define FMI_F32_PLAN_BATCH_W 0x4000  /* per-sample weights: batch_w = d->N */
#define FMI_F32_PLAN_DET 0x8000      /* with FMI_F32_PLAN_MODES: reproducible mode */
#define FMI_F32_PLAN_MODES 0x10000   /* take reproducible mode and FMI_DMA_OFF (bits 17..19) from flags, not from the process */
#define FMI_F32_PLAN_DMA_OFF_SHIFT 17
#define FMI_F32_PLAN_THIN_OUT 0x100000
#define FMI_F32_PLAN_THIN_IN 0x200000
int fmi_conv2d_f32_plan(const fmi_conv_desc* d, int pass, int flags, int* out);
/* Route, kernel form and tile of the last forward, adjoint or weight-gradient launch of the fp32 family: route << 24 | LDS-DMA kernel << 23 |
 * blocked accumulation << 22 | tile, as out[13 + 10 p] of the query names it; 0 before the first.  Each launcher writes it in the branch that
 * launches, from that kernel instantiation's own tile and form, not from the plan.  An early exit to the thin kernels leaves it. */
int fmi_debug_f32_last_plan(void);
int fmi_conv2d_pair_fwd_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int C2, const float* wf1, const float* wf2,
                            const void* w3b, const float* b1, const float* b2, float* y, int act, void* stream);
int fmi_conv2d_pair_wgrad_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int C2, const float* dy, float* dw1, float* dw2,
                              float* dbias, void* stream);
/* Adjoint of  act(x) -> conv : dx = conv_adjoint(dy, wt) * act'(x), act' = (mask > 0 ? 1 : mask_slope); mask = x or act(x), dx's layout.
 * The LeakyReLU -> conv pairs of ResBlock / ResBlockEncoderOptimized (base_function.py:207-305) and the ReLU -> conv pairs inside
 * VGG16 (loss.py:45-65): the multiplication happens in the GEMM epilogue, the separate activation-backward pass disappears.
 * Zero padding, shared weights, no bias / residual. */
int fmi_conv2d_dgrad_masked_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* mask, float mask_slope, float* dx,
                                void* stream);
/* the same with dx = conv_adjoint(dy, wt) * act'(x) + gadd: x's second consumer in a ResBlock (the 1x1 bypass convolution,
 * base_function.py:242-268) hands its gradient in here, so no separate accumulation pass runs */
int fmi_conv2d_dgrad_masked_add_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* mask, float mask_slope,
                                    const float* gadd, float* dx, void* stream);
/* dwf[tap][C][K] += sum over pixels x (gathered) * dy ; fp32 atomics, caller zeroes dwf.
 * With d->x3 (piece image of x) AND d->y3 (here an INPUT: the piece image of dy) given, dbias == NULL, C % 32 == 0, K % 16 == 0 and dense
 * tensors, the product runs on the pieces (csrc/conv_p3.h: transposed LDS reads, no split arithmetic); results agree to fp32 rounding.
 * dbias (may be NULL; needs kh*kw*C % 4 == 0 and batch_w == 1): dbias[k] += sum over pixels dy[p][k], computed by the same
 * GEMM as one extra row of ones -- no separate pass over dy; caller zeroes it. */
int fmi_conv2d_wgrad_f32(const fmi_conv_desc* d, const float* x, const float* dy, float* dwf, float* dbias,
                         int batch_w, int64_t w_bstride, void* stream);
/* Thin-output 3x3 convolution (K <= 4 output channels, stride 1, pad 1, C = 4..64 a power of two): the Output block of
 * the PICNet generator, base_function.py:367-398 (LeakyReLU -> ReflectionPad2d(1) -> conv3x3(32 -> 3) -> tanh) at 1024^2.
 * Bandwidth kernels; fmi_conv2d_fwd_f32 / _wgrad_f32 / _dgrad_f32 (zero padding) route to them by themselves.
 * fmi_conv2d_thin_dgrad_f32 also takes pad_mode = reflect on the UNPADDED extent and includes the fold of the padded gradient
 * (one pass instead of fmi_conv2d_dgrad_f32 on the padded extent + fmi_reflect_pad_fold_f32). */
int fmi_conv2d_thin_supported(const fmi_conv_desc* d);
int fmi_conv2d_thin_fwd_f32(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias,
                            const float* residual, float* y, int act, void* stream);
int fmi_conv2d_thin_dgrad_f32(const fmi_conv_desc* d, const float* dy, const float* wt, float* dx, void* stream);
int fmi_conv2d_thin_wgrad_f32(const fmi_conv_desc* d, const float* x, const float* dy, float* dwf, float* dbias, void* stream);
/* The same thin-output convolution reading lrelu(x, in_slope) -- the whole Output block LeakyReLU -> ReflectionPad2d(1) -> conv3x3 -> tanh
 * (base_function.py:386-396) in ONE pass over the activation per direction: the activation is applied while the halo window is staged
 * (forward, weight gradient), the adjoint multiplies its result by lrelu'(x).  C = 32 only (fmi_conv2d_thin_lrelu_supported). */
int fmi_conv2d_thin_lrelu_supported(const fmi_conv_desc* d);
int fmi_conv2d_thin_lrelu_fwd_f32(const fmi_conv_desc* d, const float* x, float in_slope, const float* wf, const float* bias, float* y, int act,
                                  void* stream);
/* The forward of that block from a bf16 activation (the bf16 PICNet decoder, inference): x [N,H,W,32] bf16 with a pixel pitch of
 * d->x_cstride bf16 elements (a multiple of 8), read as 16-byte chunks of 8 channels; lrelu, taps, bias and act in fp32, y the fp32
 * image [N,H,W,K].  Same geometry as fmi_conv2d_thin_lrelu_supported (ragged H / W included); x 16-byte aligned; else FMI_ERR_UNSUPPORTED. */
int fmi_conv2d_thin_lrelu_fwd_bf16(const fmi_conv_desc* d, const uint16_t* x, float in_slope, const float* wf, const float* bias, float* y,
                                   int act, void* stream);
int fmi_conv2d_thin_lrelu_dgrad_f32(const fmi_conv_desc* d, const float* dy, const float* wt, const float* x, float in_slope, float* dx,
                                    void* stream);
int fmi_conv2d_thin_lrelu_wgrad_f32(const fmi_conv_desc* d, const float* x, float in_slope, const float* dy, float* dwf, float* dbias,
                                    void* stream);
/* Whole backward of that fused block in ONE pass over x: dx = lrelu'(x) * adjoint(dy'), dwf[9][C][K] = lrelu(x)^T dy', dbias[k] = sum dy'
 * (dbias may be NULL), with dy' = dy * (1 - y * y) when y (the tanh output, layout of dy) is given and dy' = dy when y is NULL -- the
 * separate tanh-backward pass disappears.  pad_mode = reflect includes the fold of the padded gradient, as fmi_conv2d_thin_dgrad_f32.
 * dwf and dbias are WRITTEN, not accumulated: nothing has to be zeroed.  The sum over workgroups goes through ws (one row of
 * 9*C*K + K partial sums per workgroup, added in a fixed order by a finishing launch): no atomics, the result is bit-reproducible in
 * either mode.  ws: device memory, fmi_conv2d_thin_lrelu_bwd_ws_bytes(d) =
 *   min(N * ceil(H / 8) * ceil(W / 32), 2048) * (9*C*K + K) * 4 bytes (0 for a shape the entry does not take); a smaller ws (at least
 * one row) only lowers the number of workgroups.  Same shapes as fmi_conv2d_thin_lrelu_supported; x and dx 16-byte aligned. */
int fmi_conv2d_thin_lrelu_bwd_ws_bytes(const fmi_conv_desc* d);
int fmi_conv2d_thin_lrelu_bwd_f32(const fmi_conv_desc* d, const float* x, float in_slope, const float* dy, const float* y, const float* wt,
                                  float* dx, float* dwf, float* dbias, void* ws, int64_t ws_bytes, void* stream);
/* adjoint of a thin-INPUT 3x3 convolution (C <= 4, K = 4..64 a power of two, stride 1, pad 1, zeros): dx = thin-output convolution of
 * dy with flipped taps -- the input gradient of VGG16's first layer (loss.py:45-65); fmi_conv2d_dgrad_f32 routes to it by itself.
 * Dense tensors (x_cstride == C, y_cstride == K) with K = 8 .. 64 run on the streaming kernel of csrc/thinin.hip (dy rows staged once in
 * LDS, plain fp32 FMAs) from 131072 pixels on (fmi_conv2d_thin_in_routed) and, at any size, in the 1x1 pad-0 form, which no other kernel
 * behind this entry takes; the results of every other shape are unchanged. */
int fmi_conv2d_thin_input_dgrad_f32(const fmi_conv_desc* d, const float* dy, const float* wt, float* dx, void* stream);
/* Thin-INPUT convolutions (csrc/thinin.hip): 1 <= C <= 4 with x dense (x_cstride == C), K % 8 == 0, 8 <= K <= 64 with y dense
 * (y_cstride == K), 3x3 pad 1 or 1x1 pad 0, stride 1, no dilation, zero padding, OH == H, OW == W, N*H*W < 2^31 -- the image-facing first
 * layers of the encoders, the discriminator and VGG16.  fmi_conv2d_thin_in_supported says 1 for this class (0 for NULL): what the two
 * entries below accept.  fmi_conv2d_thin_in_routed says 1 for the part of it that the library's own dispatch (fmi_conv2d_fwd_f32,
 * fmi_conv2d_dgrad_f32; both for the 3x3 form only) and functional._Conv2d.backward (weight gradient, 3x3 and 1x1) send to these
 * kernels: N*H*W >= 131072 pixels, the smallest map at which they were timed against the generic path; smaller maps are launch-bound
 * and keep the path (and the bits) they had, and so do the 1x1 forward and input gradient, 9 - 13 us launches either way.  Streaming
 * kernels on plain fp32 FMAs.  Any other geometry: FMI_ERR_UNSUPPORTED; NULL descriptor or required pointer: FMI_ERR_BAD_ARG; both
 * before anything is launched.
 *   fwd  : y = act(conv(x, wf) + bias + residual), wf[taps][C][K], bias / residual may be NULL, act = 0 none / 1 tanh / 2 relu.  y and
 *          residual 16-byte aligned (else FMI_ERR_UNSUPPORTED).  fmi_conv2d_fwd_f32 routes to it by itself (routed 3x3 shapes).
 *   wgrad: dwf[taps][C][K] = x^T dy and, when dbias != NULL, dbias[K] = sum dy, both from ONE read of dy.  Both are WRITTEN, not
 *          accumulated: nothing has to be zeroed.  Persistent workgroups store one row of partial sums each into ws and a finishing launch
 *          adds the rows in a fixed order: no atomics, bit-identical from run to run and in either mode.  dy 16-byte aligned (else
 *          FMI_ERR_UNSUPPORTED).  ws: device memory, 16-byte aligned, fmi_conv2d_thin_in_wgrad_ws_bytes(d) =
 *            min(ceil(N * H * ceil(W / 4) / (256 / P)), 1024) * (taps*C*K + K) * 4 bytes, P = K / 4 rounded up to a power of two
 *          (0 for a shape outside the class); contents irrelevant.  A ws of fewer rows only lowers the number of workgroups; shorter
 *          than one row, misaligned or NULL: FMI_ERR_BAD_ARG.  fmi_conv2d_wgrad_f32 keeps the generic path for these shapes. */
int fmi_conv2d_thin_in_supported(const fmi_conv_desc* d);
int fmi_conv2d_thin_in_routed(const fmi_conv_desc* d);
int fmi_conv2d_thin_in_fwd_f32(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias, const float* residual, float* y,
                               int act, void* stream);
int fmi_conv2d_thin_in_wgrad_ws_bytes(const fmi_conv_desc* d);
int fmi_conv2d_thin_in_wgrad_f32(const fmi_conv_desc* d, const float* x, const float* dy, float* dwf, float* dbias, void* ws,
                                 int64_t ws_bytes, void* stream);
/* ------------------------------------------------------------------------
 * bf16 convolution family (fp32 accumulate) for the StyleGAN2 decoder of the pSp path in configs C3 / C5
 * (stylegan2/model.py:241-279: the grouped conv2d / conv_transpose2d of ModulatedConv2d.forward).  Activations are bf16 NHWC
 * (uint16_t = raw bf16 bits), weights are bf16 copies of the fp32 packs with the REDUCTION index contiguous:
 *   forward : wnk[K][kh*kw][C]   = fmi_pack_weight_bf16(wf[tap][C][K], T=taps, A=C, B=K)
 *   adjoint : wck[C][kh*kw][K]   = fmi_pack_weight_bf16(wt[tap][K][C], T=taps, A=K, B=C)
 * Needs the reduced channel count % 32 == 0, pixel pitches % 8 == 0, 16-byte aligned bases and zero padding
 * (fmi_conv2d_bf16_supported); anything else returns FMI_ERR_UNSUPPORTED -- there is no silent fp32 detour.
 * colscale (may be NULL): [N][out channels] fp32, multiplied into the result per (sample, channel) -- the demodulation factor.
 * The adjoint handles stride 2 by sub-pixel phases, i.e. it is also the ConvTranspose2d forward of the upsampling layers.
 * ws (may be NULL): a ZEROED fp32 buffer of ws_floats >= elements of the output tensor; when given (and colscale is NULL) small
 * feature maps with a deep reduction split it over workgroups (fp32 atomics into ws, then one conversion launch).  All sub-pixel
 * phases of a stride-2 adjoint run in ONE launch; stride > 2 is FMI_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
int fmi_conv2d_bf16_supported(const fmi_conv_desc* d);
/* Kernel selection override of the bf16 convolution family (tests; initial value 0): 0 = by shape,
 * 1 = never the eight-wave tiles, 2 = no eight-phase kernel, 8 = the eight-phase kernel (csrc/conv_bf16_8ph.h) wherever it is legal.
 * mode < 0 only queries.  Returns the previous mode. */
int fmi_debug_bf16_tile(int mode);
/* The tile the last launch of the bf16 forward / adjoint kernels took (tests assert which kernel a shape reached): 1000 BM + BN of the
 * tile (rows x output columns), plus 1000000 for the eight-phase kernel; 0 before the first launch.  Every entry that launches them records
 * it: fmi_conv2d_fwd_bf16, _fwd_act_bf16, _fwd_chan_bf16, the tile path of _grouped_fwd_bf16, _dgrad_bf16 and _dgrad_relu_bf16. */
int fmi_debug_bf16_last_tile(void);
/* The launch one of those entries, or fmi_conv2d_wgrad_bf16, would make for d -- decided by the code the entries run (csrc/conv_bf16_plan.h),
 * without a launch and without a GPU.  pass: 0 forward, 1 adjoint, 2 weight gradient.  stage: 0 plain, 1 the fused StyledConv stage
 * (_fwd_act_), 2 per-column (_fwd_chan_), 3 grouped (groups = G, d per group; a shared map is ONE group of G K columns), 4 masked
 * (_dgrad_relu_).  flags: what the decision reads of a call's pointers, and optionally the two modes.  out[FMI_CONV_BF16_PLAN_INTS]:
 * [0] status (FMI_OK / FMI_ERR_UNSUPPORTED as the entry returns it; the rest is 0 when refused), [1] tile code as above (weight gradient:
 * 128 x {32, 64, 128}, or 256 x 256 + 1000000 for its eight-phase kernel), [2] splits of the reduction, [3..5] grid, [6..9] tiles per
 * phase, [10] column tiles, [11] phases, [12] / [13] the weight gradient's pixels per split / splits dealt to the XCDs in groups of 8.
 * Returns out[0]; FMI_ERR_BAD_ARG for a null d or out, an unknown pass or stage.  Only the descriptor checks common to the entries are
 * made: an entry's own refusals (channel multiples, alignment) are not repeated. */
#define FMI_CONV_BF16_PLAN_INTS 14
#define FMI_PLAN_SPLIT_WS 1       /* a split workspace is offered: 16-byte aligned, at least the output's element count in floats */
#define FMI_PLAN_COLSCALE 2       /* colscale != NULL */
#define FMI_PLAN_COLSCALE_AL16 4  /* ... and 16-byte aligned */
#define FMI_PLAN_OUT_AL8 8        /* the output tensor is 8-byte aligned */
#define FMI_PLAN_DET 16           /* with FMI_PLAN_MODES: reproducible mode */
#define FMI_PLAN_MODES 32         /* take reproducible mode and tile mode (bits 8..11) from flags, not from the library's current settings */
int fmi_conv2d_bf16_plan(const fmi_conv_desc* d, int pass, int stage, int groups, int flags, int* out);
int fmi_conv2d_fwd_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* colscale, uint16_t* y, float* ws,
                        int64_t ws_floats, void* stream);
/* y = lrelu(conv(x, W) * colscale[n][k] + nw[0] * noise[n][oy][ox] + bias[k], slope) * gain in one launch: ModulatedConv2d on pre-scaled
 * activations + demodulation + NoiseInjection + FusedLeakyReLU (stylegan2/model.py:241-294, op/fused_act.py:30-37).  colscale [N][K],
 * noise [N][OH][OW], bias [K] may be NULL.  FMI_ERR_UNSUPPORTED where the eight-phase kernel does not apply (needs C % 64 == 0,
 * K % 4 == 0, y 8-byte and colscale / bias 16-byte aligned).  With colscale = gamma / sqrt(running_var + eps) per sample, bias =
 * beta + (conv_bias - running_mean) * scale, slope 0 and gain 1 this is an eval-mode conv + BatchNorm + ReLU. */
int fmi_conv2d_fwd_act_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* colscale, const float* noise,
                            const float* nw, const float* bias, float slope, float gain, uint16_t* y, void* stream);
int fmi_conv2d_dgrad_bf16(const fmi_conv_desc* d, const uint16_t* dy, const uint16_t* wck, const float* colscale, uint16_t* dx, float* ws,
                          int64_t ws_floats, void* stream);
/* dwf[tap][C][K] (fp32, the layout of fmi_conv2d_wgrad_f32) += sum over pixels x (gathered) * dy; fp32 atomics across the pixel
 * splits, caller zeroes dwf.  Operands reach the matrix cores through ds_read_b64_tr_b16 (the reduction index -- pixels -- is the
 * slow index of both NHWC tensors).  Needs C % 32 == 0, K % 8 == 0. */
int fmi_conv2d_wgrad_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dwf, void* stream);
/* dst[b][t][a] = bf16(src[t][a][b]) */
int fmi_pack_weight_bf16(const float* src_tab, uint16_t* dst_bta, int T, int A, int B, void* stream);
/* bf16 NHWC activations around those convolutions (C % 8 == 0; per-sample / per-channel factors, noise, biases and all reduction
 * results are fp32).  Same semantics as the _f32 entries of the same names:
 *   scale_channels      y = x * s[n][c]                    (modulation / demodulation, model.py:244-252); _gs: gs[n][c] = sum_p g x
 *   noise_bias_act      y = lrelu(x + bias[c] + nw*noise[p], alpha) * scale   (model.py:282-294,340-346; op/fused_act.py:72-85)
 *   noise_bias_act_bwd  gx = g*scale*(y>0 ? 1 : alpha); gbias[c] = sum gx; gnw = sum gx*noise   (ONE pass; either may be NULL)
 * The reductions (_gs, _bwd, torgb_bwd) WRITE their results: each row block stores its partial sums into `ws` (ws_floats fp32, 16-byte
 * aligned, contents irrelevant; the minimum is one partial row per sample, more lets more blocks run -- 2048 rows saturate) and a
 * second small launch adds them: no fp32 atomics (thousands of them on a few hundred addresses serialise), bit-reproducible.
 *   upfirdn2d_nhwc      the decoder's Blur and its gradient only: up = down = 1, square FIR of 2..4 taps (model.py:52-68)
 *   torgb               out[n][p][o<3] = sum_c x w[o][c] s[n][c] + bias[o] + skip   (ToRGB, model.py:349-369; out / skip fp32)
 *   torgb_bwd           gx (bf16), gw[3][C], gs[N][C], gbias[3] (may be NULL); ws_floats >= 2 * N * (3 C + 8)
 * scale_channels and scale_channels_gs also take C % 8 != 0, one element per thread (gs: one workgroup per 64-channel stripe and sample
 * walking P / 4 rows per thread, ws may be NULL) -- for odd widths, not for a body layer.  With C % 8 == 0 they need 16-byte aligned
 * operands, and gs needs C / 8 a power of two <= 256; anything else is FMI_ERR_UNSUPPORTED. */
int fmi_scale_channels_bf16(const uint16_t* x, const float* s, uint16_t* y, int N, int64_t P, int C, void* stream);
int fmi_scale_channels_gs_bf16(const uint16_t* g, const uint16_t* x, float* gs, float* ws, int64_t ws_floats, int N, int64_t P, int C,
                               void* stream);
int fmi_noise_bias_act_bf16(const uint16_t* x, const float* bias, const float* noise, const float* nw, uint16_t* y, int64_t pixels, int C,
                            float alpha, float scale, void* stream);
int fmi_noise_bias_act_bwd_bf16(const uint16_t* g, const uint16_t* y, const float* noise, uint16_t* gx, float* gnw, float* gbias,
                                float* ws, int64_t ws_floats, int64_t pixels, int C, float alpha, float scale, void* stream);
int fmi_upfirdn2d_nhwc_bf16(const uint16_t* in, const float* kernel, uint16_t* out, int N, int in_h, int in_w, int C, int kh, int kw,
                            int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
/* out = lrelu(FIR4x4(in) * colscale[n][c] + nw[0] * noise[n][oy][ox] + bias[c], slope) * gain on bf16 NHWC maps in ONE pass: the Blur of
 * an upsampling StyledConv (stylegan2/model.py:88-91, 268-271) together with the demodulation (:250-252), NoiseInjection (:282-294)
 * and FusedLeakyReLU (op/fused_act.py:30-37) that follow it.  in [N][in_h][in_w][C], out [N][in_h+pad_y0+pad_y1-3][in_w+pad_x0+pad_x1-3][C];
 * kernel: 16 fp32 taps in upfirdn2d's orientation; colscale [N][C], noise [N][OH][OW], bias [C] may each be NULL; C % 32 == 0.
 * separable != 0: the caller states that the taps are an outer product k[i][j] = ky[i] kx[j] (the Blur's kernel is one by construction,
 * model.py:36-45) with k[0][0] != 0; the kernel then filters rows and columns in turn (8 multiplies per output instead of 16). */
int fmi_blur_act_bf16(const uint16_t* in, const float* kernel, uint16_t* out, int N, int in_h, int in_w, int C, int pad_x0, int pad_x1,
                      int pad_y0, int pad_y1, const float* colscale, const float* noise, const float* nw, const float* bias, float slope,
                      float gain, int separable, void* stream);
/* Adjoint of the fused output stage y = lrelu(z * colscale[n][c] + nw[0] * noise[n][p] + bias[c], slope) * gain of fmi_blur_act_bf16 /
 * fmi_conv2d_fwd_act_bf16 in one pass over g and y ([N][P][C] bf16): t = gradient wrt z (bf16), gd [N][C] = gradient wrt colscale,
 * gbias [C], gnw [1] (gd / gbias / gnw may be NULL).  z is not needed: gpre * (z d + nw noise + bias) = g y on both branches of the
 * leaky ReLU.  ws: partial sums, >= N*3*C floats; sums: N*3*C floats (both scratch).  Replaces the autograd chain through
 * FusedLeakyReLU / NoiseInjection / the demodulation product (op/fused_act.py:40-69, model.py:250-252, 282-294). */
int fmi_styled_out_bwd_bf16(const uint16_t* g, const uint16_t* y, const float* noise, const float* colscale, const float* nw,
                            const float* bias, uint16_t* t, float* gd, float* gbias, float* gnw, float* ws, int64_t ws_floats, float* sums,
                            int N, int64_t P, int C, float slope, float gain, void* stream);
int fmi_torgb_fwd_bf16(const uint16_t* x, const float* w, const float* s, const float* bias, const float* skip, float* out, int N,
                       int64_t P, int C, void* stream);
int fmi_torgb_bwd_bf16(const uint16_t* x, const float* w, const float* s, const float* g, uint16_t* gx, float* ws, int64_t ws_floats,
                       float* gw, float* gs, float* gbias, int N, int64_t P, int C, void* stream);

/* dbias[k] = sum over rows of g[rows, cstride] (caller zeroes dbias). */
int fmi_bias_grad_f32(const float* g, int64_t rows, int K, int cstride, float* dbias, void* stream);
/* fold the gradient w.r.t. a reflection-padded tensor [N,H+2p,W+2p,C] back onto [N,H,W,C]. */
int fmi_reflect_pad_fold_f32(const float* gpad, float* gx, int N, int H, int W, int C, int pad, void* stream);

/* ------------------------------------------------------------------------
 * Weight preparation, incl. SpectralNorm (external_function.py:30-41,70-72).
 * One launch handles a whole network: entry i describes one conv weight in the
 * torch layout w[rows][C*taps] (rows = K for Conv2d, = in_channels for
 * ConvTranspose2d, which is also the conv-view K).
 * If u != NULL: `iters` times { v <- normalize(W^T u); u <- normalize(W v) }; sigma = u.(W v);
 * the packed copies hold W / sigma.  If u == NULL the packed copies hold W.
 * ---------------------------------------------------------------------- */
typedef struct {
  const float* w;   /* [rows][C*taps] */
  float* u;         /* [rows] or NULL */
  float* v;         /* [C*taps] or NULL */
  float* wf;        /* out [taps][C][rows] */
  float* wt;        /* out [taps][rows][C] (may be NULL) */
  float* sigma;     /* out [1] (may be NULL when u == NULL) */
  int rows, C, taps;
  int iters;        /* power iterations of the spectral norm (external_function.py:22,36); 0 or 1 = one, as every caller in the reference */
  void* wf3;        /* out, optional: wf as three bf16 piece images [3][taps][C/8][rows][8] (C % 8 == 0, taps <= 36), see fmi_conv_desc.w3 */
  void* wt3;        /* out, optional: wt as three bf16 piece images [3][taps][rows/8][C][8] (rows % 8 == 0, taps <= 36) */
} fmi_weight_entry;
/* entries: HOST array (pointers inside are device pointers); passed to the kernels by value, <= 32 per launch */
int fmi_weight_prepare_f32(const fmi_weight_entry* entries, int count, void* stream);

typedef struct {
  const float* w;      /* [rows][C*taps] */
  const float* u;      /* live u (see DESIGN.md "u/v rebinding") or NULL */
  const float* v;
  const float* sigma;  /* sigma of the forward call this gradient belongs to */
  const float* dwf;    /* [taps][C][rows] gradient w.r.t. the packed effective weight */
  float* dw;           /* out [rows][C*taps], overwritten */
  int rows, C, taps, pad_;
} fmi_weight_grad_entry;
/* entries: HOST array; scratch_zeroed: DEVICE float[count], zero on entry (holds sum dWeff o W per tensor) */
int fmi_weight_grad_f32(const fmi_weight_grad_entry* entries, int count, float* scratch_zeroed, void* stream);

/* ------------------------------------------------------------------------
 * Row softmax over the last dimension (base_function.py:412,430,
 * example_guided_att.py:30) and its backward, in place capable.
 * ---------------------------------------------------------------------- */
int fmi_softmax_rows_f32(const float* x, float* y, int64_t rows, int cols, void* stream);
/* ds = p * (dp - sum_j p*dp) ; ds may alias dp */
int fmi_softmax_rows_bwd_f32(const float* p, const float* dp, float* ds, int64_t rows, int cols, void* stream);

/* Fused flash-style self-attention (queries = keys, no scaling):  O_i = softmax(q q^T) V_i, V = [V1 | V2] along channels.
 * q [N,T,D], v1 [N,T,C1], v2 [N,T,C2] or NULL, outputs o1/o2 alike, lse [N,T] = log sum_j exp(q_i.q_j) (may be NULL).
 * Supported: T % 128 == 0, D in {16,32,64}, C1 % 32 == C2 % 32 == 0, (C1+C2)/32 in {2,4,8}; else FMI_ERR_UNSUPPORTED
 * (callers fall back to the GEMM + softmax composition). */
int fmi_attention_fwd_f32(const float* q, const float* v1, const float* v2, float* o1, float* o2, float* lse,
                          int N, int T, int D, int C1, int C2, void* stream);

/* The shape dispatch of the two fused attention passes (pure host arithmetic; the entry points call these themselves):
 *   fmi_attention_fwd_waves      waves per forward workgroup, each owning 32 queries: 8 if T % 256 == 0 and (T/256) N >= 256,
 *                                else 2 if (T/128) N < 256, else 4
 *   fmi_attention_bwd_structure  2 (one key block per wave) if T % 128 == 0 and (T/128) N >= 128, else 1 (one key block per workgroup) */
int fmi_attention_fwd_waves(int N, int T);
int fmi_attention_bwd_structure(int N, int T);

/* The same forward on bf16 operands (inference, and training with the backward below): q [N,T,D], v [N,T,C] and o [N,T,C] bf16, scores / running maximum / row
 * sum / output accumulators fp32, P rounded to bf16 only as the matrix operand of P V (the row sum adds the fp32 values).
 * Optional epilogue o = gamma[0] * O + residual, computed in fp32 before the one rounding of o: gamma a 1-element fp32 DEVICE tensor,
 * residual bf16 in o's layout (Auto_Attn's gamma * out + x, base_function.py:439); both NULL or both given.  lse [N,T] fp32 as above
 * (may be NULL).  waves: 0 = the shape dispatch fmi_attention_fwd_bf16_waves(N, T) (8 if T % 256 == 0 and (T/256) N >= 256, else 4);
 * 4 or 8 request that workgroup form explicitly (8 needs T % 256 == 0) -- same bits either way is NOT promised, same accuracy is.
 * Supported: T % 128 == 0, (D, C) in {(64, 256), (32, 128)}, N <= 65535; else FMI_ERR_UNSUPPORTED before any launch.  NULL q / v / o,
 * a lone gamma or residual, q / v / o / residual off 16-byte alignment: FMI_ERR_BAD_ARG.  There is no fp32 detour. */
int fmi_attention_fwd_bf16_waves(int N, int T);
int fmi_attention_fwd_bf16(const uint16_t* q, const uint16_t* v, uint16_t* o, float* lse, const float* gamma, const uint16_t* residual,
                           int N, int T, int D, int C, int waves, void* stream);

/* Backward of fmi_attention_fwd_bf16 without its epilogue (csrc/attention_bwd_bf16.hip), K = Q and no scaling as there:
 *     P = exp(S - lse),  dP = go V^T,  dS = P o (dP - delta),  gv = P^T go,  gq = dS Q + dS^T Q.
 *   fmi_attention_bwd_prep_bf16  one pass over go (fp32 [N,T,C], the gradient of O) and o (bf16, as the forward stored it): writes
 *                                go16 = bf16(go) (round to nearest even) and delta[n,t] = sum_c go o (fp32 products and sum, from the
 *                                unrounded go).  No atomics: one thread group owns a row.
 *   fmi_attention_bwd_bf16       q16 [N,T,D], v16 / go16 [N,T,C] bf16, lse / delta [N,T] fp32 -> gq [N,T,D], gv [N,T,C] fp32.  Two launches:
 *                                key-stationary (gv and the key-side half dS^T Q of gq, plain stores), then query-stationary (the
 *                                query-side half dS Q, added by the row's one owner).  No float atomics, no hand-off between
 *                                workgroups: two runs give the same bits whatever fmi_set_deterministic says.  gq and gv need no zeroing.
 * Rounding: q16, v16, go16, and P and dS as matrix operands, are rounded to bf16 once each; scores, exp, dP - delta and all accumulators
 * are fp32.  Supported: T % 128 == 0, (D, C) in {(64, 256), (32, 128)}, N <= 65535; else FMI_ERR_UNSUPPORTED before any launch.  A NULL
 * pointer or one off 16-byte alignment: FMI_ERR_BAD_ARG. */
int fmi_attention_bwd_prep_bf16(const float* go, const uint16_t* o, uint16_t* go16, float* delta, int N, int T, int D, int C, void* stream);
int fmi_attention_bwd_bf16(const uint16_t* q, const uint16_t* v, const uint16_t* go16, const float* lse, const float* delta, float* gq,
                           float* gv, int N, int T, int D, int C, void* stream);

/* The same forward with the bf16 pieces of K (= q) and V cut ONCE per pass into a key-tile image (layout: csrc/attention.hip, AttKImg)
 * that every workgroup streams into LDS by LDS-DMA; bit-identical results (the same pieces in the same MFMA order).
 *   fmi_attention_fwd_uses_pieces   1 where the library's shape dispatch takes this path (T % 256 == 0, (T/256) N >= 256, D in {32,64},
 *                                   (C1+C2)/32 in {4,8}); callers take fmi_attention_fwd_f32 elsewhere
 *   fmi_attention_fwd_image_bytes   size of the image workspace (0: the shape has none)
 *   fmi_attention_fwd_pieces_f32    cuts the image (workspace `image`, 16-byte aligned) and runs the forward; accepts every
 *                                   T % 256 == 0 of the supported D / C, also below the dispatch threshold */
int fmi_attention_fwd_uses_pieces(int N, int T, int D, int C1, int C2);
int fmi_attention_fwd_image_bytes(int N, int T, int D, int C1, int C2, int64_t* bytes);
int fmi_attention_fwd_pieces_f32(const float* q, const float* v1, const float* v2, void* image, int64_t image_bytes, float* o1, float* o2,
                                 float* lse, int N, int T, int D, int C1, int C2, void* stream);

/* Backward of fmi_attention_fwd_f32 (P recomputed from lse): gv1/gv2 [N,T,C] overwritten, gq_zeroed [N,T,D] accumulated with
 * fp32 atomics (caller zeroes it), delta_scratch [N,T] workspace.  Supported: T % 128 == 0 (the forward's: lse must be the one
 * fmi_attention_fwd_f32 wrote, P = exp(S - lse) relies on its rounding of the scores), D in {32,64}, (C1+C2)/32 in {4,8}; else
 * FMI_ERR_UNSUPPORTED, before anything is launched. */
int fmi_attention_bwd_f32(const float* q, const float* v1, const float* v2, const float* o1, const float* o2,
                          const float* go1, const float* go2, const float* lse, float* delta_scratch,
                          float* gv1, float* gv2, float* gq_zeroed, int N, int T, int D, int C1, int C2, void* stream);

/* The same backward with the bf16 pieces of gO and Q cut ONCE per pass into a query-tile image (layout: csrc/attention.hip, AttQImg)
 * that every workgroup streams into LDS by LDS-DMA, instead of every workgroup splitting every tile itself.  Same results as the
 * key-block structure of fmi_attention_bwd_f32 (the same pieces in the same MFMA order; dQ meets through the same atomics).
 *   fmi_attention_bwd_uses_pieces   1 where the library's shape dispatch takes this path (T % 128 == 0, (T/128) N >= 128, D in {32,64},
 *                                   (C1+C2)/32 in {4,8}); callers take fmi_attention_bwd_f32 elsewhere
 *   fmi_attention_bwd_image_bytes   size of the image workspace (0: the shape has none); the only place the layout arithmetic lives
 *   fmi_attention_bwd_pieces_f32    cuts the image (workspace `image`, 16-byte aligned, image_bytes >= the size above) and runs the
 *                                   backward; accepts every T % 128 == 0 of the supported D / C, also below the dispatch threshold */
int fmi_attention_bwd_uses_pieces(int N, int T, int D, int C1, int C2);
int fmi_attention_bwd_image_bytes(int N, int T, int D, int C1, int C2, int64_t* bytes);
int fmi_attention_bwd_pieces_f32(const float* q, const float* v1, const float* v2, const float* o1, const float* o2,
                                 const float* go1, const float* go2, const float* lse, float* delta_scratch, void* image,
                                 int64_t image_bytes, float* gv1, float* gv2, float* gq_zeroed, int N, int T, int D, int C1, int C2,
                                 void* stream);

/* ------------------------------------------------------------------------
 * Bandwidth-class element-wise kernels (float4 vectorised).
 * ---------------------------------------------------------------------- */
enum {
  FMI_EW_LRELU = 0,        /* y = x > 0 ? x : p0*x            (nn.LeakyReLU / ReLU with p0 = 0) */
  FMI_EW_LRELU_BWD = 1,    /* y = a * (b > 0 ? 1 : p0)        a = grad, b = forward input */
  FMI_EW_TANH_BWD = 2,     /* y = a * (1 - b*b)               b = forward output */
  FMI_EW_ADD = 3,          /* y = a + b */
  FMI_EW_SCALE = 4,        /* y = p0 * a */
  FMI_EW_AXPY = 5,         /* y = p0 * a + b */
  FMI_EW_MUL = 6,          /* y = a * b */
  FMI_EW_RELU_BWD_OUT = 7, /* y = a * (b > 0)                 b = forward output */
  FMI_EW_SOFTPLUS = 8,     /* y = log1p(exp(a)) (threshold 20, F.softplus) */
  FMI_EW_SOFTPLUS_BWD = 9, /* y = a * sigmoid(b)              b = forward input */
  FMI_EW_SUB = 10,         /* y = a - b */
  FMI_EW_RSQRT = 11,       /* y = rsqrt(a + p0) */
  FMI_EW_RSQRT_BWD = 12,   /* y = -0.5 * a * b^3          a = grad, b = forward output */
  FMI_EW_SIGMOID = 13,     /* y = 1 / (1 + exp(-a)) */
  FMI_EW_SIGMOID_BWD = 14, /* y = a * b * (1 - b)         b = forward output */
  FMI_EW_COUNT_
};
int fmi_eltwise_f32(int op, const float* a, const float* b, float* y, int64_t n, float p0, void* stream);
/* y = a * s[0] + b (b may be NULL), s is a 1-element DEVICE tensor (Auto_Attn gamma, base_function.py:439) */
int fmi_axpy_dev_f32(const float* a, const float* s, const float* b, float* y, int64_t n, void* stream);
/* out[0] += scale * sum(a*b)  (caller zeroes out) */
int fmi_dot_f32(const float* a, const float* b, int64_t n, float scale, float* out, void* stream);

/* mask helpers (train_reference_fill.py:340, loss.py:88-95, example_guided_att.py:35) */
int fmi_mask_binarise_i64(const int64_t* mask, float* out, int64_t n, void* stream);          /* (m > 0) ? 1 : 0, bit exact */
/* y[p,c] = x[p,c] * (invert ? 1 - m[p] : m[p]) */
int fmi_mask_mul_f32(const float* x, const float* m, float* y, int64_t pixels, int C, int invert, void* stream);
/* out[p, 0:C] = (1-m[p]) * ref_att[p,:] + m[p] * ref[p,:]   (out pixel stride out_cstride) */
int fmi_guide_blend_f32(const float* ref_att, const float* ref, const float* m, float* out,
                        int64_t pixels, int C, int out_cstride, void* stream);
/* backward: g has pixel stride g_cstride; d_ref_att = (1-m) g ; d_ref = m g */
int fmi_guide_blend_bwd_f32(const float* g, const float* m, float* d_ref_att, float* d_ref,
                            int64_t pixels, int C, int g_cstride, void* stream);
/* z[p, 0:Z] = o_src[p,0:Z] + softplus(o_src[p,Z:2Z]) * eps_q ; z[p, Z:2Z] likewise from o_ref/eps_p
 * (network.py:167-168,275-307 with the normal draws injected). */
int fmi_vae_sample_f32(const float* o_src, const float* o_ref, const float* eps_q, const float* eps_p,
                       float* z, int64_t pixels, int Z, void* stream);
int fmi_vae_sample_bwd_f32(const float* gz, const float* o_src, const float* o_ref, const float* eps_q,
                           const float* eps_p, float* g_src, float* g_ref, int64_t pixels, int Z, void* stream);

/* ------------------------------------------------------------------------
 * Pooling / resampling / normalisation (NHWC).
 * ---------------------------------------------------------------------- */
/* k x k mean pooling, stride k (nn.AvgPool2d(2,2) base_function.py:233; AdaptiveAvgPool2d 1024->256 model.py:79) */
int fmi_avgpool_f32(const float* x, float* y, int N, int H, int W, int C, int k, void* stream);
int fmi_avgpool_bwd_f32(const float* gy, float* gx, int N, int H, int W, int C, int k, void* stream);
/* ---- bf16 activations for the IR-SE50 body of the pSp encoder (helpers.py:56-119; SURVEY.md 8a part B: bf16 compute, fp32
 * accumulate / parameters): NHWC bf16 tensors, fp32 statistics, slopes, gates and reduction results.  C % 8 == 0 (C % 4 for the norms).
 * The BatchNorm2d kernels are the instance-norm kernels above on bf16 tensors (gadd of the backward may be NULL). ---- */
int fmi_instnorm_stats_bf16(const uint16_t* x, double* sums, float* stats, int N, int HW, int C, float eps, double* ws, int64_t ws_doubles,
                            void* stream);
int fmi_instnorm_apply_bf16(const uint16_t* x, const float* stats, const float* gamma, const float* beta, uint16_t* y, int N, int HW, int C,
                            float slope, void* stream);
int fmi_instnorm_bwd_reduce_bf16(const uint16_t* x, const uint16_t* gy, const float* stats, const float* gamma, const float* beta, double* red,
                                 int N, int HW, int C, float slope, double* ws, int64_t ws_doubles, void* stream);
int fmi_instnorm_bwd_apply_bf16(const uint16_t* x, const uint16_t* gy, const float* stats, const float* gamma, const float* beta,
                                const double* red, const uint16_t* gadd, uint16_t* gx, float* dgamma, float* dbeta, int N, int HW, int C,
                                float slope, void* stream);
/* nn.PReLU(C) (helpers.py:105) and its backward; ga[C] is WRITTEN (partials workspace ws of >= C floats, ideally 512 C) */
int fmi_prelu_bf16(const uint16_t* x, const float* a, uint16_t* y, int64_t rows, int C, void* stream);
int fmi_prelu_bwd_bf16(const uint16_t* g, const uint16_t* x, const float* a, uint16_t* gx, float* ga, float* ws, int64_t ws_floats, int64_t rows,
                       int C, void* stream);
/* SE gate x residual add (helpers.py:64-72,116-118), plain residual add, AdaptiveAvgPool2d(1) -> fp32 [N][C] (ws >= N C floats), the
 * gradient of the pooled branch joined with the scaled branch's (gx = g + gpool[n][c] / P), MaxPool2d(1, stride) and its backward */
int fmi_scale_channels_add_bf16(const uint16_t* x, const float* s, const uint16_t* res, uint16_t* y, int N, int64_t P, int C, void* stream);
int fmi_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, int64_t n, void* stream); /* n % 8 != 0: scalar form */
int fmi_global_avgpool_bf16(const uint16_t* x, float* pooled, float* ws, int64_t ws_floats, int N, int64_t P, int C, void* stream);
int fmi_add_bcast_bf16(const uint16_t* g, const float* gpool, uint16_t* gx, int N, int64_t P, int C, void* stream);
/* fp32 twin: gx[n][p][c] = g[n][p][c] + gpool[n][c] / P -- the two gradients of an SE module's input (helpers.py:38-54: avg_pool and the
 * gated product both read it) in one pass.  C % 4 == 0, 16-byte aligned pointers. */
int fmi_add_bcast_f32(const float* g, const float* gpool, float* gx, int N, int64_t P, int C, void* stream);
int fmi_subsample_bf16(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int stride, int backward, void* stream);
/* y = x * s[n][c] + res: SE gate and residual add of a bottleneck_IR_SE block (helpers.py:64-72,116-118) in one pass (C % 4 == 0) */
int fmi_scale_channels_add_f32(const float* x, const float* s, const float* res, float* y, int N, int64_t P, int C, void* stream);
/* Both gradients of y = x * s[n][c] (fp32 NHWC, s [N][C]) in one pass: gx = g * s, gs[n][c] = sum_p g * x -- the SE gate of the IR-SE
 * blocks (helpers.py:38-54 under autograd), the modulation / demodulation products (model.py:244-252).  C % 4 == 0, C <= 1024, 16-byte
 * aligned pointers; ws: >= N * C floats of scratch. */
int fmi_scale_channels_bwd_f32(const float* g, const float* x, const float* s, float* gx, float* gs, float* ws, int64_t ws_floats, int N,
                               int64_t P, int C, void* stream);
/* fmi_instnorm_bwd_apply_f32 with gx += gadd: the gradient of a second consumer of x (the identity shortcut of an IR block) joins in the
 * same pass */
int fmi_instnorm_bwd_apply_add_f32(const float* x, const float* gy, const float* stats, const float* gamma, const float* beta,
                                   const double* red, const float* gadd, float* gx, float* dgamma, float* dbeta, int N, int HW, int C,
                                   float slope, void* stream);
/* y[r][:] = x[r][:] / (||x[r]|| + eps), inv_norm[r] = 1 / (||x[r]|| + eps): LPIPS' normalize_activation over the channels of a
 * pixel (criteria/lpips/utils.py:6-8, eps 1e-10) and ArcFace's l2_norm of an embedding (encoders/helpers.py:15-18, eps 0) */
int fmi_l2norm_rows_f32(const float* x, float* y, float* inv_norm, int64_t rows, int C, float eps, void* stream);
int fmi_l2norm_rows_bwd_f32(const float* g, const float* y, const float* inv_norm, float* gx, int64_t rows, int C, float eps, void* stream);
/* out[0] += scale * sum_p sum_c w[c] (fx[p][c] - fy[p][c])^2: one layer of LPIPS.forward (criteria/lpips/lpips.py:33-36: squared
 * difference, 1x1 lin convolution, spatial mean, batch sum) in one pass; caller zeroes out.  Backward: gfx / gfy may be NULL */
int fmi_lpips_layer_f32(const float* fx, const float* fy, const float* w, float* out, int64_t pixels, int C, float scale, void* stream);
int fmi_lpips_layer_bwd_f32(const float* fx, const float* fy, const float* w, const float* gout, float* gfx, float* gfy, int64_t pixels,
                            int C, float scale, void* stream);
/* dst[r][dst_c0 + j] = src[r][src_c0 + j] for j < c: channel slice / concatenation of NHWC maps (model.py:106 return_zq;
 * unet_parts.py:70 and example_guided_att.py:37 torch.cat) */
int fmi_copy_channels_f32(const float* src, float* dst, int64_t rows, int src_stride, int src_c0, int dst_stride, int dst_c0, int c,
                          void* stream);
/* the same for bf16 maps; strides, offsets and c in bf16 elements, all multiples of 8, 16-byte aligned bases (else FMI_ERR_UNSUPPORTED) */
int fmi_copy_channels_bf16(const uint16_t* src, uint16_t* dst, int64_t rows, int src_stride, int src_c0, int dst_stride, int dst_c0, int c,
                           void* stream);
/* nn.AdaptiveAvgPool2d for any input / output size (model.py:79,111 on non-1024 decoder outputs; psp.py:33 on outputs smaller than
 * 256; id_loss.py:19 188 -> 112): window i of an axis = [floor(i L / OL), ceil((i + 1) L / OL)).  NHWC. */
int fmi_adaptive_avgpool_f32(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, void* stream);
int fmi_adaptive_avgpool_bwd_f32(const float* gy, float* gx, int N, int H, int W, int C, int OH, int OW, void* stream);
/* nn.MaxPool2d(k, stride), no padding, floor mode (criteria/lpips/networks.py: AlexNet trunk k 3 stride 2); argmax[N,OH,OW,C]
 * (may be NULL) = window position of the first maximum; the backward scatters with atomics, caller zeroes gx */
int fmi_maxpool_f32(const float* x, float* y, int32_t* argmax, int N, int H, int W, int C, int k, int stride, void* stream);
int fmi_maxpool_bwd_f32(const float* gy, const int32_t* argmax, float* gx, int N, int H, int W, int C, int k, int stride, void* stream);
/* The image tail of pSp inference, from ONE read of the decoder's image x [N][S][S][3] (NHWC fp32, what ToRGB returns; S = 256 f,
 * f in {1, 2, 4}).  Each output may be NULL (not wanted), at least one is given:
 *   pooled [N][3][256][256] fp32 = nn.AdaptiveAvgPool2d((256, 256)) (modules/psp/psp.py:33,113-114 face_pool): every window summed
 *          row-major, one multiply by 1 / f^2 -- independent of the launch shape; a plain transposition for f = 1;
 *   unit   [N][3][256][256] fp32 = (pooled + 1) / 2, the operand of SSIM / MS-SSIM in psp_inference.py:116-117 (evaluate);
 *   u8     [N][256][256][3] uint8 = tensor2im (psp_inference.py:106-112 with (shift, scale) = (1, 0.5); gradio_serve.py:45-51 with
 *          (0, 1)): t = (pooled + shift) * scale, t < 0 -> 0, t > 1 -> 1, t * 255, truncation; every step one rounded fp32 operation
 *          (never contracted into an FMA), so it equals numpy float32 on ``pooled`` bit for bit.  NaN -> 0 (outside the contract).
 * x, pooled, unit 16-byte and u8 4-byte aligned, else FMI_ERR_BAD_ARG; any other S is FMI_ERR_UNSUPPORTED (callers keep
 * fmi_avgpool_f32 / fmi_adaptive_avgpool_f32 for those). */
int fmi_image_tail_f32(const float* x, float* pooled, float* unit, uint8_t* u8, int N, int S, float shift, float scale, void* stream);
/* The same uint8 conversion for planar input: x [N][C][H][W] fp32 -> u8 [N][H][W][3], any H, W.  C = 3 (the resized image of
 * gradio_serve.py:59-63) or C = 1 with the channel replicated (the detected mask: psp_inference.py:183-184
 * tensor2im(mask.repeat((3, 1, 1))), gradio_serve.py:60); other C are FMI_ERR_UNSUPPORTED. */
int fmi_planes_to_u8_f32(const float* x, uint8_t* u8, int N, int C, int H, int W, float shift, float scale, void* stream);
/* out[p] = (float) argmax_c x[p][c] (first maximum wins, NaN is the maximum): PICNet_inference.py:100-101
 * mask_detector(src, 'train').argmax(1).float(); bit exact */
int fmi_argmax_channels_f32(const float* x, float* out, int64_t pixels, int C, void* stream);
/* 2x2 max pooling (VGG16 features, loss.py:21-25); backward routes to the first maximum */
int fmi_maxpool2_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
int fmi_maxpool2_bwd_f32(const float* x, const float* gy, float* gx, int N, int H, int W, int C, void* stream);
/* bilinear, align_corners=True (model.py:10-12) with the optional per-channel normalisation
 * y = (v - mean[c]) / std[c] of the VGG input (loss.py:51-52) fused in; in/out NHWC */
int fmi_resize_bilinear_f32(const float* x, float* y, int N, int H, int W, int C, int OH, int OW,
                            const float* ch_mean, const float* ch_std, void* stream);
/* gx += ... (atomic scatter; caller zeroes gx) */
int fmi_resize_bilinear_bwd_f32(const float* gy, float* gx, int N, int H, int W, int C, int OH, int OW,
                                const float* ch_std, void* stream);
/* InstanceNorm2d(affine) (base_function.py:47): stats[n][c] = {mean, rstd}; y = act((x-mean)*rstd*g + b),
 * act = LeakyReLU(slope) fused when slope != 1.
 * ws (may be NULL): fp64 partials workspace of ws_doubles >= N*C*2 doubles (contents irrelevant; ~1024*C*2 lets every CU stream).
 * With it each workgroup stores its partial sums as one row and a second launch adds the rows: sums / red are WRITTEN.  Without it
 * the workgroups add onto the caller-ZEROED sums / red with fp64 atomics (which serialise per address: slower, and not
 * bit-reproducible). */
int fmi_instnorm_stats_f32(const float* x, double* sums /*[N][C][2]*/, float* stats /*[N][C][2]*/,
                           int N, int HW, int C, float eps, double* ws, int64_t ws_doubles, void* stream);
int fmi_instnorm_apply_f32(const float* x, const float* stats, const float* gamma, const float* beta, float* y,
                           int N, int HW, int C, float slope, void* stream);
/* nn.BatchNorm2d running statistics (helpers.py:83-113 run BatchNorm2d in training mode) from stats[C][2] = (mean, rstd) of the batch:
 * running = (1 - momentum) * running + momentum * (mean | unbiased variance), num_batches_tracked[0] += 1 (may be NULL).
 * sums[C][2] (may be NULL) = the fp64 (sum, sum of squares) fmi_instnorm_stats_f32 wrote: the variance is then taken from them
 * instead of being reconstructed as 1 / rstd^2 - eps */
int fmi_batchnorm_running_update_f32(const float* stats, const double* sums, float* running_mean, float* running_var,
                                     int64_t* num_batches_tracked, int C, int64_t count, float eps, float momentum, void* stream);
/* the same update for a tensor that was normalised WITHOUT a per-channel constant that cancels in the mean subtraction (the bias of the
 * convolution in front): running_mean takes batch mean + mean_offset[c], the value the path that applies the constant stores */
int fmi_batchnorm_running_update_offset_f32(const float* stats, const double* sums, const float* mean_offset, float* running_mean,
                                            float* running_var, int64_t* num_batches_tracked, int C, int64_t count, float eps,
                                            float momentum, void* stream);
/* backward of y = lrelu(IN(x)): red[n][c] = {sum g', sum g'*xhat} (ws as above), then gx; dgamma/dbeta += */
int fmi_instnorm_bwd_reduce_f32(const float* x, const float* gy, const float* stats, const float* gamma,
                                const float* beta, double* red, int N, int HW, int C, float slope, double* ws, int64_t ws_doubles,
                                void* stream);
int fmi_instnorm_bwd_apply_f32(const float* x, const float* gy, const float* stats, const float* gamma,
                               const float* beta, const double* red, float* gx, float* dgamma, float* dbeta,
                               int N, int HW, int C, float slope, void* stream);

/* ------------------------------------------------------------------------
 * Reductions for the losses (loss.py:58-64,97-118; external_function.py:110-131,187-192).
 * kind: 0 = sum |a-b| , 1 = sum (a-b)^2 , 2 = sum (a-c0)^2 (b ignored)
 * out[0] += scale * reduction  (double-precision accumulation; caller zeroes out)
 * ---------------------------------------------------------------------- */
int fmi_reduce_loss_f32(int kind, const float* a, const float* b, int64_t n, float c0, float scale,
                        float* out, void* stream);
/* gradient of the above w.r.t. a: ga = gscale[0]*scale * d/da ; gscale is a DEVICE scalar (upstream grad) */
int fmi_reduce_loss_bwd_f32(int kind, const float* a, const float* b, int64_t n, float c0, float scale,
                            const float* gscale, float* ga, void* stream);


/* SSIM metric (modules/evaluations/ssim.py:18-38): NCHW planes, window = outer product of window1d[ws], zero padding;
 * out[plane / planes_per_out] += sum over the plane's pixels of the ssim map (caller zeroes out and divides). */
int fmi_ssim_f32(const float* img1, const float* img2, const float* window1d, int ws, int planes, int H, int W,
                 int planes_per_out, float* out_zeroed, void* stream);
/* SSIM / MS-SSIM as the trainers' metric package computes them (pytorch_msssim -- third-party, absent from /root/reference and offline:
 * train_reference_fill.py:207-209,252-257, train_psp.py:176-178, PICNet_inference.py:130-131; parity unpinned): Gaussian window
 * WITHOUT padding; out_plane2[plane] = (mean of the ssim map, mean of its contrast-structure factor cs) over the (H-ws+1) x (W-ws+1)
 * valid positions.  ws_part: fp64 scratch of >= planes * 64 * 2 entries (per-workgroup partial sums, added in a fixed order:
 * reproducible).  fmi_avgpool2_pad_f32: the 2 x 2 mean pool between the scales of MS-SSIM (zero padding 0 / 1 per axis, counted in
 * the divisor); y is [planes][(H + 2 ph - 2) / 2 + 1][(W + 2 pw - 2) / 2 + 1]. */
int fmi_ssim_valid_f32(const float* img1, const float* img2, const float* window1d, int ws, int planes, int H, int W, float C1, float C2,
                       float* out_plane2, double* ws_part, int64_t ws_doubles, void* stream);
int fmi_avgpool2_pad_f32(const float* x, float* y, int planes, int H, int W, int pad_h, int pad_w, void* stream);

/* ------------------------------------------------------------------------
 * The mask-detector trainer's loss and metric (csrc/segloss.hip).  logits: NHWC fp32 [P][C], P = N * H * W, 2 <= C <= 8 (any other C is
 * FMI_ERR_BAD_ARG; C = 2 is MaskDetector's).  target: target_kind 0 = the dataset's int64 map, 1 = an fp32 map; the class of a pixel is
 * (target > 0) -- the `(true_masks > 0)` of train_mask_detector.py:127 is applied in the kernel.  logits / target / dlogits 16-byte
 * aligned.  ws_part: fp64 scratch for the per-workgroup partial rows, added in a fixed order by a finishing launch (no atomics, nothing
 * to zero, bit-reproducible in either mode).
 * ---------------------------------------------------------------------- */
/* train_mask_detector.py:131-134: nn.CrossEntropyLoss()(logits, t) + dice_loss(softmax(logits, 1).float(), one_hot(t, C).permute(0, 3, 1, 2)
 * .float(), multiclass=True) with modules/loss.py:148-186, from one pass over logits and target.  out3 = (ce, dice, ce + dice) with
 * ce = mean_p -log p_t and dice = 1 - mean_c (2 I_c + eps) / (sum p_c + sum t_c + eps), dice_coeff's `sets_sum == 0 -> 2 * inter`
 * branch (loss.py:159-160) evaluated on the device.  sums[1 + 3 C] (fp64, kept for the backward) = sum -log p_t, then I_c = sum p_c t_c,
 * sum p_c, sum t_c per class.  ws_doubles >= 1024 * (1 + 3 C). */
int fmi_seg_ce_dice_fwd_f32(const float* logits, const void* target, int target_kind, int64_t P, int C, double eps, float* out3,
                            double* sums, double* ws_part, int64_t ws_doubles, void* stream);
/* the backward of the above (autograd through train_mask_detector.py:131-137) in one pass that recomputes the softmax:
 * dlogits[p][k] = g p_k (h_k - sum_j p_j h_j) + g (p_k - t_k) / P,  h_c = -(1 / C) (2 t_c (U_c + eps) - (2 I_c + eps)) / (U_c + eps)^2,
 * U_c = sum p_c + sum t_c; gout is a DEVICE scalar (the upstream gradient of ce + dice), sums is what the forward left */
int fmi_seg_ce_dice_bwd_f32(const float* logits, const void* target, int target_kind, int64_t P, int C, double eps, const double* sums,
                            const float* gout, float* dlogits, void* stream);
/* the validation metric of evaluate() (train_mask_detector.py:34-35,47-49): multiclass_dice_coeff(one_hot(argmax)[:, 1:], one_hot(t)[:, 1:],
 * reduce_batch_first=False) -- per sample the argmax over classes (first maximum wins, as torch.argmax), dice_coeff per (sample, class
 * 1 .. C-1) including its empty branch ((0 + eps) / (0 + eps) = 1), mean over classes, mean over samples -> out[0].
 * logits [N][HW][C]; ws_doubles >= N * 64 * 3 * (C - 1); N <= 65535. */
int fmi_seg_dice_score_f32(const float* logits, const void* target, int target_kind, int N, int64_t HW, int C, double eps, float* out,
                           double* ws_part, int64_t ws_doubles, void* stream);
/* out3[plane] = (sum a b, sum a, sum b) in fp64 over planes of n elements of two fp32 tensors: the torch.dot / torch.sum calls of
 * dice_coeff (modules/loss.py:157-158) for arbitrary inputs.  ws_doubles >= planes * (planes == 1 ? 256 : 64) * 3; planes <= 65535. */
int fmi_plane_sums_f32(const float* a, const float* b, int planes, int64_t n, double* out3, double* ws_part, int64_t ws_doubles, void* stream);

/* ------------------------------------------------------------------------
 * The pixel head of pSpLoss.__call__ (csrc/psploss.hip; modules/psp/criteria/__init__.py:58-65,80-87).  y_hat, y, ref: planar fp32
 * [N][3][H][W] as pSp.forward and the dataloader hand them over (ref may be NULL); mask [N][H][W] fp32 (may be NULL).  m = mask,
 * im = 1 - m (one rounded subtraction); with a NULL mask im = 1.  The inner pair (the `ref` side, :80-87) exists only when ref AND mask
 * are given; without them it is skipped, its sum is 0 and a non-NULL pair_in / g_pair_in is FMI_ERR_BAD_ARG.  N <= 65535.
 * y_hat_hwc = 1: y_hat (and d_y_hat) is [N][H][W][3] in memory -- the channels-last tensor pSp.forward's face_pool returns, read without
 * a transposition; 0: planar; anything else is FMI_ERR_BAD_ARG.  The arithmetic and the outputs do not depend on it.
 * All pointers 4-byte aligned (sums / ws_part 8), else FMI_ERR_BAD_ARG; when H * W % 4 == 0 and every tensor is 16-byte aligned a thread
 * takes four pixels with 16-byte loads and stores, otherwise one pixel.
 * ---------------------------------------------------------------------- */
/* forward, one pass; every output may be NULL (not wanted), at least one is given:
 *   pair_out [2N][H][W][3] NHWC: images 0 .. N-1 = y_hat im, N .. 2N-1 = y im -- the batch LPIPS.forward builds with
 *            cat(to_nhwc(x), to_nhwc(y)) from the operands of :59-60,64-65; every product one rounded fp32 multiply (bit exact);
 *   pair_in  [2N][H][W][3]: y_hat m, then ref m (:80-81);
 *   sums     fp64[2] = sum (y_hat im - y im)^2, sum (y_hat m - ref m)^2: the difference in fp32, squared and accumulated in fp64;
 *   out2     fp32[2] = sums / (3 N H W): the two F.mse_loss values of :59-60,86.
 * ws_part: fp64 scratch of ws_doubles >= N * 64 * 2 entries (needed when sums or out2 is wanted): per-workgroup partial rows, added in
 * a fixed order by a finishing launch -- no atomics, nothing to zero, bit-reproducible whether or not fmi_set_deterministic is on. */
int fmi_psp_pixel_head_fwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, float* pair_out, float* pair_in,
                               double* sums, float* out2, int N, int H, int W, int y_hat_hwc, double* ws_part, int64_t ws_doubles, void* stream);
/* backward with respect to y_hat, one pass and one launch that recomputes the products from the same four inputs (nothing per pixel is
 * saved).  g_pair_out, g_pair_in [2N][H][W][3] (either may be NULL = zero; only images 0 .. N-1 of each reach y_hat); g2: a DEVICE array
 * of two floats, the upstream gradients of out2 (no host read).  With count = 3 N H W:
 *   d_y_hat [N][3][H][W] = im (g_pair_out + g2[0] 2 (y_hat im - y im) / count) + m (g_pair_in + g2[1] 2 (y_hat m - ref m) / count)
 * with the differences evaluated as im (y_hat - y) and m (y_hat - ref): the same value, one rounding of the difference instead of one per
 * product, so every entry is within 8 * 2^-24 of the sum of the magnitudes of its four terms. */
int fmi_psp_pixel_head_bwd_f32(const float* y_hat, const float* y, const float* ref, const float* mask, const float* g_pair_out,
                               const float* g_pair_in, const float* g2, float* d_y_hat, int N, int H, int W, int y_hat_hwc, void* stream);

/* ------------------------------------------------------------------------
 * The image head of GANOptimizer.__call__ (csrc/ganhead.hip; modules/loss.py:48-51,84-95,115).  gen: fp32 [N][3][H][W], planar
 * (gen_hwc = 0) or [N][H][W][3] in memory (gen_hwc = 1: the channels-last tensor ReferenceFill.forward returns, read without a
 * transposition; d_gen has the same layout); anything else is FMI_ERR_BAD_ARG.  gt, src, ref planar [N][3][H][W]; mask [N][H][W] fp32;
 * mean, stdv: DEVICE arrays of three floats.  m = mask, im = 1 - m (one rounded subtraction); every product one rounded multiply,
 * taken BEFORE the resize as loss.py:87-95 does.  R: bilinear resize to [OH][OW] with align_corners=True -- the source-index arithmetic
 * and the expression of fmi_resize_bilinear_f32; (OH, OW) == (H, W) is the no-resize case of loss.py:48 (R is then the identity, bit
 * for bit).  norm(v) = (v - mean[c]) / stdv[c] (loss.py:50-51).  N <= 65535.  All pointers 4-byte aligned (ws_part 8), else
 * FMI_ERR_BAD_ARG; 16-byte accesses where the bases are 16-byte aligned and the row length is a multiple of four, one pixel otherwise.
 * ---------------------------------------------------------------------- */
/* forward, one pass and a finishing launch:
 *   x_in [3N][OH][OW][3] NHWC: images 0 .. N-1 = norm(R(gen)), N .. 2N-1 = norm(R(gen im)), 2N .. 3N-1 = norm(R(gen m));
 *   y_in [3N][OH][OW][3]:      norm(R(gt)), norm(R(src)), norm(R(ref m)) -- the operands VGGLoss.forward hands its first block for the
 *                              perceptual, style and contextual terms (loss.py:84-95), in that order;
 *   l1   fp32[1] = mean |gen - gt| over N 3 H W (loss.py:115): the difference in fp32, accumulated in fp64.
 * ws_part: fp64 scratch of ws_doubles >= N * 64 entries: one partial row per workgroup, added in a fixed order by the finishing launch
 * -- no atomics, nothing to zero, bit-reproducible whether or not fmi_set_deterministic is on. */
int fmi_gan_image_head_fwd_f32(const float* gen, const float* gt, const float* src, const float* ref, const float* mask, const float* mean,
                               const float* stdv, float* x_in, float* y_in, float* l1, int N, int H, int W, int OH, int OW, int gen_hwc,
                               double* ws_part, int64_t ws_doubles, void* stream);
/* backward with respect to gen, one launch that recomputes the products (nothing per pixel is saved).  gx [3N][OH][OW][3]: the gradient
 * of x_in (NULL = zero); g_l1: a DEVICE scalar, the gradient of l1 (NULL = zero; no host read).  With gk = images kN .. kN + N-1 of gx:
 *   d_gen = g_l1 sign(gen - gt) / (3 N H W) + Rt(g0 / stdv) + im Rt(g1 / stdv) + m Rt(g2 / stdv)
 * Rt, the adjoint of R, in gather form: every input pixel sums its contributing output pixels in a fixed order (the scheme of
 * fmi_resize_bilinear_bwd_f32 in reproducible mode), so d_gen is written, not accumulated: no atomics, no zero fill, the same bits in
 * either mode. */
int fmi_gan_image_head_bwd_f32(const float* gen, const float* gt, const float* mask, const float* stdv, const float* gx, const float* g_l1,
                               float* d_gen, int N, int H, int W, int OH, int OW, int gen_hwc, void* stream);

/* ------------------------------------------------------------------------
 * Contextual loss (external_function.py:231-274), x,y NHWC features [N,P,C].
 * ---------------------------------------------------------------------- */
int fmi_cx_channel_mean_f32(const float* y, float* mu /*[C] zeroed*/, int64_t rows, int C, void* stream);
/* out[p,:] = (x[p,:]-mu)/||x[p,:]-mu|| ; inv_norm[p] saved for backward */
int fmi_cx_normalise_f32(const float* x, const float* mu, float* out, float* inv_norm, int64_t rows, int C, void* stream);
int fmi_cx_normalise_bwd_f32(const float* g, const float* xn, const float* inv_norm, float* gx, int64_t rows, int C, void* stream);
/* from cos[N][P][P] (row i = x point, col j = y point): per-row d_min, w = exp((1 - d/(dmin+1e-5))/h), row sums;
 * cxij = w/rowsum; colmax[n][j] + argmax over i; cx[n] = mean_j colmax; loss += scale * -log(cx+1e-5)/N */
int fmi_cx_rows_f32(const float* cosm, float* cxij, float* dmin, int* argmin, float* rowsum, int N, int P, float h, void* stream);
int fmi_cx_cols_f32(const float* cxij, float* colmax, int* colarg, int N, int P, void* stream);
int fmi_cx_loss_f32(const float* colmax, float* cx /*[N]*/, float* loss /*[1] zeroed*/, int N, int P, float scale, void* stream);
/* backward: writes dcos[N][P][P] (overwrites) */
int fmi_cx_bwd_f32(const float* cxij, const float* dmin, const int* argmin, const float* rowsum, const float* cosm,
                   const int* colarg, const float* cx, const float* gscale, float* dcos, int N, int P, float h, float scale,
                   void* stream);

/* ------------------------------------------------------------------------
 * Multi-tensor Adam (torch.optim.Adam defaults as used at train_reference_fill.py:309-315).
 * ---------------------------------------------------------------------- */
typedef struct {
  float* p; const float* g; float* m; float* v; int64_t n;
} fmi_adam_entry;
int fmi_adam_step_f32(const fmi_adam_entry* entries /* HOST array */, int count, int64_t max_n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, void* stream);
/* the same Adam step with the step count in device memory: step_dev[0] is incremented first, the bias corrections are computed on
 * the device from it -- a training step captured in a HIP graph (torch.cuda.graph) replays with the right corrections */
int fmi_adam_step_dev_f32(const fmi_adam_entry* entries /* HOST array */, int count, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int* step_dev, void* stream);
/* the same with a device-side guard: when guard[0] (a device scalar, normally the loss of this step) is not finite the call changes
 * nothing -- parameters, moments and the step count keep their values: train_psp.py:328-331 ("skip the step if the loss is not finite")
 * without a host read, so it survives HIP-graph capture.  guard == NULL: fmi_adam_step_dev_f32. */
int fmi_adam_step_dev_guarded_f32(const fmi_adam_entry* entries /* HOST array */, int count, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, int* step_dev, const float* guard, void* stream);
/* multi-tensor Ranger step = RAdam + Lookahead + gradient centralisation (modules/psp/ranger.py:92-184, the --optimizer ranger of
 * train_psp.py:290-293).  row_mean (scratch, rows floats) non-NULL = centralise: g -= mean of its row (tensors with more than one
 * dimension, cols = numel / shape[0]); step_size / rectified from the host (the RAdam variance rectification depends on the step
 * count only); lookahead != 0 on every k-th step: slow += alpha (p - slow), p = slow */
typedef struct {
  float* p; const float* g; float* m; float* v; float* slow; float* row_mean; int64_t n; int64_t cols;
} fmi_ranger_entry;
int fmi_ranger_step_f32(const fmi_ranger_entry* entries /* HOST array */, int count, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float step_size, int rectified, float alpha, int lookahead, void* stream);

/* ------------------------------------------------------------------------
 * The reference's own native ops (modules/psp/stylegan2/op).
 * ---------------------------------------------------------------------- */
/* in [major,in_h,in_w] (minor = 1, as op/upfirdn2d.py:96 always reshapes), kernel [kh,kw], out [major,out_h,out_w];
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1.  Generic up/down/kernel sizes are supported. */
int fmi_upfirdn2d_f32(const float* in, const float* kernel, float* out, int major, int in_h, int in_w,
                      int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                      int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
/* bf16 storage (uint16_t bit patterns), fp32 arithmetic, round-to-nearest-even results: the reference's op is templated on the
 * tensor dtype (op/upfirdn2d_kernel.cu:149-170 AT_DISPATCH), taps included */
int fmi_upfirdn2d_bf16(const uint16_t* in, const uint16_t* kernel, uint16_t* out, int major, int in_h, int in_w, int kh, int kw,
                       int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
/* x [.., C, step_b...] contiguous NCHW as in the reference: bias index = (i / step_b) % size_b.
 * act: 1 linear, 3 leaky relu; grad: 0 forward, 1 first derivative w.r.t. x using ref = forward OUTPUT, 2 second (=0).
 * bias / ref may be NULL. */
int fmi_fused_bias_act_f32(const float* x, const float* bias, const float* ref, float* out, int64_t n,
                           int step_b, int size_b, int act, int grad, float alpha, float scale, void* stream);
int fmi_fused_bias_act_bf16(const uint16_t* x, const uint16_t* bias, const uint16_t* ref, uint16_t* out, int64_t n, int step_b,
                            int size_b, int act, int grad, float alpha, float scale, void* stream);
/* dbias[c] += sum_{n,hw} g[n][c][hw] for NCHW g (grad_bias of FusedLeakyReLU, op/fused_act.py:29-36); caller zeroes dbias */
int fmi_bias_grad_nchw_f32(const float* g, int N, int C, int64_t HW, float* dbias, void* stream);
/* the same sum for a bf16 cotangent (fused_leaky_relu on a bf16 tensor); dbias stays fp32 */
int fmi_bias_grad_nchw_bf16(const void* g, int N, int C, int64_t HW, float* dbias, void* stream);
/* NHWC variant used by the product's StyledConv: y = lrelu(x + bias[c] + nw[0]*noise[p]) * scale */
int fmi_noise_bias_act_f32(const float* x, const float* bias, const float* noise, const float* nw, float* y,
                           int64_t pixels, int C, float alpha, float scale, void* stream);

/* ------------------------------------------------------------------------
 * StyleGAN2 decoder on NHWC activations (stylegan2/model.py:187-369).  ModulatedConv2d is evaluated as
 * demod[n,o] * conv(x * s[n,c], W): algebraically the reference's per-sample weight modulation (model.py:244-250).
 * ---------------------------------------------------------------------- */
int fmi_scale_channels_f32(const float* x, const float* s, float* y, int N, int64_t P, int C, void* stream);       /* y[n,p,c] = x * s[n,c] */
/* gs[n,c] = sum_p g*x: written when a partials workspace ws (ws_floats >= N*C, contents irrelevant) is given, else += by atomics onto
 * a caller-zeroed gs */
int fmi_scale_channels_gs_f32(const float* g, const float* x, float* gs, float* ws, int64_t ws_floats, int N, int64_t P, int C, void* stream);
int fmi_sqsum_last_f32(const float* x, float* out, int64_t rows, int k, void* stream);                             /* out[r] = sum_k x[r,k]^2 */
int fmi_sqsum_last_bwd_f32(const float* x, const float* g, float* gx, int64_t rows, int k, void* stream);
/* backward of fmi_noise_bias_act_f32: gx = g*scale*(y>0?1:alpha); gnw[0] += sum gx*noise[p] (noise/gnw may be NULL) */
int fmi_noise_bias_act_bwd_f32(const float* g, const float* y, const float* noise, float* gx, float* gnw,
                               int64_t pixels, int C, float alpha, float scale, void* stream);
/* upfirdn2d with minor dimension = channels: in [N,in_h,in_w,C] -> out [N,out_h,out_w,C] */
int fmi_upfirdn2d_nhwc_f32(const float* in, const float* kernel, float* out, int N, int in_h, int in_w, int C,
                           int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                           int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* pSp encoder helpers (modules/psp/encoders/helpers.py:56-119), NHWC rows x C */
int fmi_prelu_f32(const float* x, const float* a, float* y, int64_t rows, int C, void* stream);                 /* nn.PReLU(C) */
/* ws (may be NULL): fp32 partials workspace of ws_floats >= C (contents irrelevant): ga is then WRITTEN; without it ga must be zeroed
 * and receives fp32 atomics */
int fmi_prelu_bwd_f32(const float* g, const float* x, const float* a, float* gx, float* ga, float* ws, int64_t ws_floats, int64_t rows,
                      int C, void* stream);
/* MaxPool2d(1, stride) = sub-sampling; backward != 0: x is the output gradient [N,OH,OW,C], y the (fully written) input gradient */
int fmi_subsample_f32(const float* x, float* y, int N, int H, int W, int C, int stride, int backward, void* stream);

/* ------------------------------------------------------------------------
 * bf16 body of the UNet mask detector (modules/unet/unet_parts.py), csrc/unet_bf16.hip.  NHWC bf16 tensors (raw bits), C % 8 == 0 and
 * 16-byte aligned pointers (FMI_ERR_UNSUPPORTED otherwise), fp32 arithmetic, round-to-nearest-even stores, no atomics.
 * ---------------------------------------------------------------------- */
/* 2 x 2 stride-2 max pooling, H and W even; the backward routes gy to the FIRST maximum of the window in row-major order */
int fmi_maxpool2_bf16(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, void* stream);
int fmi_maxpool2_bwd_bf16(const uint16_t* x, const uint16_t* gy, uint16_t* gx, int N, int H, int W, int C, void* stream);
/* Up (unet_parts.py:45-72) in one pass: y [N,H,W,C2+C1] = cat([skip [N,H,W,C2], pad(bilinear x2 align_corners=True of x1 [N,h,w,C1])], C);
 * the zero border is (H - 2h) / 2 rows on top and the rest below, the same split left and right; H >= 2h, W >= 2w.
 * Backward: gskip = the first C2 channels of g, gx1 = the adjoint of the interpolation as a gather (both fully written). */
int fmi_up2_cat_bf16(const uint16_t* x1, const uint16_t* skip, uint16_t* y, int N, int h, int w, int C1, int H, int W, int C2, void* stream);
int fmi_up2_cat_bwd_bf16(const uint16_t* g, uint16_t* gskip, uint16_t* gx1, int N, int h, int w, int C1, int H, int W, int C2, void* stream);
/* OutConv (1 x 1): y [P,K] fp32 = x [P,C] bf16 . w [K][C] fp32 + b [K]; K <= 4, C <= 1024.  The argmax form writes the float index of
 * the first maximum per pixel (fmi_argmax_channels_f32 of the same logits, which are never stored). */
int fmi_head1x1_bf16(const uint16_t* x, const float* w, const float* b, float* y, int64_t P, int C, int K, void* stream);
int fmi_head1x1_argmax_bf16(const uint16_t* x, const float* w, const float* b, float* mask, int64_t P, int C, int K, void* stream);
/* g [P,K] fp32 -> gx [P,C] bf16, gw [K][C] and gb [K] fp32 (written): one partial row per workgroup in ws (ws_doubles >= K*C + K; up to
 * 512 rows are used), added in a fixed order by a finishing launch */
int fmi_head1x1_bwd_bf16(const float* g, const uint16_t* x, const float* w, uint16_t* gx, float* gw, float* gb, double* ws,
                         int64_t ws_doubles, int64_t P, int C, int K, void* stream);

/* ------------------------------------------------------------------------
 * Inference form of the IR-SE bottleneck blocks of the pSp encoder on bf16 NHWC activations (modules/psp/encoders/helpers.py:56-119,
 * eval mode: the BatchNorm statistics are constants), csrc/irse_infer_bf16.hip and the per-column output stage of csrc/conv_bf16.hip.
 * fp32 parameters and arithmetic, one round-to-nearest-even per stored bf16 value, no atomics: every result is bit-reproducible.
 * An identity-shortcut SE block is conv1, conv2, gate, tail = 4 launches; a block with a convolution shortcut is 5.
 * ---------------------------------------------------------------------- */
#define FMI_CHAN_COLSUM_ROWS 64 /* rows of one partial block of fmi_conv2d_fwd_chan_bf16's column sums */
/* y = prelu(conv(x, W) * scale[k] + bias[k], slope[k]) in one launch; scale / bias / slope are fp32 [K], each may be NULL (1 / 0 / 1).
 * With slope: Conv2d + PReLU (helpers.py:87 / :109-110); with scale / bias: Conv2d + eval BatchNorm2d folded to scale = gamma /
 * sqrt(var + eps), bias = beta - mean * scale (helpers.py:88 / :111-112, and the shortcut :82-83 / :104-105).  wnk: bf16 [K][kh*kw][C]
 * (fmi_pack_weight_bf16).  3x3 pad 1 or 1x1 pad 0, stride 1 or 2, C % 64 == 0, K % 64 == 0, else FMI_ERR_UNSUPPORTED.
 * colsum (may be NULL; colsum_floats >= ceil(N*OH*OW / 64) * 2 * K, 16-byte aligned, contents irrelevant): the squeeze of the SE module
 * (helpers.py:67) from this output stage -- row [b][0][k] = the fp32 sum of v = acc * scale + bias (before the rounding) over those of rows
 * 64 b .. 64 b + 63 (rows = n*OH*OW + oy*OW + ox) that belong to the sample of row 64 b, row [b][1][k] over those of the next sample;
 * every row is written.  fmi_se_gate_f32 finishes them.  OH*OW < 128: FMI_ERR_UNSUPPORTED with colsum (use fmi_global_avgpool_bf16). */
int fmi_conv2d_fwd_chan_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* scale, const float* bias,
                             const float* slope, uint16_t* y, float* colsum, int64_t colsum_floats, void* stream);
/* SEModule's gate (helpers.py:67-71: avg_pool, fc1, relu, fc2, sigmoid) in one launch, one workgroup per sample:
 * gates[n][c] = sigmoid(fc2 . relu(fc1 . pooled[n])), fc1 fp32 [C/16][C], fc2 fp32 [C][C/16], C % 16 == 0, C <= 512.
 * rows_per_part > 0: part is the colsum workspace of fmi_conv2d_fwd_chan_bf16 ([blocks of rows_per_part rows][2][C], P rows per sample,
 * P >= rows_per_part); a sample's partial rows are added in a fixed order and pooled = sum * inv_count.
 * rows_per_part == 0: part is [N][C] and pooled = part * inv_count (1 for the means of fmi_global_avgpool_bf16). */
int fmi_se_gate_f32(const float* part, int rows_per_part, int64_t P, float inv_count, const float* fc1, const float* fc2, float* gates, int N,
                    int C, void* stream);
/* the block's tail (helpers.py:72 and :94 / :119, and the NEXT block's first BatchNorm :86 / :108) in one pass:
 * y = r * gate[n][c] + sc (gate NULL: y = r + sc, bottleneck_IR) and z = y * next_scale[c] + next_shift[c] from the fp32 y; y and z are
 * each rounded once to bf16; tap (may be NULL) receives the fp32 y.  z may be NULL (then next_scale / next_shift are not read).
 * r, y, z, tap are [N][OH][OW][C]; sc is [N][SH][SW][C] read at (oy * sc_stride, ox * sc_stride) -- the MaxPool2d(1, stride) shortcut
 * (helpers.py:79 / :101) without a pass of its own; OH == (SH - 1) / sc_stride + 1, sc_stride 1 or 2.  C % 8 == 0, 16-byte pointers. */
int fmi_irse_tail_bf16(const uint16_t* r, const float* gate, const uint16_t* sc, const float* next_scale, const float* next_shift, uint16_t* y,
                       uint16_t* z, float* tap, int N, int OH, int OW, int C, int SH, int SW, int sc_stride, void* stream);
/* hand-over from the fp32 stem (after its PReLU) to the bf16 body: y = bf16(x), z = bf16(x * scale[c] + shift[c]) -- block 0's first
 * BatchNorm (helpers.py:86 / :108) evaluated on the fp32 x.  C % 8 == 0. */
int fmi_irse_stem_bf16(const float* x, const float* scale, const float* shift, uint16_t* y, uint16_t* z, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------
 * Inference form of the PICNet encoders and the guided attention on bf16 NHWC activations (ResEncoder(compute_dtype=bf16),
 * ExampleGuidedAttention on bf16 maps), csrc/picnet_enc_bf16.hip and csrc/attention_bf16.hip.  Replaces base_function.py:242-305
 * (ResBlock with norm 'none', ResBlockEncoderOptimized) and example_guided_att.py:21-41 of the reference.  fp32 parameters and
 * accumulation, one round-to-nearest-even per stored bf16 value, no atomics: every result is bit-reproducible.  The layers with C and K
 * multiples of 64 run on fmi_conv2d_fwd_chan_bf16 (scale NULL, slope a [K] vector of 0.1 for conv1).  A ResBlock is conv1, bypass,
 * conv2, tail = 4 launches, the stem 3, the guided attention 2.  Every entry refuses bad arguments (FMI_ERR_BAD_ARG: NULL pointers,
 * non-positive extents, a descriptor whose OH / OW do not follow from it) and unsupported shapes or misaligned pointers
 * (FMI_ERR_UNSUPPORTED) before any HIP call.
 * ---------------------------------------------------------------------- */
/* the stem's conv1 (base_function.py:278, :283): y = lrelu(conv3x3(x) + bias, slope), zero padding 1, stride 1.  x fp32 [N,H,W,C <= 4],
 * wf fp32 [9][C][K] (the fp32 forward pack), bias fp32 [K] or NULL, y bf16 [N,H,W,K], K in {32, 64}; fp32 FMAs.  The LeakyReLU of
 * model[1] lives here because conv2 is the only consumer.  y 16-byte aligned. */
int fmi_conv2d_thin_in_fwd_bf16(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias, float slope, uint16_t* y,
                                void* stream);
/* the pSp encoder's stem (psp_encoders.py:59-61: Conv2d(3, 64, 3x3, pad 1, no bias), BatchNorm2d, PReLU) and block 0's first BatchNorm
 * (helpers.py:86 / :108) in one launch, eval mode:  v = conv3x3(x) in fp32 FMAs,  a = prelu(v * scale[k] + shift[k], slope[k]),
 * y = bf16(a),  z = bf16(a * scale0[k] + shift0[k]) -- both rounded once from the fp32 a, the rounding points of the fp32 convolution
 * followed by fmi_irse_stem_bf16.  x fp32 [N,H,W,C <= 4], wf fp32 [9][C][K] (the fp32 forward pack), the five vectors fp32 [K],
 * y / z bf16 [N,H,W,K]; a32 (debug, may be NULL) receives the fp32 a.  K % 8 == 0 and K <= 256, 3x3 pad 1 stride 1, x below 4 GiB,
 * y / z / a32 16-byte aligned, else FMI_ERR_UNSUPPORTED; a NULL operand or an inconsistent descriptor: FMI_ERR_BAD_ARG. */
int fmi_irse_stem_fwd_bf16(const fmi_conv_desc* d, const float* x, const float* wf, const float* scale, const float* shift, const float* slope,
                           const float* scale0, const float* shift0, uint16_t* y, uint16_t* z, float* a32, void* stream);
/* the 32-channel layers (base_function.py:254-256 at ngf 32, :279): y = lrelu(conv(x) + bias, slope); slope = 1 is the plain convolution.
 * x bf16 [N,H,W,32], wnk bf16 [K][kh*kw][32] (fmi_pack_weight_bf16), bias fp32 [K] or NULL, y bf16 [N,H,W,K].  C == 32, K in {32, 64},
 * 3x3 pad 1 or 1x1 pad 0, stride 1, dense pixel pitches; 16-byte aligned pointers.  bf16 MFMA, fp32 accumulation; the whole weight set
 * stays in registers for the launch and the map is read once. */
int fmi_conv2d_c32_fwd_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* bias, float slope, uint16_t* y,
                            void* stream);
/* the block tail (base_function.py:266-271): v = main + shortcut in fp32, with pool = 1 the 2x2 mean of that sum (pool(a) + pool(b) =
 * pool(a + b)).  main / shortcut bf16 [N,H,W,C]; outputs [N,H',W',C] with H' = H / 2 under pool: y_raw = bf16(v), y_act =
 * bf16(lrelu(v, slope)), y_f32 = v.  A NULL output is skipped; all three NULL: FMI_ERR_BAD_ARG.  C % 8 == 0, H and W even with pool. */
int fmi_resblock_tail_bf16(const uint16_t* main_, const uint16_t* shortcut, uint16_t* y_raw, uint16_t* y_act, float* y_f32, int N, int H, int W,
                           int C, int pool, float slope, void* stream);
/* the stem's tail (base_function.py:296-305): v = pool2(h) + bypass1x1(pool2(img)) + bias.  h bf16 [N,H,W,K] (conv2's output), img fp32
 * [N,H,W,C <= 4], wb fp32 [C][K], bias fp32 [K] or NULL; y_raw / y_act bf16 [N,H/2,W/2,K] as above (one may be NULL).  K % 8 == 0, H
 * and W even. */
int fmi_picnet_stem_tail_bf16(const uint16_t* h, const float* img, const float* wb, const float* bias, uint16_t* y_raw, uint16_t* y_act, int N,
                              int H, int W, int C, int K, float slope, void* stream);
/* ExampleGuidedAttention's two attentions and its blend in one launch (example_guided_att.py:21-41), A = softmax_j(q_i . q_j) evaluated
 * once:  out[..., :C] = (1 - m) (A ref) + m ref,  out[..., C:] = A src.  q [N,T,D], src / ref [N,T,C], out [N,T,2C] bf16; mask fp32 [N,T]
 * (the soft mask after the bilinear resize).  The blend is evaluated in fp32 before the one rounding; m == 1 returns ref bit for bit.
 * The kernel is fmi_attention_fwd_bf16's with a V tile [ref | src]; same lazy reference maximum.  Supported: T % 128 == 0, (D, C) =
 * (32, 128), N <= 65535; waves as there, 0 = fmi_guided_attention_fwd_bf16_waves(N, T) (8 if T % 256 == 0 and (T/256) N >= 256, else
 * 4).  NULL pointers or q / src / ref / out off 16-byte alignment: FMI_ERR_BAD_ARG. */
int fmi_guided_attention_fwd_bf16_waves(int N, int T);
int fmi_guided_attention_fwd_bf16(const uint16_t* q, const uint16_t* src, const uint16_t* ref, const float* mask, uint16_t* out, int N, int T,
                                  int D, int C, int waves, void* stream);
/* the same at the pSp encoder's shapes (example_guided_att.py:21-41 as psp_encoders.py:128-132 builds it): (D, C) in {(64, 256),
 * (128, 512)} = attention2 / attention1.  The kernel is the one above with grid index z a slice of 128 channels: its V tile is
 * [ref slice | src slice] read at row pitch C, it writes out[..., 128 z : +128] and out[..., C + 128 z : +128], and every slice recomputes
 * the scores from the shared q, so the accumulators of a wave do not grow with C.  Same arguments, checks, blend (m == 1 returns ref
 * bit for bit), lazy reference maximum and wave dispatch; any other (D, C), (32, 128) included: FMI_ERR_UNSUPPORTED. */
int fmi_guided_attention_sliced_fwd_bf16(const uint16_t* q, const uint16_t* src, const uint16_t* ref, const float* mask, uint16_t* out, int N,
                                         int T, int D, int C, int waves, void* stream);

/* ------------------------------------------------------------------------
 * Inference form of the map2style heads of the pSp encoder on bf16 NHWC activations: the G heads of one pyramid level run together, one
 * launch per layer (csrc/style_heads_bf16.hip and the grouped output stage of csrc/conv_bf16.hip).  Replaces, of the reference,
 * psp_encoders.py:13-37 (GradualStyleBlock: log2(spatial) x [Conv2d 3x3 stride 2 + LeakyReLU], EqualLinear), psp_encoders.py:97-98
 * (_upsample_add), psp_encoders.py:140-151 (the loops over the heads of a level, torch.stack) and stylegan2/model.py EqualLinear
 * (F.linear(x, weight * scale, bias * lr_mul)).  fp32 parameters and accumulation, one round-to-nearest-even per stored bf16 value, no
 * atomics: every result is bit-reproducible.  Every entry returns FMI_ERR_BAD_ARG / FMI_ERR_UNSUPPORTED before any HIP call.
 * ---------------------------------------------------------------------- */
#define FMI_STYLE_SKINNY_ROWS 128 /* fmi_conv2d_grouped_fwd_bf16: calls with at most this many output rows take the weight-streaming kernel */
/* G convolutions in one launch (psp_encoders.py:13-37 for all heads of a level, psp_encoders.py:140-151): group g reads channels
 * [g * x_group_off, g * x_group_off + C) of every pixel of x (x_group_off = 0: all groups read the same map, layer 1 of a level;
 * x_group_off = C: layers 2 and later) and writes columns [g*K, (g+1)*K) of every pixel of y; d->C / d->K are per group, d->x_cstride /
 * d->y_cstride the pixel pitches (x_cstride >= (G-1) * x_group_off + C, y_cstride >= G*K; columns outside [0, G*K) are never written).
 * wnk: bf16 [G][K][kh*kw][C]; bias: fp32 [G][K] or NULL.  y = v > 0 ? v : slope * v with v = acc + bias (slope = 1: no activation).
 * Exactly one of y16 (bf16) and y32 (fp32) is non-NULL, else FMI_ERR_BAD_ARG; so are NULL operands, G <= 0, x_group_off not in {0, C}
 * and a descriptor whose OH / OW do not follow.  Supported: 3x3 pad 1 stride 2 or 1x1 pad 0 stride 1; C % 64 == 0, K % 64 == 0; 16-byte
 * aligned operands; pitches that are multiples of 8; y32 for 1x1 only -- the EqualLinear of all heads of a level (stylegan2/model.py
 * EqualLinear, psp_encoders.py:36; wnk = bf16(weight * scale), bias = bias * lr_mul) written straight into its slots of the
 * [N, n_styles, K] latent tensor: y32 = latents + first*K, y_cstride = n_styles*K.  Everything else: FMI_ERR_UNSUPPORTED.
 * rows = N*OH*OW > FMI_STYLE_SKINNY_ROWS with y16: the 128-byte-row tile kernel of csrc/conv_bf16.hip, one grid row per group.
 * rows <= FMI_STYLE_SKINNY_ROWS, and every y32 call: a kernel that streams each group's weights once -- grid (K/16, G, ceil(rows/64)),
 * four waves that split the reduction and meet through LDS in a fixed order. */
int fmi_conv2d_grouped_fwd_bf16(const fmi_conv_desc* d, int G, int64_t x_group_off, const uint16_t* x, const uint16_t* wnk,
                                const float* bias, float slope, uint16_t* y16, float* y32, void* stream);
/* _upsample_add (psp_encoders.py:97-98) and the hand-over to the heads in one pass: p = bilinear(coarse, align_corners=True, to H x W) +
 * lateral, written as fp32 p32 (may be NULL) and bf16 p16.  coarse NULL: the plain conversion p = lateral (the coarsest map).  lateral,
 * p32, p16 are [N,H,W,C], coarse is [N,CH,CW,C]; C % 8 == 0, 16-byte aligned pointers (else FMI_ERR_UNSUPPORTED).  NULL lateral / p16
 * or a non-positive extent: FMI_ERR_BAD_ARG. */
int fmi_fpn_merge_bf16(const float* lateral, const float* coarse, float* p32, uint16_t* p16, int N, int H, int W, int CH, int CW, int C,
                       void* stream);
/* _upsample_add (psp_encoders.py:97-98) from bf16 maps: p16 = bf16(bilinear(coarse, align_corners=True, to H x W) + lateral) with the same
 * integer bilinear weights and fp32 arithmetic as fmi_fpn_merge_bf16, one rounding.  lateral, p16 bf16 [N,H,W,C], coarse bf16
 * [N,CH,CW,C]; C % 8 == 0, 16-byte aligned pointers (else FMI_ERR_UNSUPPORTED).  A NULL pointer or a non-positive extent: FMI_ERR_BAD_ARG. */
int fmi_fpn_merge_in_bf16(const uint16_t* lateral, const uint16_t* coarse, uint16_t* p16, int N, int H, int W, int CH, int CW, int C,
                          void* stream);
/* the mask blend of the pyramid levels (psp_encoders.py:135-138) in one launch: y = bf16(m r + (1 - m) c), evaluated in fp32, from bf16
 * r, c [rows][C] and fp32 m [rows].  m == 1 returns r and m == 0 returns c bit for bit.  C % 8 == 0, r / c / y 16-byte aligned (else
 * FMI_ERR_UNSUPPORTED); a NULL pointer or a non-positive extent: FMI_ERR_BAD_ARG. */
int fmi_mask_blend_bf16(const uint16_t* r, const uint16_t* c, const float* m, uint16_t* y, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------
 * bf16 VGG16 trunk of VGGLoss for training (VGGLoss(feature_dtype=torch.bfloat16) / FMI_VGG_DTYPE=bf16): the frozen convolutions between
 * the image and the four feature maps the losses read, forward and input-gradient chain.  Replaces modules/loss.py:16-65 of the reference
 * (the four blocks of vgg16.features[:23] and the loop that taps them); the loss terms themselves stay the fp32 kernels.  The forward
 * convolutions are fmi_conv2d_thin_in_fwd_bf16 (conv1_1) and fmi_conv2d_fwd_act_bf16 (bias + ReLU in the output stage).  fp32 parameters
 * and accumulation, one round-to-nearest-even per stored bf16 value, no split reductions and no atomics: every result is bit-reproducible
 * in either mode of fmi_set_deterministic.  Every entry refuses bad arguments (FMI_ERR_BAD_ARG: NULL pointers, non-positive extents, a
 * descriptor whose OH / OW do not follow from it) and unsupported shapes or misaligned pointers (FMI_ERR_UNSUPPORTED) before any HIP call.
 * ---------------------------------------------------------------------- */
/* the adjoint of a convolution whose input is another convolution's ReLU output (loss.py:33-52: conv1_2, 2_2, 3_2, 3_3, 4_2, 4_3):
 * dx = bf16(a_in > 0 ? adjoint(dy) : 0) -- fmi_conv2d_dgrad_bf16 with that ReLU's mask in the output stage.  dy bf16 [N,OH,OW,K], wck bf16
 * [C][9][K] (fmi_pack_weight_bf16), a_in and dx bf16 [N,H,W,x_cstride].  3x3 pad 1 stride 1, C % 64 == 0, K % 64 == 0, x_cstride % 4 == 0,
 * y_cstride % 8 == 0, 16-byte aligned pointers.  The tile is the one fmi_conv2d_dgrad_bf16 takes for the shape (fmi_debug_bf16_tile
 * applies), never the split reduction; with a_in > 0 everywhere the result is that entry's, bit for bit. */
int fmi_conv2d_dgrad_relu_bf16(const fmi_conv_desc* d, const uint16_t* dy, const uint16_t* wck, const uint16_t* a_in, uint16_t* dx, void* stream);
/* the point where the losses tap a block's activated map a bf16 [N,H,W,C] (loss.py:54-65), one pass over a: tap fp32 [N,H,W,C] = float(a)
 * (exact) and, pooled not NULL, pooled bf16 [N,H/2,W/2,C] = the 2x2 max pool that opens the next block, with fmi_maxpool2_bf16's winner
 * rule (first maximum in row-major order, a NaN wins).  C % 8 == 0, 16-byte aligned pointers, H and W even with pooled. */
int fmi_vgg_tap_fwd_bf16(const uint16_t* a, float* tap, uint16_t* pooled, int N, int H, int W, int C, void* stream);
/* its backward with the block's last ReLU: dy = bf16(a > 0 ? gtap + unpool(gpool) : 0), the sum in fp32 and one rounding; gtap fp32
 * [N,H,W,C], gpool bf16 [N,H/2,W/2,C] or NULL (block 4), routed to each window's winner by the forward's rule.  Same conditions. */
int fmi_vgg_tap_bwd_bf16(const uint16_t* a, const float* gtap, const uint16_t* gpool, uint16_t* dy, int N, int H, int W, int C, void* stream);
/* fmi_conv2d_thin_input_dgrad_f32 reading a bf16 gradient (conv1_1's adjoint, loss.py:33-52 towards the generated image): dy16 bf16
 * [N,H,W,K], wt fp32 [taps][K][C], dx fp32 [N,H,W,C <= 4]; fp32 FMAs.  The class fmi_conv2d_thin_in_supported accepts with K/4 a power of
 * two, at any map size (the streaming kernel of csrc/thinin.hip); dy16 16-byte aligned. */
int fmi_conv2d_thin_input_dgrad_bf16(const fmi_conv_desc* d, const uint16_t* dy16, const float* wt, float* dx, void* stream);

/* ------------------------------------------------------------------------
 * The tap passes of the fp32 VGG16 trunk (csrc/vgg_f32.hip; loss.py:54-65): the activated map a fp32 [N,H,W,C] of a block's last
 * convolution is the tap itself.  No atomics, the same code in both modes of fmi_set_deterministic.  C % 4 == 0, pieces C % 16 == 0,
 * 16-byte aligned pointers, else FMI_ERR_UNSUPPORTED (the caller keeps the composed kernels).
 * ---------------------------------------------------------------------- */
/* forward, one pass over a: pooled [N,H/2,W/2,C] = the 2x2 floor-mode max pool that opens the next block (fmi_maxpool2_f32's values) and,
 * pooled3 not NULL, pooled's bf16 piece image, bit for bit what fmi_split3_f32 makes of pooled */
int fmi_vgg_tap_fwd_f32(const float* a, float* pooled, void* pooled3, int N, int H, int W, int C, void* stream);
/* backward, one pass: dy = a > 0 ? (gtap + unpool(gpool)) : 0.  gtap arrives as nslice (1..4) batch slices gslice[s] of rows_per_slice =
 * N / nslice images each; a NULL slice is zeros and is neither filled nor read.  gpool [N,H/2,W/2,C] or NULL (last block: no add) goes
 * to the FIRST maximum of its window in row-major order (strict >, fmi_maxpool2_bwd_f32's rule); rows and columns beyond 2 (H/2), 2 (W/2)
 * receive nothing.  dy (fp32) and dy3 (dy's piece image, fmi_split3_f32's bits) are each optional -- a NULL one is not written -- and one
 * of them is required.  Bit-equal to zeros / cat, add, fmi_maxpool2_bwd_f32, FMI_EW_RELU_BWD_OUT (and fmi_split3_f32) on these operands. */
int fmi_vgg_tap_bwd_f32(const float* a, const float* const* gslice, int nslice, int rows_per_slice, const float* gpool, float* dy, void* dy3,
                        int N, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FMI_HIP_H */
