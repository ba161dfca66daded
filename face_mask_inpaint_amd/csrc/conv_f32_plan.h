// Which kernel an fp32 convolution runs on, as pure host functions: route, tile, split of the reduction, blocked accumulation, the
// initialising launch and the grid of every launch of the fp32 family -- the generic GEMM kernels (gemm_core.h; the dense GEMM of gemm.hip
// too), the tap-reuse 3x3 kernels (conv3x3.h), the piece-image kernels (conv_p3.h), the one-launch ConvTranspose (convt3x3.h) and the
// weight gradients.  conv.hip fills the inputs; the launchers launch what comes back and decide nothing; fmi_conv2d_f32_plan returns the
// same answer without a launch.  Plain C++ (no HIP types, no build switches): tests/test_host_conv_f32_plan.py holds every threshold below
// against tests/golden/conv_f32_plan.npz on a g++ build.  Reproducible mode (`det`) and the FMI_DMA_OFF bits (`dma_off`) are inputs.
// Every threshold is a routing decision that a measurement justified; the measured rates stay next to the numbers.
//
// Not here: functional.p3_wanted (Python) decides whether a split pass that WRITES piece images is worth running at all -- the tests
// monkeypatch its module constants; this header only decides what to do with the piece images a call brings.  The insides of the thin
// kernels' files (thinconv.hip, thinin.hip) keep their own acceptance tests: their predicates' answers are inputs (thin_out, thin_in).
#pragma once
#include <stdint.h>

#include "../../include/fmi_hip.h"

// routes: the `route` of a launch plan and of fmi_debug_f32_last_plan
enum ConvRouteF {
  ROUTE_NONE_F = 0,
  ROUTE_GEMM_F = 1,          // gemm_dma_f32_kernel / gemm_mfma_f32_kernel<ConvK, ConvWX>
  ROUTE_GEMM_W3_F = 2,       // ... <ConvK, ConvWX3>: the weights as bf16 piece images
  ROUTE_GEMM_P3_F = 3,       // gemm_p3_kernel: both operands as piece images
  ROUTE_C3_F = 4,            // conv3x3_dma_kernel<TILE, false>
  ROUTE_C3_W3_F = 5,         // conv3x3_dma_kernel<Tile128x64w, true>
  ROUTE_C3_P3_F = 6,         // conv3x3_p3_kernel
  ROUTE_CONVT3X3_F = 7,      // convt3x3s2_dma_kernel: all four sub-pixel phases in one launch
  ROUTE_WGRAD_GEMM_F = 8,    // gemm kernels <WgradAX, DenseX, WgradEp>
  ROUTE_WGRAD_P3_F = 9,      // wgrad_p3_kernel
  ROUTE_WGRAD_P3_3X3_F = 10, // wgrad3x3_p3_kernel
  ROUTE_THIN_OUT_F = 11,     // early exit to thinconv.hip (no launch plan: the kernels there choose their own grids)
  ROUTE_THIN_IN_F = 12,      // early exit to thinin.hip
  ROUTE_DENSE_F = 13         // launch_gemm for a caller that names no route (gemm.hip, the pair's weight gradient): not recorded
};

// tile id: 1000 rows + columns of the workgroup's output tile (wgrad3x3_p3_kernel: 192 rows = 3 taps x 64 channels)
constexpr int tile_id_f(int bm, int bn) { return 1000 * bm + bn; }
constexpr int tile_bm_f(int id) { return id / 1000; }
constexpr int tile_bn_f(int id) { return id % 1000; }
// the code of fmi_debug_f32_last_plan: route, LDS-DMA kernel or register kernel, blocked accumulation, tile
constexpr int plan_code_f(int route, bool dma, bool fl, int tile) { return (route << 24) | ((dma ? 1 : 0) << 23) | ((fl ? 1 : 0) << 22) | tile; }

struct LaunchPlanF {
  int status;        // FMI_OK, or what the launcher returns without launching
  int route, tile;
  bool dma;          // GEMM routes: the LDS-DMA kernel (else the register-staged one)
  bool fl;           // blocked accumulation of a long unsplit reduction (the FL instantiation)
  bool init;         // conv_split_init_kernel runs before this launch
  int asked;         // the split the caller asked for
  int ksplit, chunk; // normalised: splits, and reduction elements (GEMM: kchunk; weight gradients: pixels) or steps (3x3: it_chunk) per split
  int xcd_splits;    // piece-image weight gradients: the splits are dealt to the 8 XCDs in groups of 8
  int tiles, tiles_n;  // output tiles (weight gradients), column tiles
  unsigned grid[2];
  int code() const { return plan_code_f(route, dma, fl, tile); }
};
static inline LaunchPlanF refused_f(int status) {
  LaunchPlanF pl{};
  pl.status = status;
  return pl;
}
static inline int64_t plan_ceil_div_f(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------------
// Split of the (tap, channel) reduction of a forward / adjoint phase
// ---------------------------------------------------------------------------------------------
// Small feature maps with deep reductions (the 128-channel residual stacks at 32x32 and below, and the discriminator) give
// the implicit GEMM only a handful of output tiles: split the (tap, channel) reduction over several workgroups per tile.
static inline int conv_ksplit_f(int64_t M, int N, int K, bool det) {
  // keep the 128-wide tiles (operand reuse) and fill the chip by splitting the reduction instead of shrinking the tile
  const int64_t tiles = plan_ceil_div_f(M, 128) * plan_ceil_div_f(N, N <= 32 ? 32 : (N <= 64 ? 64 : 128));
  if (K < 512 || det) return 1;  // reproducible mode: no split reduction (partial sums would meet through atomics)
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
  int64_t ks = plan_ceil_div_f(384, tiles);
  // at least 16 k-tiles per split; a handful of output tiles (M <= 128 rows: the pSp style heads at 4^2 .. 1^2) only stream the
  // weights, so more, shorter splits put more loads in flight: 4 k-tiles there
  const int64_t kmin = (M <= 128 && tiles <= 16) ? 64 : 256;
  if (ks > K / kmin) ks = K / kmin;
  return ks < 2 ? 1 : (int)(ks > (kmin == 64 ? 64 : 16) ? (kmin == 64 ? 64 : 16) : ks);
}

// ---------------------------------------------------------------------------------------------
// The generic GEMM launchers: launch_gemm (gemm_core.h) and launch_gemm_p3 (conv_p3.h)
// ---------------------------------------------------------------------------------------------
// Tile for an M x N output with z workgroups per output tile (batch x reduction splits): the largest tile that still gives ~1.5
// workgroups per CU; small problems trade operand reuse for occupancy.  rows32: the launcher has the 32 x 128 tile and the rules that
// lead to it (launch_gemm, launch_gemm_p3); the tap-reuse launcher (launch_conv3x3) has no such tile and takes 64 x 128 for every wide
// output below the 128 x 128 threshold.  That is the one difference between the two tables.
static inline int gemm_tile_f(int M, int N, int64_t z, bool rows32) {
  auto wgs = [&](int bm, int bn) { return plan_ceil_div_f(M, bm) * plan_ceil_div_f(N, bn) * z; };
  const int64_t want = 384, want128 = 800;  // 128x128 only from ~one full round of workgroups (3 per CU) up: below that the
                                           // fullest CUs set the time and the 64x128 tile balances better (measured: -0.7 ms per step)
  if (N <= 32) return tile_id_f(128, 32);
  if (N <= 64) return (M > 64 && wgs(128, 64) >= want) ? tile_id_f(128, 64) : tile_id_f(64, 64);
  // between one and two rounds of 128x128 workgroups (3 per CU) the fullest CUs set the time: halve the work unit instead
  // (VGG 28^2: 588 tiles = 2.3 per CU, 94 -> 100 TFLOP/s with 64x128; at 1176 tiles the 128x128 tile wins again, 114 vs 102)
  if (M > 64 && wgs(128, 128) >= want128) return tile_id_f(128, 128);
  if (!rows32) return tile_id_f(64, 128);
  if (M > 32 && wgs(64, 128) >= want) return tile_id_f(64, 128);
  if (M > 64 && wgs(32, 128) < 256) return tile_id_f(64, 128);
  return tile_id_f(32, 128);
}

// FMI_DMA_OFF (debug): bit 0 dense GEMM, bit 1 conv forward / adjoint, bit 2 weight gradient -> use the register-staged kernel
enum { DMA_FAMILY_DENSE_F = 1, DMA_FAMILY_CONV_F = 2, DMA_FAMILY_WGRAD_F = 4 };

// dma_ok: both loaders can stage through LDS-DMA.  k0_ok: an empty reduction is launched (the epilogue still writes bias / residual);
// launch_gemm_p3 refuses it.
static inline LaunchPlanF gemm_plan_f(int route, int M, int N, int K, int batch, int ksplit, bool dma_ok, int family, int dma_off, bool det,
                                      bool k0_ok = true) {
  if (M <= 0 || N <= 0 || K < 0 || (K == 0 && !k0_ok) || batch <= 0 || ksplit <= 0) return refused_f(FMI_ERR_BAD_ARG);
  LaunchPlanF pl{};
  pl.route = route;
  pl.asked = ksplit;
  int kchunk = 16;
  if (K == 0) {
    ksplit = 1;  // empty reduction: the epilogue still writes bias / residual
  } else {
    kchunk = (int)plan_ceil_div_f(plan_ceil_div_f(K, ksplit), 16) * 16;
    ksplit = (int)plan_ceil_div_f(K, kchunk);
  }
  const int64_t gy = (int64_t)batch * ksplit;
  if (gy > 65535) return refused_f(FMI_ERR_UNSUPPORTED);
  pl.dma = !(dma_off & family) && dma_ok;
  // blocked accumulation (a second accumulator set: ~64 registers, an occupancy step for the 128 x 128 tile) where one workgroup adds more
  // than ~600 products in a row AND the run asks for it: the reproducible mode, where no split reduction blocks the sum for us.  The
  // register-staged GEMM kernel has no such form; gemm_p3_kernel has.
  pl.fl = kchunk > 640 && det && (pl.dma || route == ROUTE_GEMM_P3_F);
  pl.tile = gemm_tile_f(M, N, gy, true);
  const int64_t tm = plan_ceil_div_f(M, tile_bm_f(pl.tile)), tn = plan_ceil_div_f(N, tile_bn_f(pl.tile));
  if (tm * tn > 0x7fffffffLL) return refused_f(FMI_ERR_UNSUPPORTED);
  pl.ksplit = ksplit;
  pl.chunk = kchunk;
  pl.tiles_n = (int)tn;
  pl.grid[0] = (unsigned)(tm * tn);
  pl.grid[1] = (unsigned)gy;
  return pl;
}

// ---------------------------------------------------------------------------------------------
// The tap-reuse 3x3 launchers: launch_conv3x3 (conv3x3.h) and launch_conv3x3_p3 (conv_p3.h)
// ---------------------------------------------------------------------------------------------
// whole (ky, 16 channels) steps per split: nit steps in ksplit splits of it_chunk steps
static inline void c3_split_f(LaunchPlanF& pl, int nit, int ksplit) {
  pl.asked = ksplit;
  if (ksplit > nit) ksplit = nit;
  pl.chunk = (nit + ksplit - 1) / ksplit;
  pl.ksplit = (nit + pl.chunk - 1) / pl.chunk;
}
static inline void c3_grid_f(LaunchPlanF& pl, int M, int N) {
  const int64_t tm = plan_ceil_div_f(M, tile_bm_f(pl.tile)), tn = plan_ceil_div_f(N, tile_bn_f(pl.tile));
  pl.tiles_n = (int)tn;
  pl.grid[0] = (unsigned)(tm * tn);
  pl.grid[1] = (unsigned)pl.ksplit;
}
// have_w3: the piece image of the weights (of both packs, for the pair) is there
static inline LaunchPlanF c3_plan_f(int M, int N, int nit, int ksplit, bool have_w3, bool det) {
  LaunchPlanF pl{};
  c3_split_f(pl, nit, ksplit);
  auto wgs = [&](int bm, int bn) { return plan_ceil_div_f(M, bm) * plan_ceil_div_f(N, bn) * pl.ksplit; };
  pl.fl = pl.chunk > 13 && det;  // blocked accumulation of a long unsplit reduction (conv_p3.h)
  // piece images of the weights: 2 x 27 KB of LDS at 64 columns (two workgroups per CU; a 128-column piece tile would leave one).  Measured
  // at 8 x 128^2 256 -> 256 / 24 x 224^2 64 -> 64 / 8 x 32^2 128 -> 128: 163 / 154 / 81 TFLOP/s against 170 / 144 / 75 with both operands split in the
  // consuming waves (128 x 128 tiles): taken for narrow outputs and for launches too small to fill the chip with the large tile
  if (have_w3 && N > 32 && (N <= 64 || wgs(128, 128) < 800)) {
    pl.route = ROUTE_C3_W3_F;
    pl.tile = tile_id_f(128, 64);  // Tile128x64w
  } else {
    pl.route = ROUTE_C3_F;
    pl.tile = gemm_tile_f(M, N, pl.ksplit, false);
  }
  c3_grid_f(pl, M, N);
  return pl;
}
static inline LaunchPlanF c3p3_plan_f(int M, int N, int nit, int ksplit, bool det) {
  LaunchPlanF pl{};
  pl.route = ROUTE_C3_P3_F;
  c3_split_f(pl, nit, ksplit);
  auto wgs = [&](int bm, int bn) { return plan_ceil_div_f(M, bm) * plan_ceil_div_f(N, bn) * pl.ksplit; };
  // blocked accumulation: the eight-wave tiles hold one workgroup per CU (LDS) at 150 of 256 registers -- the second accumulator set is
  // free there, so every long reduction takes it; the four-wave tiles only in the reproducible mode (occupancy)
  const bool long_red = pl.chunk > 13;
  bool eight;
  if (N > 64) pl.tile = (eight = wgs(256, 128) >= 256) ? tile_id_f(256, 128) : tile_id_f(128, 128);
  else pl.tile = (eight = wgs(256, 64) >= 256) ? tile_id_f(256, 64) : tile_id_f(128, 64);
  pl.fl = long_red && (eight || det);
  c3_grid_f(pl, M, N);
  return pl;
}

// ---------------------------------------------------------------------------------------------
// Eligibility of the special kernels.  *_al16 / presence facts come from the call's pointers.
// ---------------------------------------------------------------------------------------------
// d->w3, the bf16 piece image of the weights, where the kernels can read it: shared weights, 16-channel groups of the reduction
static inline bool weight_pieces_f(bool w3_present_al16, int batch_w, int red_c) { return w3_present_al16 && batch_w == 1 && red_c % 16 == 0; }
// geometry the tap-reuse kernel takes (the caller falls back to the generic path otherwise).  C >= 64 or a narrow output: with 32
// reduction channels a tile has only 6 k-steps and, for 64 outputs, the heavier prologue loses (52 -> 42 TFLOP/s at 8 x 128^2, 32 -> 64)
// while 32 -> 32 still gains (71 -> 81)
static inline bool conv3x3_eligible_f(bool x_al16, bool w_al16, int C, int cs, int Nout, int64_t pixels) {
  return (C & 15) == 0 && (C >= 64 || Nout <= 32) && (cs & 3) == 0 && (Nout & 3) == 0 && x_al16 && w_al16 && pixels < (1ll << 30);
}
// x3 / w3: present and 16-byte aligned
static inline bool p3_generic_ok_f(bool x3, bool w3, int C, int pad_mode, int Nout, int64_t pixels) {
  return x3 && w3 && (C & 15) == 0 && !pad_mode && (Nout & 3) == 0 && pixels * 3 * C < (1ll << 40);
}
static inline bool conv3x3_p3_eligible_f(bool x3, bool w3, int C, int Nout, int64_t pixels) {
  return x3 && w3 && (C & 15) == 0 && (Nout & 3) == 0 && pixels < (1ll << 30);
}
// d: the descriptor of the convolution whose adjoint this is (fmi_conv2d_dgrad_f32): d->H x d->W = the ConvTranspose's OUTPUT
static inline bool convt3x3_eligible_f(const fmi_conv_desc* d, bool dy_al16, bool w3) {
  return w3 && d->kh == 3 && d->kw == 3 && d->stride == 2 && d->pad == 1 && d->dil <= 1 && d->H == 2 * d->OH && d->W == 2 * d->OW &&
         (d->K & 15) == 0 && d->C <= 64 && (d->C & 3) == 0 && (d->y_cstride & 3) == 0 && dy_al16 &&
         (int64_t)d->N * d->OH * d->OW >= 32768 && (int64_t)d->N * d->OH * d->OW < (1ll << 30);
}
static inline LaunchPlanF convt3x3_plan_f(int M, int Nout) {
  LaunchPlanF pl{};
  const int64_t tm = plan_ceil_div_f(M, 128), tn = plan_ceil_div_f(Nout, 32);
  if (tm * tn > 0x7fffffffLL) return refused_f(FMI_ERR_UNSUPPORTED);
  pl.route = ROUTE_CONVT3X3_F;
  pl.tile = tile_id_f(128, 32);
  pl.asked = pl.ksplit = 1;
  pl.tiles_n = (int)tn;
  pl.grid[0] = (unsigned)(tm * tn);
  pl.grid[1] = 1;
  return pl;
}
// x3 / dy3: present and 16-byte aligned
static inline bool wgrad_p3_ok_f(const fmi_conv_desc* d, bool x3, bool dy3) {
  return x3 && dy3 && d->C % 32 == 0 && d->K % 16 == 0 && d->x_cstride == d->C && d->y_cstride == d->K && d->pad_mode == 0 &&
         (int64_t)d->N * d->H * d->W * 3 * d->C < (1ll << 40) && (int64_t)d->N * d->OH * d->OW < 0x7fffffffLL;
}
// C % 64: with one 32-channel group per tile (GA = 1) the three taps share too little -- measured 47 against 72 TFLOP/s of the kernel above
static inline bool wgrad3x3_p3_ok_f(const fmi_conv_desc* d) {
  return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->dil <= 1 && d->W >= 16 && d->OH == d->H && d->OW == d->W && d->C % 64 == 0;
}

// ---------------------------------------------------------------------------------------------
// One forward or adjoint phase
// ---------------------------------------------------------------------------------------------
struct ConvPhaseInF {
  int M, Nout, Kdim, C, cstride;  // rows, output channels, reduction = taps x C, gathered channels and their pitch
  int64_t pixels;                 // of the gathered image
  int pad_mode;
  bool tap3;            // 3x3, stride 1, pad 1, no dilation, zero padding: the tap-reuse kernels' geometry
  int batch_w;
  bool x3, w3;          // piece images of the gathered tensor / of the weights (weight_pieces_f): present and 16-byte aligned
  bool x_al16, w_al16;  // the fp32 operands, for the tap-reuse kernel
  bool la_dma, lb_dma;  // dma_ok() of ConvK and of ConvWX (ConvWX3's follows from w3 and C)
  bool may_split;       // the reduction may be split over workgroups, whose partial sums meet through atomics in an output initialised first
  bool shared_init;     // the caller has initialised the output once for all phases (the adjoint's strided split): this phase only adds
  bool det;
  int dma_off;
};
static inline LaunchPlanF conv_phase_plan_f(const ConvPhaseInF& in) {
  const int ks = in.may_split ? conv_ksplit_f(in.M, in.Nout, in.Kdim, in.det) : 1;
  const int nit = 3 * (in.C >> 4);
  LaunchPlanF pl;
  // both operands as bf16 piece images (conv_p3.h): the activation pieces of x came from x's producer
  const bool p3 = in.batch_w == 1 && in.cstride == in.C && in.Kdim > 0 && p3_generic_ok_f(in.x3, in.w3, in.C, in.pad_mode, in.Nout, in.pixels);
  if (p3 && in.tap3 && conv3x3_p3_eligible_f(in.x3, in.w3, in.C, in.Nout, in.pixels))
    pl = c3p3_plan_f(in.M, in.Nout, nit, ks, in.det);
  else if (p3)
    pl = gemm_plan_f(ROUTE_GEMM_P3_F, in.M, in.Nout, in.Kdim, 1, ks, false, DMA_FAMILY_CONV_F, in.dma_off, in.det, false);
  else if (in.batch_w == 1 && in.tap3 && conv3x3_eligible_f(in.x_al16, in.w_al16, in.C, in.cstride, in.Nout, in.pixels))
    pl = c3_plan_f(in.M, in.Nout, nit, ks, in.w3, in.det);
  else if (in.w3 && in.la_dma)
    pl = gemm_plan_f(ROUTE_GEMM_W3_F, in.M, in.Nout, in.Kdim, 1, ks, in.la_dma && (in.C & 15) == 0, DMA_FAMILY_CONV_F, in.dma_off, in.det);
  else
    pl = gemm_plan_f(ROUTE_GEMM_F, in.M, in.Nout, in.Kdim, in.batch_w, ks, in.la_dma && in.lb_dma, DMA_FAMILY_CONV_F, in.dma_off, in.det);
  // the initialising launch follows the ASKED split, before a launcher normalises (or refuses) it
  pl.asked = ks;
  pl.init = !in.shared_init && ks > 1;
  return pl;
}
// the phase's output stage adds to an initialised output (no bias, residual or activation of its own)
static inline bool phase_adds_f(const ConvPhaseInF& in, const LaunchPlanF& pl) { return in.shared_init || pl.asked > 1; }

// ---------------------------------------------------------------------------------------------
// The entries' early exits.  thin_out / thin_in: the answers of fmi_conv2d_thin_supported and fmi_conv2d_thin_in_routed (forward), or of
// the thin-input adjoint's own acceptance test (fmi_conv2d_thin_input_dgrad_f32 returns FMI_ERR_UNSUPPORTED for what it leaves).
// ---------------------------------------------------------------------------------------------
struct ConvCallF {
  bool x_al16, w_al16, out_al16, res_al16;  // gathered tensor; second operand (weights, the weight gradient's dy); output; residual
  bool x3, x3_al16, w3, w3_al16, y3, y3_al16;
  bool bias, res, mask;
  int act, batch_w;
  bool det;
  int dma_off;
  bool thin_out, thin_in;
};
static inline int fwd_early_f(const fmi_conv_desc* d, const ConvCallF& c) {
  if (c.batch_w == 1 && c.thin_out && c.x_al16) return ROUTE_THIN_OUT_F;
  // thin INPUT (C <= 4: the image-facing first layers), 3x3 on a large map: streaming FMA kernel (thinin.hip).  The 1x1 form is a 9 - 13 us
  // launch either way and did not clear the keep-only-if-faster rule (profiles/thin_in.txt): it stays on the generic path
  if (c.batch_w == 1 && d->kh == 3 && c.thin_in && c.out_al16 && c.res_al16) return ROUTE_THIN_IN_F;
  return ROUTE_NONE_F;
}
static inline bool dgrad_bare_f(const ConvCallF& c) { return c.batch_w == 1 && !c.bias && !c.res && !c.mask; }
static inline bool dgrad_thin_out_f(const ConvCallF& c) { return dgrad_bare_f(c) && c.thin_out && c.out_al16; }
// thin INPUT: VGG16's first layer (the entry's 1x1 form is not routed here: see the forward).  The thin-input entry is TRIED at these.
static inline bool dgrad_thin_in_tried_f(const fmi_conv_desc* d, const ConvCallF& c) {
  return dgrad_bare_f(c) && d->C <= 4 && d->x_cstride == d->C && d->kh == 3;
}
static inline bool wgrad_thin_out_f(const ConvCallF& c) { return c.batch_w == 1 && c.thin_out && c.x_al16; }
// thin ConvTranspose2d(3, stride 2) on a large map: all four sub-pixel phases in one tap-reuse launch (convt3x3.h)
static inline bool dgrad_convt3x3_f(const fmi_conv_desc* d, const ConvCallF& c, bool strided_split) {
  return c.batch_w == 1 && !strided_split && !c.x3 && convt3x3_eligible_f(d, c.x_al16, weight_pieces_f(c.w3 && c.w3_al16, c.batch_w, d->K));
}
// Strided adjoints of small feature maps (the stride-2 style heads of the pSp encoder: 512 -> 512 at 16^2 .. 2^2) are a few
// output tiles per sub-pixel phase with up to 128 reduction tiles each -- 0.25 ms of pure load latency per call.  If any phase
// wants a split reduction, dx is initialised once and EVERY phase adds its (partial) sums atomically.  This is the test of ONE phase.
static inline bool dgrad_phase_wants_split_f(const fmi_conv_desc* d, const ConvCallF& c, int GH, int GW, int M, int Kdim) {
  return d->stride > 1 && c.batch_w == 1 && GH > 0 && GW > 0 && conv_ksplit_f(M, d->C, Kdim, c.det) > 1;
}
static inline bool dgrad_may_split_f(const fmi_conv_desc* d, const ConvCallF& c, bool strided_split) {
  return c.batch_w == 1 && (d->stride == 1 || strided_split);
}

// ---------------------------------------------------------------------------------------------
// Weight gradients: the split of the (long) pixel reduction over workgroups; partial sums meet through fp32 atomics
// ---------------------------------------------------------------------------------------------
// tiles: output tiles of the launch; P: pixels.  At least min_px pixels per split, about `budget` workgroups in all.  The four launch
// sites differ, and the differences are kept as they were (profiles/conv_f32_dispatch.txt):
//   xcd_round  the piece-image kernels deal splits to the 8 XCDs in groups of 8 and keep the groups full; the GEMM route does not
//   cap        65535 (grid y) on the GEMM routes, applied AFTER the reproducible-mode reset and with batch_w; on wgrad_p3_kernel applied
//              BEFORE the XCD rounding; wgrad3x3_p3_kernel has none (cap = 0)
//   batch_w    per-sample weights multiply the workgroups (GEMM route only)
static inline int64_t wgrad_split_f(int64_t tiles, int64_t P, int batch_w, int64_t cap, bool xcd_round, bool det, int min_px = 512, int budget = 2048) {
  int64_t ksplit = budget / (tiles * batch_w);
  const int64_t kmax = P / min_px;
  if (ksplit > kmax) ksplit = kmax;
  if (ksplit < 1) ksplit = 1;
  if (xcd_round) {
    if (cap && ksplit > cap) ksplit = cap;
    if (ksplit >= 6) ksplit = (ksplit + 4) / 8 * 8;  // splits are dealt to the 8 XCDs in groups of 8: keep the groups full
  }
  if (det) ksplit = 1;  // reproducible mode: one workgroup per tile walks the whole pixel reduction
  if (!xcd_round && cap && ksplit * batch_w > cap) ksplit = cap / batch_w;
  return ksplit;
}
static inline int64_t wgrad_gemm_tiles_f(int Mg, int Ng) { return plan_ceil_div_f(Mg, 128) * plan_ceil_div_f(Ng, Ng <= 32 ? 32 : (Ng <= 64 ? 64 : 128)); }

// both piece-image weight-gradient kernels (conv_p3.h)
static inline LaunchPlanF wgrad_p3_plan_f(const fmi_conv_desc* d, bool det) {
  LaunchPlanF pl{};
  const bool k3 = wgrad3x3_p3_ok_f(d);
  int64_t tm, P;
  int bn;
  if (k3) {
    pl.route = ROUTE_WGRAD_P3_3X3_F;
    bn = d->K <= 64 ? 64 : 128;
    tm = 3 * (d->C / 64);
    P = d->N * d->H * d->W;
    pl.tile = tile_id_f(192, bn);
  } else {
    pl.route = ROUTE_WGRAD_P3_F;
    bn = d->K <= 32 ? 32 : (d->K <= 64 ? 64 : 128);
    tm = plan_ceil_div_f(d->kh * d->kw * d->C, 128);
    P = d->N * d->OH * d->OW;
    pl.tile = tile_id_f(128, bn);
  }
  const int64_t tn = plan_ceil_div_f(d->K, bn);
  int64_t ks = wgrad_split_f(tm * tn, P, 1, k3 ? 0 : 65535, true, det);
  pl.asked = (int)ks;
  pl.chunk = (int)(plan_ceil_div_f(plan_ceil_div_f(P, ks), 16) * 16);
  ks = plan_ceil_div_f(P, pl.chunk);
  pl.ksplit = (int)ks;
  pl.xcd_splits = ks >= 8 ? 1 : 0;
  const int64_t nwg = pl.xcd_splits ? tm * tn * plan_ceil_div_f(ks, 8) * 8 : tm * tn;
  if (nwg > 0x7fffffffLL) return refused_f(FMI_ERR_UNSUPPORTED);
  pl.tiles = (int)(tm * tn);
  pl.tiles_n = (int)tn;
  pl.grid[0] = (unsigned)nwg;
  pl.grid[1] = pl.xcd_splits ? 1u : (unsigned)ks;
  pl.fl = pl.chunk > 640 && det;  // blocked accumulation of a long unsplit pixel reduction
  return pl;
}

// fmi_conv2d_wgrad_f32 after its thin-output exit.  Kdim = taps x C, P = pixels of the output; x_vec = WgradAX's dma_ok, dy_vec = DenseX's vec
struct WgradPlanF {
  LaunchPlanF pl;
  bool fuse_bias;  // the bias gradient rides along as one extra output row (needs a float4-aligned row index and shared weights)
};
static inline WgradPlanF wgrad_plan_f(const fmi_conv_desc* d, const ConvCallF& c, int Kdim, int P, bool x_vec, bool dy_vec) {
  WgradPlanF w{};
  // both operands as bf16 piece images (d->x3 = pieces of x, d->y3 = pieces of dy, INPUTS here): no split arithmetic, transposed LDS reads.
  // The bias gradient does not ride along on this path (the caller runs fmi_bias_grad_f32).
  if (c.batch_w == 1 && !c.bias && wgrad_p3_ok_f(d, c.x3 && c.x3_al16, c.y3 && c.y3_al16)) {
    w.pl = wgrad_p3_plan_f(d, c.det);
    return w;
  }
  w.fuse_bias = c.bias && c.batch_w == 1 && (Kdim % 4 == 0);
  if (c.bias && !w.fuse_bias) {
    w.pl = refused_f(FMI_ERR_UNSUPPORTED);
    return w;
  }
  const int Mg = Kdim + (w.fuse_bias ? 1 : 0), Ng = d->K;
  const int64_t ksplit = wgrad_split_f(wgrad_gemm_tiles_f(Mg, Ng), P, c.batch_w, 65535, false, c.det);
  w.pl = gemm_plan_f(ROUTE_WGRAD_GEMM_F, Mg, Ng, P, c.batch_w, (int)ksplit, x_vec && dy_vec && (Ng & 3) == 0, DMA_FAMILY_WGRAD_F, c.dma_off, c.det);
  return w;
}

// ---------------------------------------------------------------------------------------------
// The stride-1 ResBlock pair (conv_pair.h)
// ---------------------------------------------------------------------------------------------
static inline int pair_shape_check_f(const fmi_conv_desc* d, int C2) {  // after the descriptor check
  if (C2 <= 0) return FMI_ERR_BAD_ARG;
  if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1 || d->pad_mode != 0 || d->dil > 1) return FMI_ERR_UNSUPPORTED;
  if ((d->C & 15) || (C2 & 15) || (d->K & 3) || d->x_cstride != d->C || d->y_cstride != d->K) return FMI_ERR_UNSUPPORTED;
  if (9ll * d->C + C2 > 0x3fffffffLL || (int64_t)d->N * d->H * d->W >= (1ll << 30)) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
// reduction splits of the pair's forward, as the launch takes them (1: unsplit)
static inline int pair_ksplit_f(const fmi_conv_desc* d, int C2, int act, bool tap_reuse, bool det) {
  const int M = d->N * d->H * d->W, Kd = 9 * d->C + C2;
  int ks = act == 0 ? conv_ksplit_f(M, d->K, Kd, det) : 1;
  if (tap_reuse) {  // launch_conv3x3: whole (ky, 16 channels) steps per split
    const int nit = 3 * (d->C >> 4) + (C2 >> 4);
    if (ks > nit) ks = nit;
    const int it_chunk = (nit + ks - 1) / ks;
    return (nit + it_chunk - 1) / it_chunk;
  }
  const int kchunk = (int)plan_ceil_div_f(plan_ceil_div_f(Kd, ks), 16) * 16;  // launch_gemm: 16-deep tiles per split
  return (int)plan_ceil_div_f(Kd, kchunk);
}
static inline bool pair_tap_reuse_f(const fmi_conv_desc* d) {
  return (d->C >= 64 || d->K <= 32);  // conv3x3_eligible_f's channel rule; alignment is checked at the call
}
// Which passes of a supported shape the ResBlock routes to the pair: bit 0 the forward, bit 1 the weight gradient.  A pass is routed only where the
// fused launch was faster than conv2 + bypass in EVERY alternated round of tools/bench_tools/resblock_pair_time.py
// (profiles/resblock_pair.txt): the weight gradient at every measured shape (8 x 8^2 .. 8 x 128^2); the forward at all of them but
// 8 x 32^2 128 -> 128, a tie (39.6 against 39.5 us, lower in 2 rounds of 5).  Where conv2 runs from piece images of x1 today
// (functional.p3_wanted: >= 16384 pixels, C >= 64, K >= 128) only the measured shape, 8 x 64^2 64 -> 128, is routed.  Below 32 channels
// (nothing measured: the step has no such block) the two launches stay.
static inline int pair_routed_f(const fmi_conv_desc* d) {  // of a supported shape
  if (d->C < 32) return 0;
  const int64_t px = (int64_t)d->N * d->H * d->W;
  if (px >= 16384 && d->C >= 64 && d->K >= 128) return (d->C == 64 && d->K == 128 && px <= 32768) ? 3 : 0;
  const bool fwd_tie = d->C == 128 && d->K == 128 && px > 2048 && px < 16384;
  return fwd_tie ? 2 : 3;
}
// the pixel split of the pair's weight gradient: that of fmi_conv2d_wgrad_f32 over the taller row range, shared weights
static inline int64_t pair_wgrad_split_f(int Mg, int Ng, int P, bool det) { return wgrad_split_f(wgrad_gemm_tiles_f(Mg, Ng), P, 1, 65535, false, det); }
