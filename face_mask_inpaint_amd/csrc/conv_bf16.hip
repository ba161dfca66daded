// bf16 implicit-GEMM convolution family for the StyleGAN2 decoder of the pSp path (stylegan2/model.py:241-279, configs C3 / C5:
// bf16 compute, fp32 accumulate): forward, adjoint (= ConvTranspose2d forward / input gradient) and weight gradient.
//
// Machine mapping (gfx950):
//  * v_mfma_f32_32x32x16_bf16: lane l supplies A[row l&31][k = 8*(l>>5) .. +7] and B[k = 8*(l>>5) .. +7][col l&31] as eight bf16
//    (one 16-byte register quad); the 32x32 fp32 result has the layout of the fp32 core (gemm_core.h).
//  * operands reach LDS by global_load_lds_dwordx4 (LDS-DMA), 16 bytes = 8 bf16 per lane, two-stage ring, one raw s_barrier and a
//    counted s_waitcnt vmcnt per reduction tile -- the pipeline of gemm_dma_f32_kernel.
//  * forward / adjoint: both operands have the reduction index contiguous in memory (NHWC pixels x (tap, channel); weights packed
//    [out][tap][in]), so a tile image is [row][BK bf16] and ONE ds_read_b128 is one MFMA operand.  BK = 64 (128-byte rows, whole
//    cache lines per row) when the channel count allows, else 32.  The 16-byte chunk index is XOR-swizzled on the SOURCE address
//    (the DMA writes lane-linear) and on the read: (row>>1)&7 for 128-byte rows, (row>>2)&3 for 64-byte rows -- every 16-lane
//    group of a ds_read_b128 then covers all 64 banks once.
//  * weight gradient: the reduction runs over pixels, which are the SLOW index of both x[pixel][c] and dy[pixel][k]; the MFMA
//    operands come from ds_read_b64_tr_b16 (hardware transpose of a 4-pixel x 16-row block per 16 lanes), two per operand.  The
//    image is [32-row group][64 pixels][32 rows]: the four pixel rows one transposed read touches are 256 contiguous bytes (one
//    bank row, conflict-free without a swizzle) and all copies of a thread belong to one pixel (one anchor decode per tile).
#include <type_traits>

#include "bf16x8.h"
#include "conv_bf16_plan.h"
#include "gemm_core.h"

// ---------------------------------------------------------------------------------------------------------------------------
// host side of the dispatch that needs no GPU (also the g++ -DFMI_HOST_EMU build, tests/test_host_conv_bf16_plan.py): descriptor checks,
// the integer geometry of the phases, the inputs of the plan (conv_bf16_plan.h) and the query fmi_conv2d_bf16_plan
// ---------------------------------------------------------------------------------------------------------------------------
// kernel selection override (tests): 0 = by shape, 1 = never the 8-wave tiles, 2 = no eight-phase kernel, 8 = the eight-phase kernel
// wherever it is legal
static int g_bf16_tile_mode = 0;
extern "C" int fmi_debug_bf16_tile(int mode) {
  const int prev = g_bf16_tile_mode;
  if (mode >= 0) g_bf16_tile_mode = mode;
  return prev;
}
// the tile of the last launch of conv_bf16_kernel / the eight-phase kernel, whichever entry made it (tests assert which kernel a shape
// reached): the plan's tile id
static int g_bf16_last_tile = 0;
extern "C" int fmi_debug_bf16_last_tile(void) { return g_bf16_last_tile; }

static int check_desc_b(const fmi_conv_desc* d) {
  if (!d) return FMI_ERR_BAD_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0 ||
      d->x_cstride < d->C || d->y_cstride < d->K)
    return FMI_ERR_BAD_ARG;
  if (d->dil > 1) return FMI_ERR_UNSUPPORTED;  // dilated convolutions (modules/drn.py) exist in the fp32 family only
  if (d->OH != (d->H + 2 * d->pad - d->kh) / d->stride + 1 || d->OW != (d->W + 2 * d->pad - d->kw) / d->stride + 1) return FMI_ERR_BAD_ARG;
  if (d->OH <= 0 || d->OW <= 0) return FMI_ERR_BAD_ARG;
  if (d->pad_mode != 0) return FMI_ERR_UNSUPPORTED;
  if ((int64_t)d->N * d->H * d->W > 0x7fffffffLL / 2 || (int64_t)d->N * d->OH * d->OW > 0x7fffffffLL / 2 ||
      (int64_t)d->kh * d->kw * d->C > 0x3fffffffLL || (int64_t)d->kh * d->kw * d->K > 0x3fffffffLL)
    return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}

extern "C" int fmi_conv2d_bf16_supported(const fmi_conv_desc* d) {
  if (check_desc_b(d) != FMI_OK) return 0;
  return d->C % 32 == 0 && d->K % 32 == 0 && d->x_cstride % 8 == 0 && d->y_cstride % 8 == 0;
}

// The integer part of a launch's phases: one geometry per phase -- the one phase of a forward convolution (pass 0), or the non-empty
// sub-pixel phases (py, px) of the stride of an adjoint (pass 1: up to four, d->stride <= 2).  conv_set_b puts the pointers around.
struct ConvPhasesB {
  int nph;
  ConvGeom g[4];
  int py[4], px[4];
};
static ConvPhasesB conv_phases_b(const fmi_conv_desc* d, int pass) {
  ConvPhasesB ph{};
  if (pass == 0) {
    ConvGeom& g = ph.g[ph.nph++];
    g = fwd_geom(d, d->N);               // check_desc_b: no dilation, pad_mode 0.  img_bs stays 0: no per-sample weights in this family
    g.vec = d->C % 64 == 0 ? 6 : 5;      // here: log2 of the reduction tile BK (the fp32 family keeps a float4 flag in this field)
    g.dC = make_fastdiv(g.nty * g.ntx);  // here: divides by the number of TAPS (ConvKB::tile; the weight gradients and fp32 divide by C)
    return ph;
  }
  const int s = d->stride;
  for (int py = 0; py < s; ++py) {
    for (int px = 0; px < s; ++px) {
      ConvGeom g = adj_geom(d, d->N, py, px);  // img_bs stays 0: no per-sample weights in this family
      if (g.GH <= 0 || g.GW <= 0) continue;
      g.vec = d->K % 64 == 0 ? 6 : 5;                              // here: log2 of the reduction tile
      g.dC = make_fastdiv(g.nty * g.ntx > 0 ? g.nty * g.ntx : 1);  // here: divides by the number of TAPS (1: the empty phase)
      ph.py[ph.nph] = py, ph.px[ph.nph] = px;
      ph.g[ph.nph++] = g;
    }
  }
  return ph;
}
// elements of the tensor a pass writes (y of the forward, dx of the adjoint) and whether it takes the 8-byte stores (ConvEpB::vec)
static int64_t out_elems_b(const fmi_conv_desc* d, int pass) {
  return pass == 0 ? (int64_t)d->N * d->OH * d->OW * d->y_cstride : (int64_t)d->N * d->H * d->W * d->x_cstride;
}
static int out_vec_b(const fmi_conv_desc* d, int pass, bool out_al8) {
  return ((pass == 0 ? d->K % 4 == 0 && d->y_cstride % 4 == 0 : d->C % 4 == 0 && d->x_cstride % 4 == 0) && out_al8) ? 1 : 0;
}
// The plan's inputs of a call.  flags: FMI_PLAN_* (include/fmi_hip.h) -- what the plan reads of the call's pointers, which an entry derives
// from them and the query is told; without FMI_PLAN_MODES the reproducible mode and the tile mode are the library's current ones.
static bool plan_det_b(int flags) { return flags & FMI_PLAN_MODES ? (flags & FMI_PLAN_DET) != 0 : fmi_det(); }
static int plan_tile_mode_b(int flags) { return flags & FMI_PLAN_MODES ? (flags >> 8) & 15 : g_bf16_tile_mode; }
static ConvPlanInB conv_plan_in_b(const fmi_conv_desc* d, int pass, int stage, int groups, const ConvPhasesB& ph, int flags) {
  ConvPlanInB in{};
  in.stage = stage;
  in.BK = 1 << ph.g[0].vec;
  in.N = pass == 0 ? d->K : d->C;
  in.groups = groups;
  in.nph = ph.nph;
  for (int p = 0; p < ph.nph; ++p) {
    in.M[p] = ph.g[p].Mdim(), in.K[p] = ph.g[p].Kdim(), in.taps[p] = ph.g[p].ntaps();
    in.vec[p] = out_vec_b(d, pass, (flags & FMI_PLAN_OUT_AL8) != 0);
  }
  in.colscale = (flags & FMI_PLAN_COLSCALE) != 0, in.colscale_al16 = (flags & FMI_PLAN_COLSCALE_AL16) != 0;
  in.split_ws = (flags & FMI_PLAN_SPLIT_WS) && out_elems_b(d, pass) % 4 == 0;
  in.det = plan_det_b(flags), in.tile_mode = plan_tile_mode_b(flags);
  return in;
}
static WgradPlanInB wgrad_plan_in_b(const fmi_conv_desc* d, int flags) {
  return WgradPlanInB{d->kh * d->kw * d->C, d->K, d->N * d->OH * d->OW, (int64_t)d->N * d->H * d->W * d->x_cstride, plan_det_b(flags),
                      plan_tile_mode_b(flags)};
}

/* The plan of a launch without the launch (include/fmi_hip.h): the entries fill the plan's inputs through the functions above, and so
 * does this.  The descriptor is checked as every entry checks it first; the further refusals of an entry (channel multiples, pointers)
 * are the entry's. */
extern "C" int fmi_conv2d_bf16_plan(const fmi_conv_desc* d, int pass, int stage, int groups, int flags, int* out) {
  if (!out || pass < 0 || pass > 2 || stage < STAGE_PLAIN_B || stage > STAGE_MASK_B || groups < 1) return FMI_ERR_BAD_ARG;
  for (int i = 0; i < FMI_CONV_BF16_PLAN_INTS; ++i) out[i] = 0;
  int rc = check_desc_b(d);
  if (rc == FMI_OK && pass == 1 && d->stride > 2) rc = FMI_ERR_UNSUPPORTED;  // at most four sub-pixel phases per launch
  if (rc) return out[0] = rc;
  ConvPhasesB ph{};
  ph.nph = 1;
  if (pass < 2) ph = conv_phases_b(d, pass);
  const ConvPlanB pl = pass == 2 ? wgrad_plan_b(wgrad_plan_in_b(d, flags)) : conv_plan_b(conv_plan_in_b(d, pass, stage, groups, ph, flags));
  if (pl.status) return out[0] = pl.status;
  const int v[FMI_CONV_BF16_PLAN_INTS] = {FMI_OK, pl.tile, pl.ksplit, (int)pl.grid[0], (int)pl.grid[1], (int)pl.grid[2], pl.tiles[0],
                                          pl.tiles[1], pl.tiles[2], pl.tiles[3], pl.tiles_n, ph.nph, pl.kchunk, pl.xcd_splits};
  for (int i = 0; i < FMI_CONV_BF16_PLAN_INTS; ++i) out[i] = v[i];
  return FMI_OK;
}

#ifndef FMI_HOST_EMU
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------------------
// loaders (LDS-DMA hooks only: chunk = 8 consecutive reduction elements of one row)
// ---------------------------------------------------------------------------------------------------------------------------
struct ConvKB {  // A operand: gathered pixels x (tap, channel); a reduction tile lies inside one tap (C % BK == 0), zero padding
  const bf16_t* p;
  ConvGeom g;
  struct DCtx {
    int64_t boff;
    int ry, rx;
  };
  struct Tile {
    int dy, dx;
    int64_t uoff;
  };
  __device__ DCtx dprep(int x, int kq) const {
    DCtx d;
    if (x >= g.Mdim()) {
      d.ry = -0x20000000, d.rx = 0, d.boff = 0;
      return d;
    }
    const uint32_t n = fdiv((uint32_t)x, g.dG);
    const uint32_t rem = (uint32_t)x - n * (uint32_t)(g.GH * g.GW);
    const uint32_t gy = fdiv(rem, g.dGW);
    const uint32_t gx = rem - gy * (uint32_t)g.GW;
    d.ry = (int)gy * g.S + g.dy0;
    d.rx = (int)gx * g.S + g.dx0;
    d.boff = ((int64_t)((int)n * g.IH + d.ry) * g.IW + d.rx) * g.cstride + kq;
    return d;
  }
  // Reduction order: channel chunk (one reduction tile of BK = 1 << g.vec channels) OUTER, tap INNER -- the taps of a chunk re-read
  // the same pixels, so they follow each other while those bytes are in L2 (tap-major order re-fetched the activation once per tap:
  // FETCH_SIZE 4x the operand bytes at 512 channels).  g.dC divides by the number of taps here.
  __device__ Tile tile(int k0) const {
    const int kt = k0 >> g.vec;
    const int chunk = (int)fdiv((uint32_t)kt, g.dC), tp = kt - chunk * g.ntaps();
    const int i = (int)fdiv((uint32_t)tp, g.dntx), j = tp - i * g.ntx;
    Tile t;
    t.dy = g.ystep * i;
    t.dx = g.xstep * j;
    t.uoff = ((int64_t)(g.ystep * i) * g.IW + t.dx) * g.cstride + (chunk << g.vec);
    return t;
  }
  __device__ const bf16_t* chunk(const DCtx& d, const Tile& t) const {
    const bool ok = (unsigned)(d.ry + t.dy) < (unsigned)g.IH && (unsigned)(d.rx + t.dx) < (unsigned)g.IW;
    return ok ? p + d.boff + t.uoff : nullptr;
  }
};

struct ConvWKB {  // B operand: weights packed [Nout][T taps][Cred] (reduction contiguous)
  const bf16_t* p;
  ConvGeom g;  // tap algebra and C
  int Nout, T;
  struct DCtx {
    int64_t off;
  };
  struct Tile {
    int toff;
  };
  __device__ DCtx dprep(int x, int kq) const { return DCtx{x < Nout ? (int64_t)x * T * g.C + kq : -1}; }
  __device__ Tile tile(int k0) const {
    const int kt = k0 >> g.vec;
    const int chunk = (int)fdiv((uint32_t)kt, g.dC), tp = kt - chunk * g.ntaps();
    const int i = (int)fdiv((uint32_t)tp, g.dntx), j = tp - i * g.ntx;
    const int wtap = (g.kh0 + g.khstep * i) * g.kw + (g.kw0 + g.kwstep * j);
    return Tile{wtap * g.C + (chunk << g.vec)};
  }
  __device__ const bf16_t* chunk(const DCtx& d, const Tile& t) const { return (d.off >= 0 && t.toff >= 0) ? p + d.off + t.toff : nullptr; }
};

struct ConvEpB {  // rows = anchors, written at (gy*OS+py, gx*OS+px) of the bf16 tensor [N][OHt][OWt][cstride]
  bf16_t* y;
  const float* colscale;  // [N][Nout] or null: y *= colscale[sample][col] (demodulation, model.py:250-252)
  int GH, GW, OS, py, px, OHt, OWt, cstride, Nout;
  FastDiv dGW, dG;
  int vec;
  __device__ int64_t row_pix(int row, int& n_out) const {  // pixel index of the output tensor
    const uint32_t n = fdiv((uint32_t)row, dG);
    const uint32_t rem = (uint32_t)row - n * (uint32_t)(GH * GW);
    const uint32_t gy = fdiv(rem, dGW);
    const uint32_t gx = rem - gy * (uint32_t)GW;
    n_out = (int)n;
    return (int64_t)((int)n * OHt + (int)gy * OS + py) * OWt + ((int)gx * OS + px);
  }
  __device__ int64_t row_off(int row, int& n_out) const { return row_pix(row, n_out) * cstride; }
};

// ---------------------------------------------------------------------------------------------------------------------------
// forward / adjoint kernel
// ---------------------------------------------------------------------------------------------------------------------------
// tiles of the bf16 kernels: WM x WN waves (4 or 8), each TM x TN accumulators of 32 x 32
template <int WM_, int WN_, int TM_, int TN_>
struct TileB {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_;
  static constexpr int BM = WM * TM * 32, BN = WN * TN * 32, NT = WM * WN * 64;
};
using TB128x128 = TileB<2, 2, 2, 2>;
using TB128x64 = TileB<2, 2, 2, 1>;
using TB128x32 = TileB<4, 1, 1, 1>;
using TB64x64 = TileB<2, 2, 1, 1>;
using TB64x128 = TileB<2, 2, 1, 2>;
using TB256x256 = TileB<2, 4, 4, 2>;  // 8 waves, 128 x 64 per wave: 128 FLOP per staged byte (the 128 x 128 tile: 64 -> L2-rate bound)

// One launch = up to four "phases" (the sub-pixel phases of a strided adjoint, i.e. of a ConvTranspose2d forward; one phase
// otherwise) x an optional split of the reduction: grid = (tiles of the largest phase, phases, splits).
struct ConvPhaseB {
  ConvKB la;
  ConvWKB lb;
  ConvEpB ep;
  int M, K, tiles;
};
struct ConvSetB {
  ConvPhaseB ph[4];
  int N, tiles_n, ksplit;
  float* ws;  // split reduction: fp32 twin of the output (zeroed by the caller), partial sums meet through atomics
};

// Output stages of conv_bf16_kernel.  EpNoneB: the plain store (and the split-reduction / per-sample column scale forms).
// EpChanB: a per-column stage for the eval-mode IR-SE block (modules/psp/encoders/helpers.py:85-89 / :107-113 of the reference):
// v = acc * scale[k] + bias[k] (the folded eval BatchNorm behind conv2 and behind the shortcut convolution), y = v > 0 ? v : slope[k] * v
// (the PReLU behind conv1), one rounding to bf16.  colsum (may be null): the fp32 sums of v over the rows of every FMI_CHAN_COLSUM_ROWS-row
// block, per sample -- a block straddles at most two samples (the host refuses maps with fewer rows than a tile), so it owns two rows of
// the workspace: [block][0] = its rows of the sample its first row lies in, [block][1] = its rows of the next sample.  Every row of the
// workspace is written by exactly one wave, in full: no initialisation, no atomics, the same bits every run.
struct EpNoneB {};
// EpGroupB: G convolutions of one launch (the map2style heads of one pyramid level, psp_encoders.py:13-37 of the reference).  The group is
// the grid's y index -- a launch of this stage has ONE phase, set.ph[0], shared by all groups -- and offsets x, the weights, the bias and
// y; set.N is the number of output columns of one group.  v = acc + bias[g][k], y = v > 0 ? v : slope * v, one rounding to bf16.
struct EpGroupB {
  const float* bias;  // [G][Nout] or null (= 0)
  float slope;
  int64_t x_off;      // elements between the first channels of consecutive groups inside a pixel of x (0: one shared map)
  int64_t w_off;      // elements between the weight packs of consecutive groups
};
struct EpChanB {
  const float* scale;  // [Nout] or null (= 1)
  const float* bias;   // [Nout] or null (= 0)
  const float* slope;  // [Nout] or null (= 1)
  float* colsum;       // [ceil(M / 64)][2][Nout] or null
};

// EpMaskB: the adjoint whose result is the gradient of a ReLU's OUTPUT (the VGG16 trunk of VGGLoss in bf16, modules/loss.py:33-52 of the
// reference: the convolutions of a block that read another convolution's activated map).  a = that activated map, with the geometry and
// channel stride of the tensor this launch writes: y = a > 0 ? acc : 0, one rounding to bf16, 8-byte loads of a beside the 8-byte stores.
// Also the output stage of the eight-phase kernel (conv_bf16_8ph.h).  One phase, no split reduction.
struct EpMaskB {
  const bf16_t* a;
};
template <class V>  // float[4] or a four-float vector: both kernels apply ONE rule (a NaN and a negative zero mask)
__device__ __forceinline__ void ep_mask4(uint2 m, V& v) {
  v[0] = bf_lo(m.x) > 0.f ? v[0] : 0.f, v[1] = bf_hi(m.x) > 0.f ? v[1] : 0.f;
  v[2] = bf_lo(m.y) > 0.f ? v[2] : 0.f, v[3] = bf_hi(m.y) > 0.f ? v[3] : 0.f;
}

template <class T, int BK, int NST = 2, class CH = EpNoneB>
__global__ void __launch_bounds__(T::NT) conv_bf16_kernel(ConvSetB set, CH ch) {
  const float* const zchunk = fmi_zero_chunk_ptr();  // the zero chunk's address: read from the GOT ONCE (see fmi_zero_chunk_ptr)
  constexpr int BM = T::BM, BN = T::BN, NT = T::NT;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  constexpr bool GRP = std::is_same<CH, EpGroupB>::value;
  const unsigned phi = GRP ? 0u : blockIdx.y;  // unsigned as before: the other stages compile to the code they had
  const int grp = GRP ? (int)blockIdx.y : 0;
  if (lid >= set.ph[phi].tiles) return;  // whole workgroup
  const ConvKB la = [&] {
    ConvKB a = set.ph[phi].la;
    if constexpr (GRP) a.p += (int64_t)grp * ch.x_off;
    return a;
  }();
  const ConvWKB lb = [&] {
    ConvWKB b = set.ph[phi].lb;
    if constexpr (GRP) b.p += (int64_t)grp * ch.w_off;
    return b;
  }();
  const ConvEpB ep = [&] {
    ConvEpB e = set.ph[phi].ep;
    if constexpr (GRP) e.y += (int64_t)grp * set.N;
    return e;
  }();
  const int M = set.ph[phi].M, K = set.ph[phi].K, N = set.N, tiles_n = set.tiles_n;
  constexpr int CPR = BK / 8;            // 16-byte chunks per image row
  constexpr int NLA = (BM * CPR + NT - 1) / NT, NLB = (BN * CPR + NT - 1) / NT;
  constexpr int STAGE = (BM + BN) * BK;  // bf16 elements
  constexpr int DEPTH = NST - 1;  // tiles copied ahead of the one computed
  __shared__ __attribute__((aligned(1024))) bf16_t lds[NST * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int tile_m = lid / tiles_n, tile_n = lid - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int wm = (wid / T::WN) * T::TM * 32, wn = (wid % T::WN) * T::TN * 32;

  auto swz = [](int row) { return CPR == 8 ? (row >> 1) & 7 : (row >> 2) & 3; };

  ConvKB::DCtx da[NLA];
  ConvWKB::DCtx db[NLB];
#pragma unroll
  for (int j = 0; j < NLA; ++j) {
    const int p = j * NT + tid, x = p / CPR, c = (p % CPR) ^ swz(x);
    da[j] = la.dprep(m0 + x, c * 8);
  }
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
    const int p = j * NT + tid, x = p / CPR, c = (p % CPR) ^ swz(x);
    db[j] = lb.dprep(n0 + x, c * 8);
  }
  // images smaller than 256 chunks are filled by the first waves only (wave-uniform)
  static_assert(BM * CPR % NT == 0 || BM * CPR < NT, "A image: whole instructions per thread, or fewer chunks than threads");
  static_assert(BN * CPR % NT == 0 || BN * CPR < NT, "B image: whole instructions per thread, or fewer chunks than threads");
  const int na_w = (BM * CPR % NT == 0) ? NLA : (wid * 64 < BM * CPR ? 1 : 0);
  const int nb_w = (BN * CPR % NT == 0) ? NLB : (wid * 64 < BN * CPR ? 1 : 0);

  f32x16 acc[T::TM][T::TN];
#pragma unroll
  for (int i = 0; i < T::TM; ++i)
#pragma unroll
    for (int j = 0; j < T::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) bf16_t*)lds;
  auto glds16 = [&](const void* g, uint32_t dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(dst)
                 : "memory");
  };
  auto issue = [&](int k0, int st) {
    const uint32_t sa = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(st * STAGE) * 2u + (uint32_t)wid * 1024u);
    const uint32_t sb = sa + BM * BK * 2;
    const ConvKB::Tile ta = la.tile(k0);
    const ConvWKB::Tile tb = lb.tile(k0);
#pragma unroll
    for (int j = 0; j < NLA; ++j) {
      if (BM * CPR % NT != 0 && !na_w) break;
      const void* g = la.chunk(da[j], ta);
      if (!g) g = zchunk;
      glds16(g, sa + j * NT * 16);
    }
#pragma unroll
    for (int j = 0; j < NLB; ++j) {
      if (BN * CPR % NT != 0 && !nb_w) break;
      const void* g = lb.chunk(db[j], tb);
      if (!g) g = zchunk;
      glds16(g, sb + j * NT * 16);
    }
  };
  auto compute = [&](int st) {
    const bf16_t* sa = lds + st * STAGE;
    const bf16_t* sb = sa + BM * BK;
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 fa[T::TM], fb[T::TN];
#pragma unroll
      for (int i = 0; i < T::TM; ++i) {
        const int r = wm + i * 32 + l31;
        fa[i] = *reinterpret_cast<const bf16x8*>(sa + r * BK + (((2 * s + lh) ^ swz(r)) << 3));
      }
#pragma unroll
      for (int j = 0; j < T::TN; ++j) {
        const int r = wn + j * 32 + l31;
        fb[j] = *reinterpret_cast<const bf16x8*>(sb + r * BK + (((2 * s + lh) ^ swz(r)) << 3));
      }
#pragma unroll
      for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  };
  auto wait_copies = [&](int n) {
    switch (n) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
      case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
      case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
      case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
      case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
  const int nt_all = (K + BK - 1) / BK, per = (nt_all + set.ksplit - 1) / set.ksplit;
  const int kt0 = blockIdx.z * per;
  const int nt = (kt0 + per <= nt_all ? per : nt_all - kt0);  // reduction tiles of this split (may be <= 0)
  // no reduction tile for this split: nothing to add -- EXCEPT a phase with an empty reduction (K = 0: the three tap-less sub-pixel
  // phases of the adjoint of a 1x1 stride-2 convolution, the IR-SE shortcut of the pSp encoder), whose outputs are zeros that must be
  // WRITTEN when the result goes straight to y (with a zero-initialised split workspace they already are)
  if (nt <= 0 && (K > 0 || blockIdx.z > 0 || set.ws)) return;
  const int nw = (BM * CPR % NT == 0 && BN * CPR % NT == 0) ? NLA + NLB : na_w + nb_w;  // copies this wave issues per tile
#pragma unroll
  for (int p = 0; p < DEPTH; ++p)
    if (p < nt) issue((kt0 + p) * BK, p);
  int st = 0, stn = DEPTH;
  for (int t = 0; t < nt; ++t) {
    int pend = nt - 1 - t;  // tile t must have landed; up to DEPTH-1 newer tiles may stay in flight
    if (pend > DEPTH - 1) pend = DEPTH - 1;
    wait_copies(pend * nw);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + DEPTH < nt) issue((kt0 + t + DEPTH) * BK, stn);
    compute(st);
    st = st == NST - 1 ? 0 : st + 1;
    stn = stn == NST - 1 ? 0 : stn + 1;
  }

  // epilogue: 4 x 4 transpose inside each quad of lanes -> one row, four consecutive columns per lane, 8-byte bf16 stores
  const int c = l31 & 3, colq = l31 & ~3;
  if constexpr (GRP) {  // N % 4 == 0, 8-byte aligned rows of y, 16-byte aligned bias (the host checks)
    const float* const bias = ch.bias ? ch.bias + (int64_t)grp * N : nullptr;
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = m0 + wm + i * 32 + 8 * g + 4 * lh + c;
        int n_s = 0;
        const int64_t off = row < M ? ep.row_off(row, n_s) : 0;
#pragma unroll
        for (int j = 0; j < T::TN; ++j) {
          float a[4] = {acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          quad_transpose(a, c);
          const int col = n0 + wn + j * 32 + colq;
          if (row >= M || col >= N) continue;
          const float4 b = bias ? *reinterpret_cast<const float4*>(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = a[e] + bv[e];
            a[e] = v > 0.f ? v : ch.slope * v;
          }
          uint2 v;
          v.x = bf_pack2(a[0], a[1]);
          v.y = bf_pack2(a[2], a[3]);
          *reinterpret_cast<uint2*>(ep.y + off + col) = v;
        }
      }
    }
    return;
  }
  if constexpr (std::is_same<CH, EpChanB>::value) {
    static_assert(T::TM == 2, "a wave owns one 64-row block of the column-sum workspace");
    // the lane's columns are the same for all of its rows: the three per-column vectors once per 32-column group
    float4 sc[T::TN], bs[T::TN], sl[T::TN];
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
      const int col = n0 + wn + j * 32 + colq;
      sc[j] = sl[j] = make_float4(1.f, 1.f, 1.f, 1.f);
      bs[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < N) {
        if (ch.scale) sc[j] = *reinterpret_cast<const float4*>(ch.scale + col);
        if (ch.bias) bs[j] = *reinterpret_cast<const float4*>(ch.bias + col);
        if (ch.slope) sl[j] = *reinterpret_cast<const float4*>(ch.slope + col);
      }
    }
    const int rb0 = m0 + wm;  // first row of this wave's 64-row block
    const int bound = ((int)fdiv((uint32_t)rb0, ep.dG) + 1) * (ep.GH * ep.GW);  // first row of the next sample
    float s0[T::TN][4], s1[T::TN][4];
#pragma unroll
    for (int j = 0; j < T::TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) s0[j][e] = s1[j][e] = 0.f;
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = rb0 + i * 32 + 8 * g + 4 * lh + c;
        const bool rv = row < M;
        int n_s = 0;
        const int64_t off = rv ? ep.row_off(row, n_s) : 0;
#pragma unroll
        for (int j = 0; j < T::TN; ++j) {
          float a[4] = {acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          quad_transpose(a, c);
          const int col = n0 + wn + j * 32 + colq;
          const float scv[4] = {sc[j].x, sc[j].y, sc[j].z, sc[j].w}, bsv[4] = {bs[j].x, bs[j].y, bs[j].z, bs[j].w};
          const float slv[4] = {sl[j].x, sl[j].y, sl[j].z, sl[j].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = a[e] * scv[e] + bsv[e];
            if (ch.colsum && rv) {
              if (row < bound) s0[j][e] += v;
              else s1[j][e] += v;
            }
            a[e] = v > 0.f ? v : slv[e] * v;
          }
          if (rv && col < N) {
            uint2 v;
            v.x = bf_pack2(a[0], a[1]);
            v.y = bf_pack2(a[2], a[3]);
            *reinterpret_cast<uint2*>(ep.y + off + col) = v;
          }
        }
      }
    }
    if (ch.colsum) {  // the eight lanes that share a column group hold eight rows each: two quad steps and the two wave halves
#pragma unroll
      for (int j = 0; j < T::TN; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float u0 = s0[j][e], u1 = s1[j][e];
          u0 += __shfl_xor(u0, 1, 64), u1 += __shfl_xor(u1, 1, 64);
          u0 += __shfl_xor(u0, 2, 64), u1 += __shfl_xor(u1, 2, 64);
          u0 += __shfl_xor(u0, 32, 64), u1 += __shfl_xor(u1, 32, 64);
          s0[j][e] = u0, s1[j][e] = u1;
        }
        const int col = n0 + wn + j * 32 + colq;
        if (c == 0 && lh == 0 && rb0 < M && col < N) {
          float* dst = ch.colsum + (int64_t)(rb0 >> 6) * 2 * N + col;
          *reinterpret_cast<float4*>(dst) = make_float4(s0[j][0], s0[j][1], s0[j][2], s0[j][3]);
          *reinterpret_cast<float4*>(dst + N) = make_float4(s1[j][0], s1[j][1], s1[j][2], s1[j][3]);
        }
      }
    }
    return;
  }
  if constexpr (std::is_same<CH, EpMaskB>::value) {  // N % 4 == 0, 8-byte aligned rows of y and of the mask's map (the host checks)
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = m0 + wm + i * 32 + 8 * g + 4 * lh + c;
        int n_s = 0;
        const int64_t off = row < M ? ep.row_off(row, n_s) : 0;
#pragma unroll
        for (int j = 0; j < T::TN; ++j) {
          float a[4] = {acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          quad_transpose(a, c);
          const int col = n0 + wn + j * 32 + colq;
          if (row >= M || col >= N) continue;
          ep_mask4(*reinterpret_cast<const uint2*>(ch.a + off + col), a);
          uint2 v;
          v.x = bf_pack2(a[0], a[1]);
          v.y = bf_pack2(a[2], a[3]);
          *reinterpret_cast<uint2*>(ep.y + off + col) = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < T::TM; ++i) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = m0 + wm + i * 32 + 8 * g + 4 * lh + c;
      int n_s = 0;
      const int64_t off = row < M ? ep.row_off(row, n_s) : 0;
#pragma unroll
      for (int j = 0; j < T::TN; ++j) {
        float a[4] = {acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        quad_transpose(a, c);
        const int col = n0 + wn + j * 32 + colq;
        if (row >= M || col >= N) continue;
        if (set.ws) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < N) atomicAdd(set.ws + off + col + e, a[e]);
          continue;
        }
        if (ep.colscale) {
          const float* cs = ep.colscale + (int64_t)n_s * ep.Nout + col;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < N) a[e] *= cs[e];
        }
        if (ep.vec) {
          uint2 v;
          v.x = bf_pack2(a[0], a[1]);
          v.y = bf_pack2(a[2], a[3]);
          *reinterpret_cast<uint2*>(ep.y + off + col) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < N) ep.y[off + col + e] = bf_round(a[e]);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    uint2 o;
    o.x = bf_pack2(v.x, v.y);
    o.y = bf_pack2(v.z, v.w);
    reinterpret_cast<uint2*>(dst)[i] = o;
  }
}

#include "conv_bf16_8ph.h"

// ---------------------------------------------------------------------------------------------------------------------------
// the launcher of the forward / adjoint entries: conv_bf16_plan.h decides, this launches what it decided
// ---------------------------------------------------------------------------------------------------------------------------
template <class T>
struct Is8P : std::false_type {};
template <int WM, int WN>
struct Is8P<Tile8P<WM, WN>> : std::true_type {};

// The (tile, BK, output stage) combinations that exist as kernels -- what this predicate admits is what the library instantiates: every
// TileB tile with the plain store, at both BK; with 64-deep reduction tiles the masked stage on at least 64 columns, the per-column stage
// on the two tiles of two 64-row wave blocks, the grouped stage on the four tiles of its table; the eight-phase kernel with its own
// stage (EpActB, which also is its plain store) and the masked one.
template <class TILE, int BK, class EP>
constexpr bool conv_kernel_exists_b() {
  if (Is8P<TILE>::value) return BK == 64 && (std::is_same<EP, EpActB>::value || std::is_same<EP, EpMaskB>::value);
  if (std::is_same<EP, EpNoneB>::value) return true;
  if (std::is_same<EP, EpMaskB>::value) return BK == 64 && TILE::BN >= 64;
  if (std::is_same<EP, EpChanB>::value) return BK == 64 && TILE::BM == 128 && TILE::BN >= 64;
  if (std::is_same<EP, EpGroupB>::value) return BK == 64 && TILE::BM <= TILE::BN;
  return false;
}
template <class TILE, int BK, class EP>
static int launch_tile_b(const ConvSetB& set, const ConvPlanB& pl, const EP& ep, hipStream_t st) {
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]);
  if constexpr (Is8P<TILE>::value && std::is_same<EP, EpNoneB>::value) {
    return launch_tile_b<TILE, BK>(set, pl, EpActB{}, st);  // the plain store of the eight-phase kernel: its own stage, switched off
  } else if constexpr (!conv_kernel_exists_b<TILE, BK, EP>()) {
    return FMI_ERR_UNSUPPORTED;  // the plan returns no such combination
  } else {
    if constexpr (Is8P<TILE>::value) hipLaunchKernelGGL((conv_bf16_8ph_kernel<TILE, EP>), grid, dim3(TILE::NT), 0, st, set, ep);
    else hipLaunchKernelGGL((conv_bf16_kernel<TILE, BK, 2, EP>), grid, dim3(TILE::NT), 0, st, set, ep);
    return FMI_OK;
  }
}
template <int BK, class EP>
static int launch_conv_bf16(const ConvSetB& set, const ConvPlanB& pl, const EP& ep, hipStream_t st) {
  switch (pl.tile) {
    case tile_id_b(128, 32): return launch_tile_b<TB128x32, BK>(set, pl, ep, st);
    case tile_id_b(128, 64): return launch_tile_b<TB128x64, BK>(set, pl, ep, st);
    case tile_id_b(64, 64): return launch_tile_b<TB64x64, BK>(set, pl, ep, st);
    case tile_id_b(64, 128): return launch_tile_b<TB64x128, BK>(set, pl, ep, st);
    case tile_id_b(128, 128): return launch_tile_b<TB128x128, BK>(set, pl, ep, st);
    case tile_id_b(256, 256): return launch_tile_b<TB256x256, BK>(set, pl, ep, st);
    case tile_id_b(512, 128, true): return launch_tile_b<T8P512x128, BK>(set, pl, ep, st);
    case tile_id_b(256, 256, true): return launch_tile_b<T8P256x256, BK>(set, pl, ep, st);
  }
  return FMI_ERR_UNSUPPORTED;
}

// The ConvSetB of a launch: the pointers around the phases' geometry (both loaders, the addressing of the output stage) and the plan's
// tile counts and split.  a: the gathered tensor (x of the forward, dy of the adjoint), w: the weights packed [columns][kh*kw][reduction]
// ([K][taps][C] forward, [C][taps][K] adjoint), out: y / dx.  ws: the split reduction's fp32 twin of the output, used when the plan splits.
static ConvSetB conv_set_b(const fmi_conv_desc* d, int pass, const ConvPhasesB& ph, const ConvPlanInB& in, const ConvPlanB& pl, const uint16_t* a,
                           const uint16_t* w, const float* colscale, uint16_t* out, float* ws) {
  ConvSetB set{};
  for (int p = 0; p < ph.nph; ++p) {
    const ConvGeom& g = ph.g[p];
    ConvPhaseB& P = set.ph[p];
    P.la = ConvKB{a, g};
    P.lb = ConvWKB{w, g, in.N, d->kh * d->kw};
    if (pass == 0) P.ep = ConvEpB{out, colscale, g.GH, g.GW, 1, 0, 0, d->OH, d->OW, d->y_cstride, in.N, g.dGW, g.dG, in.vec[p]};
    else P.ep = ConvEpB{out, colscale, g.GH, g.GW, d->stride, ph.py[p], ph.px[p], d->H, d->W, d->x_cstride, in.N, g.dGW, g.dG, in.vec[p]};
    P.M = in.M[p], P.K = in.K[p], P.tiles = pl.tiles[p];
  }
  set.N = in.N, set.tiles_n = pl.tiles_n, set.ksplit = pl.ksplit;
  set.ws = pl.ksplit > 1 ? ws : nullptr;
  return set;
}

// Every forward / adjoint entry behind its argument checks: phases, plan, set, launch -- and, where the plan split the reduction (small
// feature maps with a deep reduction; partial sums meet through atomics in ws, which the caller zeroed), the conversion of the sums to bf16.
template <class EP>
static int run_conv_b(const fmi_conv_desc* d, int pass, int stage, int groups, const uint16_t* a, const uint16_t* w, const float* colscale,
                      uint16_t* out, float* ws, int64_t ws_floats, const EP& ep, void* stream) {
  const ConvPhasesB ph = conv_phases_b(d, pass);
  const int64_t out_elems = out_elems_b(d, pass);
  const bool out_al8 = ((uintptr_t)out & 7) == 0;
  const int flags = (out_al8 ? FMI_PLAN_OUT_AL8 : 0) | (colscale ? FMI_PLAN_COLSCALE : 0) | (fmi_al16(colscale) ? FMI_PLAN_COLSCALE_AL16 : 0) |
                    (ws && fmi_al16(ws) && out_al8 && ws_floats >= out_elems ? FMI_PLAN_SPLIT_WS : 0);
  const ConvPlanInB in = conv_plan_in_b(d, pass, stage, groups, ph, flags);
  const ConvPlanB pl = conv_plan_b(in);
  if (pl.status) return pl.status;
  const ConvSetB set = conv_set_b(d, pass, ph, in, pl, a, w, colscale, out, ws);
  hipStream_t st = (hipStream_t)stream;
  g_bf16_last_tile = pl.tile;
  const int rc = in.BK == 64 ? launch_conv_bf16<64>(set, pl, ep, st) : launch_conv_bf16<32>(set, pl, ep, st);
  if (rc) return rc;
  if (pl.ksplit > 1) hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(fmi_bw_grid(out_elems / 4, 256)), dim3(256), 0, st, ws, out, out_elems / 4);
  return fmi_launch_status();
}

static int conv2d_fwd_bf16_check(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const uint16_t* y) {
  int rc = check_desc_b(d);
  if (rc) return rc;
  if (!x || !wnk || !y) return FMI_ERR_BAD_ARG;
  if (d->C % 32 != 0 || d->x_cstride % 8 != 0 || !fmi_al16(x) || !fmi_al16(wnk)) return FMI_ERR_UNSUPPORTED;
  return FMI_OK;
}
extern "C" int fmi_conv2d_fwd_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* colscale, uint16_t* y,
                                   float* ws, int64_t ws_floats, void* stream) {
  int rc = conv2d_fwd_bf16_check(d, x, wnk, y);
  if (rc) return rc;
  return run_conv_b(d, 0, STAGE_PLAIN_B, 1, x, wnk, colscale, y, ws, ws_floats, EpNoneB{}, stream);
}
/* y = lrelu(conv(x, W) * colscale[n][k] + nw[0] * noise[n][oy][ox] + bias[k], slope) * gain: a StyledConv without upsampling in one
 * launch (stylegan2/model.py:241-279 ModulatedConv2d on pre-scaled activations, :250-252 demodulation, :282-294 NoiseInjection,
 * op/fused_act.py:30-37 FusedLeakyReLU) -- the output stage of the eight-phase kernel (csrc/conv_bf16_8ph.h).  colscale / noise / bias
 * may be NULL; FMI_ERR_UNSUPPORTED where that kernel does not apply (C % 64, K % 4, 8-byte aligned y, 16-byte colscale / bias). */
extern "C" int fmi_conv2d_fwd_act_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* colscale, const float* noise,
                                       const float* nw, const float* bias, float slope, float gain, uint16_t* y, void* stream) {
  if (noise && !nw) return FMI_ERR_BAD_ARG;
  if (bias && ((uintptr_t)bias & 15)) return FMI_ERR_UNSUPPORTED;
  int rc = conv2d_fwd_bf16_check(d, x, wnk, y);
  if (rc) return rc;
  return run_conv_b(d, 0, STAGE_ACT_B, 1, x, wnk, colscale, y, nullptr, 0, EpActB{noise, nw, bias, slope, gain, 1}, stream);
}
/* y = prelu(conv(x, W) * scale[k] + bias[k], slope[k]): the per-column output stage EpChanB of conv_bf16_kernel, for the eval-mode IR-SE
 * block (helpers.py:85-89 / :107-113 of the reference: conv1 + PReLU with slope; conv2 + BatchNorm and the shortcut's 1x1 convolution +
 * BatchNorm, :82-83 / :104-105, with scale / bias).  colsum: see include/fmi_hip.h. */
extern "C" int fmi_conv2d_fwd_chan_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* wnk, const float* scale, const float* bias,
                                        const float* slope, uint16_t* y, float* colsum, int64_t colsum_floats, void* stream) {
  int rc = check_desc_b(d);
  if (rc) return rc;
  if (!x || !wnk || !y) return FMI_ERR_BAD_ARG;
  const bool k3 = d->kh == 3 && d->kw == 3 && d->pad == 1, k1 = d->kh == 1 && d->kw == 1 && d->pad == 0;
  if (!(k3 || k1) || (d->stride != 1 && d->stride != 2) || d->C % 64 != 0 || d->K % 64 != 0) return FMI_ERR_UNSUPPORTED;
  if (colsum) {
    if ((int64_t)d->OH * d->OW < 128) return FMI_ERR_UNSUPPORTED;  // a 128-row tile would touch more than two samples
    if (colsum_floats < ceil_div64((int64_t)d->N * d->OH * d->OW, FMI_CHAN_COLSUM_ROWS) * 2 * d->K) return FMI_ERR_BAD_ARG;
  }
  if (d->x_cstride % 8 != 0 || d->y_cstride % 4 != 0 || !fmi_al16(x) || !fmi_al16(wnk) || ((uintptr_t)y & 7) || !fmi_al16(scale) ||
      !fmi_al16(bias) || !fmi_al16(slope) || !fmi_al16(colsum))
    return FMI_ERR_UNSUPPORTED;
  return run_conv_b(d, 0, STAGE_CHAN_B, 1, x, wnk, nullptr, y, nullptr, 0, EpChanB{scale, bias, slope, colsum}, stream);
}
/* The tile path of fmi_conv2d_grouped_fwd_bf16 (style_heads_bf16.hip, which has checked every argument): G convolutions as one launch
 * of conv_bf16_kernel with the grouped output stage, grid = (tiles of one group, G).  d->C / d->K are per group; x_off / w_off are the
 * element offsets between consecutive groups inside a pixel of x and between their weight packs.  A shared map (x_off == 0) arrives here
 * as ONE group of G*K columns: the stacked packs are its [G*K][taps][C] weight as they lie. */
int fmi_conv_bf16_grouped_tiles(const fmi_conv_desc* d, int G, int64_t x_off, int64_t w_off, const uint16_t* x, const uint16_t* wnk,
                                const float* bias, float slope, uint16_t* y, void* stream) {
  return run_conv_b(d, 0, STAGE_GROUP_B, G, x, wnk, nullptr, y, nullptr, 0, EpGroupB{bias, slope, x_off, w_off}, stream);
}
/* dx = adjoint of the convolution described by d applied to dy; wck = weights packed [C][kh*kw][K] */
extern "C" int fmi_conv2d_dgrad_bf16(const fmi_conv_desc* d, const uint16_t* dy, const uint16_t* wck, const float* colscale, uint16_t* dx,
                                     float* ws, int64_t ws_floats, void* stream) {
  int rc = check_desc_b(d);
  if (rc) return rc;
  if (!dy || !wck || !dx) return FMI_ERR_BAD_ARG;
  if (d->K % 32 != 0 || d->y_cstride % 8 != 0 || !fmi_al16(dy) || !fmi_al16(wck)) return FMI_ERR_UNSUPPORTED;
  if (d->stride > 2) return FMI_ERR_UNSUPPORTED;  // at most four sub-pixel phases per launch
  return run_conv_b(d, 1, STAGE_PLAIN_B, 1, dy, wck, colscale, dx, ws, ws_floats, EpNoneB{}, stream);
}
/* dx = a_in > 0 ? adjoint(dy) : 0 -- fmi_conv2d_dgrad_bf16 with the mask of the ReLU that produced the convolution's input in the output
 * stage (EpMaskB): the convolutions of a VGG16 block that read another convolution's activated map (modules/loss.py:33-52 of the
 * reference).  a_in has the geometry of dx.  3x3, stride 1, pad 1, C and K multiples of 64; the tile is the one the plain adjoint takes
 * for the shape, without the split reduction: no atomics, the same bits every run. */
extern "C" int fmi_conv2d_dgrad_relu_bf16(const fmi_conv_desc* d, const uint16_t* dy, const uint16_t* wck, const uint16_t* a_in, uint16_t* dx,
                                          void* stream) {
  int rc = check_desc_b(d);
  if (rc) return rc;
  if (!dy || !wck || !a_in || !dx) return FMI_ERR_BAD_ARG;
  if (d->kh != 3 || d->kw != 3 || d->pad != 1 || d->stride != 1 || d->C % 64 != 0 || d->K % 64 != 0) return FMI_ERR_UNSUPPORTED;
  if (d->x_cstride % 4 != 0 || d->y_cstride % 8 != 0 || !fmi_al16(dy) || !fmi_al16(wck) || !fmi_al16(a_in) || !fmi_al16(dx)) return FMI_ERR_UNSUPPORTED;
  return run_conv_b(d, 1, STAGE_MASK_B, 1, dy, wck, nullptr, dx, nullptr, 0, EpMaskB{a_in}, stream);
}


// ---------------------------------------------------------------------------------------------------------------------------
// weight packs: src fp32 [T][A][B] (the fp32 packs wf[tap][C][K] / wt[tap][K][C]) -> bf16 [B][T][A]
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pack_bta_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int T, int A, int B,
                                                            int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int a = (int)(i % A);
    const int64_t r = i / A;
    const int t = (int)(r % T), b = (int)(r / T);
    dst[i] = bf_round(src[((int64_t)t * A + a) * B + b]);
  }
}
extern "C" int fmi_pack_weight_bf16(const float* src_tab, uint16_t* dst_bta, int T, int A, int B, void* stream) {
  if (!src_tab || !dst_bta || T <= 0 || A <= 0 || B <= 0) return FMI_ERR_BAD_ARG;
  const int64_t total = (int64_t)T * A * B;
  hipLaunchKernelGGL(pack_bta_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, src_tab, dst_bta, T, A, B, total);
  return fmi_launch_status();
}
// ---------------------------------------------------------------------------------------------------------------------------
// weight gradient: dwf[tap][c][k] += sum over pixels x[pixel + tap][c] * dy[pixel][k]   (fp32 atomics across the pixel splits)
// ---------------------------------------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
struct WgArgsB {
  const bf16_t* x;
  const bf16_t* dy;
  float* dwf;
  ConvGeom g;  // forward geometry: anchors = output pixels, all kh*kw taps
  int Kout, ycs, Mrows, P, kchunk;
  int tiles, ksplit, xcd_splits;
};

// LDS image of one operand tile: [32-row group][64 pixels][32 rows] bf16 -- a wave instruction of the copy fills 16 pixels x 64
// bytes of one group, so a thread's copies share ONE pixel decode; a transposed read of four pixel rows is 256 contiguous bytes.
template <class T>
__global__ void __launch_bounds__(T::NT) wgrad_bf16_kernel(WgArgsB a, int tiles_n) {
  const float* const zchunk = fmi_zero_chunk_ptr();  // the zero chunk's address: read from the GOT ONCE (see fmi_zero_chunk_ptr)
  constexpr int BM = T::BM, BN = T::BN, BK = 64;
  constexpr int WPP = T::NT / 256;  // waves per 16-pixel block of the tile (8-wave tiles: two, each filling every other row group)
  constexpr int NGA = BM / 32 / WPP, NGB = BN / 32 / WPP;
  static_assert(NGA >= 1 && NGB >= 1, "every wave copies at least one group of each operand");
  constexpr int STAGE_B = (BM + BN) * BK * 2;  // bytes
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE_B];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  // Workgroup -> (pixel split, tile): the workgroups of ONE split share their pixel range (every tile re-reads it for its own rows /
  // columns), so a split is pinned to one XCD (linear id % 8 = XCD): its tiles stream through the range together and the XCD's L2
  // serves all re-reads.  With tiles fastest across ALL XCDs, FETCH_SIZE was 2 GB per launch for 134 MB of operands (5 TB/s of fabric
  // traffic at 0.4 ms).
  int lid, split;
  if (a.xcd_splits) {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int grp = idx / a.tiles;
    lid = idx - grp * a.tiles;
    split = grp * 8 + xcd;
    if (split >= a.ksplit) return;
  } else {
    lid = xcd_remap(blockIdx.x, gridDim.x);
    split = blockIdx.y;
  }
  const int tile_m = lid / tiles_n, tile_n = lid - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int wm = (wid / T::WN) * T::TM * 32, wn = (wid % T::WN) * T::TN * 32;
  const ConvGeom& g = a.g;
  const int k_begin = split * a.kchunk;
  int k_end = k_begin + a.kchunk;
  if (k_end > a.P) k_end = a.P;

  const int kr = 16 * (wid & 3) + (lane >> 2), cq = lane & 3, gsel = wid >> 2;
  // A copies: group j = rows m0 + 32 j .. +31 lie inside one tap (C % 32 == 0): wave-uniform tap, per-thread channel
  int a_dy[NGA], a_dx[NGA];
  int64_t a_off[NGA];
#pragma unroll
  for (int j = 0; j < NGA; ++j) {
    const int row = m0 + 32 * (j * WPP + gsel);
    const int t = (int)fdiv((uint32_t)row, g.dC);
    const int i = (int)fdiv((uint32_t)t, g.dntx), jx = t - i * g.ntx;
    a_dy[j] = row < a.Mrows ? g.dy0 + i : -0x20000000;
    a_dx[j] = g.dx0 + jx;
    a_off[j] = ((int64_t)a_dy[j] * g.IW + a_dx[j]) * g.cstride + (row - t * g.C) + 8 * cq;
  }
  int b_col[NGB];
#pragma unroll
  for (int j = 0; j < NGB; ++j) {
    const int col = n0 + 32 * (j * WPP + gsel) + 8 * cq;
    b_col[j] = col < a.Kout ? col : -1;
  }

  f32x16 acc[T::TM][T::TN];
#pragma unroll
  for (int i = 0; i < T::TM; ++i)
#pragma unroll
    for (int j = 0; j < T::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  auto glds16 = [&](const void* gp, uint32_t dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gp), "s"(dst)
                 : "memory");
  };
  auto issue = [&](int k0, int st) {
    const uint32_t sa = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)st * STAGE_B + (uint32_t)(wid & 3) * 1024u + (uint32_t)gsel * 4096u);
    const uint32_t sb = sa + BM * BK * 2;
    const int pix = k0 + kr;
    const bool pv = pix < k_end;
    const uint32_t n = fdiv((uint32_t)pix, g.dG);
    const uint32_t rem = (uint32_t)pix - n * (uint32_t)(g.GH * g.GW);
    const uint32_t gy = fdiv(rem, g.dGW);
    const uint32_t gx = rem - gy * (uint32_t)g.GW;
    const int iy0 = (int)gy * g.S, ix0 = (int)gx * g.S;
    const int64_t xb = ((int64_t)((int)n * g.IH + iy0) * g.IW + ix0) * g.cstride;
#pragma unroll
    for (int j = 0; j < NGA; ++j) {
      const bool ok = pv && (unsigned)(iy0 + a_dy[j]) < (unsigned)g.IH && (unsigned)(ix0 + a_dx[j]) < (unsigned)g.IW;
      const void* gp = ok ? (const void*)(a.x + xb + a_off[j]) : (const void*)zchunk;
      glds16(gp, sa + j * WPP * 4096);
    }
#pragma unroll
    for (int j = 0; j < NGB; ++j) {
      const bool ok = pv && b_col[j] >= 0;
      const void* gp = ok ? (const void*)(a.dy + (int64_t)pix * a.ycs + b_col[j]) : (const void*)zchunk;
      glds16(gp, sb + j * WPP * 4096);
    }
  };
  // transposed fragment reads: lane 4q+p of a 16-lane group addresses pixel row q, rows 4p..4p+3 of the group's 16
  const int i16 = lane & 15;
  const uint32_t lbase = (uint32_t)((8 * lh + (i16 >> 2)) * 64 + 32 * ((lane >> 4) & 1) + 8 * (i16 & 3));
  auto frag = [&](uint32_t img, int grp, int s) {
    typedef __attribute__((address_space(3))) s16x4* lp;
    const uint32_t ad = img + (uint32_t)grp * 4096u + lbase + (uint32_t)s * 1024u;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)ad);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(uintptr_t)(ad + 256u));
    union {
      s16x4 h[2];
      bf16x8 v;
    } u;
    u.h[0] = lo;
    u.h[1] = hi;
    return u.v;
  };
  auto compute = [&](int st) {
    const uint32_t sa = lds0 + (uint32_t)st * STAGE_B, sb = sa + BM * BK * 2;
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 fa[T::TM], fb[T::TN];
#pragma unroll
      for (int i = 0; i < T::TM; ++i) fa[i] = frag(sa, wm / 32 + i, s);
#pragma unroll
      for (int j = 0; j < T::TN; ++j) fb[j] = frag(sb, wn / 32 + j, s);
#pragma unroll
      for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  };
  const int nt = (k_end - k_begin + BK - 1) / BK;
  if (nt > 0) issue(k_begin, 0);
  int st = 0;
  for (int t = 0; t < nt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < nt) issue(k_begin + (t + 1) * BK, st ^ 1);
    compute(st);
    st ^= 1;
  }
#pragma unroll
  for (int i = 0; i < T::TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row >= a.Mrows) continue;
#pragma unroll
      for (int j = 0; j < T::TN; ++j) {
        const int col = n0 + wn + j * 32 + l31;
        if (col < a.Kout) atomicAdd(a.dwf + (int64_t)row * a.Kout + col, acc[i][j][r]);
      }
    }
  }
}

#include "wgrad_bf16_8ph.h"

/* dwf[tap][C][K] (fp32, the layout of fmi_conv2d_wgrad_f32) += x^T dy; caller zeroes dwf */
extern "C" int fmi_conv2d_wgrad_bf16(const fmi_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dwf, void* stream) {
  int rc = check_desc_b(d);
  if (rc) return rc;
  if (!x || !dy || !dwf) return FMI_ERR_BAD_ARG;
  if (d->C % 32 != 0 || d->K % 8 != 0 || d->x_cstride % 8 != 0 || d->y_cstride % 8 != 0 || !fmi_al16(x) || !fmi_al16(dy))
    return FMI_ERR_UNSUPPORTED;
  const WgradPlanInB in = wgrad_plan_in_b(d, 0);
  const ConvPlanB pl = wgrad_plan_b(in);
  if (pl.status) return pl.status;
  ConvGeom g = fwd_geom(d, d->N);  // vec and img_bs stay 0: the weight gradient reads neither
  g.dC = make_fastdiv(g.C);        // here: divides by C (output row -> tap), as in the fp32 family
  const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]);
  hipStream_t st = (hipStream_t)stream;
  // the two kernels take their own argument structs (and wgrad_bf16_kernel the column tile count beside it): their launch lines stay here
  if (tile_8p_b(pl.tile)) {
    const Wg8Args w{x, dy, dwf, g, d->K, d->y_cstride, in.Mrows, in.P, pl.kchunk, pl.tiles[0], pl.tiles_n, pl.ksplit};
    hipLaunchKernelGGL(wgrad_bf16_8ph_kernel, grid, dim3(512), 0, st, w);
    return fmi_launch_status();
  }
  const WgArgsB a{x, dy, dwf, g, d->K, d->y_cstride, in.Mrows, in.P, pl.kchunk, pl.tiles[0], pl.ksplit, pl.xcd_splits};
  const int bn = tile_bn_b(pl.tile);
  if (bn == 32) hipLaunchKernelGGL((wgrad_bf16_kernel<TB128x32>), grid, dim3(256), 0, st, a, pl.tiles_n);
  else if (bn == 64) hipLaunchKernelGGL((wgrad_bf16_kernel<TB128x64>), grid, dim3(256), 0, st, a, pl.tiles_n);
  else hipLaunchKernelGGL((wgrad_bf16_kernel<TB128x128>), grid, dim3(256), 0, st, a, pl.tiles_n);
  return fmi_launch_status();
}

#endif  // FMI_HOST_EMU
