// Which kernel a bf16 convolution runs on, as a pure host function: the tile, the tile counts, the split of the reduction and the grid of
// every launch of conv_bf16_kernel, the eight-phase kernel (conv_bf16_8ph.h) and the two weight-gradient kernels.  conv_bf16.hip fills the
// inputs, launches what comes back and decides nothing itself; fmi_conv2d_bf16_plan returns the same answer without a launch.  Plain C++
// (no HIP types): tests/test_host_conv_bf16_plan.py holds every threshold below against tests/golden/conv_bf16_plan.npz on a g++ build.
// Every threshold is a routing decision that a profile justified; the measured rates stay next to the numbers.
#pragma once
#include <stdint.h>

#include "../../include/fmi_hip.h"

// output stages (the `stage` argument of fmi_conv2d_bf16_plan)
enum ConvStageB {
  STAGE_PLAIN_B = 0,  // EpNoneB: plain store, per-sample column scale, split reduction
  STAGE_ACT_B = 1,    // EpActB switched on: the fused StyledConv output stage -- the eight-phase kernel has it, nothing else
  STAGE_CHAN_B = 2,   // EpChanB: per-column scale / bias / slope, column sums
  STAGE_GROUP_B = 3,  // EpGroupB: G convolutions, the group is the grid's y index
  STAGE_MASK_B = 4    // EpMaskB: the masked adjoint
};

// tile id = the code of fmi_debug_bf16_last_tile: 1000 BM + BN, plus 1000000 for the eight-phase kernel
constexpr int TILE_8P_B = 1000000;
constexpr int tile_id_b(int bm, int bn, bool eight = false) { return (eight ? TILE_8P_B : 0) + 1000 * bm + bn; }
constexpr bool tile_8p_b(int id) { return id >= TILE_8P_B; }
constexpr int tile_bm_b(int id) { return id % TILE_8P_B / 1000; }
constexpr int tile_bn_b(int id) { return id % 1000; }

struct ConvPlanInB {
  int stage, BK, N, groups, nph;    // N: output columns (of one group); groups: 1 except STAGE_GROUP_B; nph: 1 except a strided adjoint
  int M[4], K[4], taps[4], vec[4];  // per phase: rows, reduction length, taps, "the output takes 8-byte stores"
  bool colscale, colscale_al16;     // per-sample column scale present / 16-byte aligned
  bool split_ws;                    // a usable split workspace: present, aligned, ws_floats >= out_elems, out_elems % 4 == 0
  bool det;                         // reproducible mode (fmi_set_deterministic)
  int tile_mode;                    // fmi_debug_bf16_tile
};
struct ConvPlanB {  // of a forward / adjoint launch and of a weight gradient (there tiles[0] is the tile count and the tile is 128 x {32, 64, 128}
                    // of wgrad_bf16_kernel, or the eight-phase id of wgrad_bf16_8ph_kernel's 256 x 256)
  int status;       // FMI_OK or FMI_ERR_UNSUPPORTED; every other field is zero when refused
  int tile, tiles[4], tiles_n, ksplit;
  int kchunk, xcd_splits;  // weight gradient: pixels per split; the splits are dealt to the 8 XCDs in groups of 8
  unsigned grid[3];        // forward / adjoint: (tiles of the largest phase, phases or groups, splits)
};

static inline int64_t plan_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// forward and adjoint
static inline ConvPlanB conv_plan_b(const ConvPlanInB& in) {
  const int N = in.N, nph = in.nph, mode = in.tile_mode;
  int Mmax = 0, Kmax = 0;
  for (int p = 0; p < nph; ++p) {
    if (in.M[p] > Mmax) Mmax = in.M[p];
    if (in.K[p] > Kmax) Kmax = in.K[p];
  }
  auto wgs = [&](int bm, int bn) { return plan_ceil_div(Mmax, bm) * plan_ceil_div(N, bn) * nph * in.groups; };
  const bool act = in.stage == STAGE_ACT_B;
  ConvPlanB refused{};
  refused.status = FMI_ERR_UNSUPPORTED;
  int tile = 0;
  if (in.stage == STAGE_CHAN_B) {
    // both tiles have 128 rows in two 64-row wave blocks (the column sums' granularity); 64 output columns take the narrow one
    tile = tile_id_b(128, N <= 64 ? 64 : 128);
  } else if (in.stage == STAGE_GROUP_B) {
    // the plain table below with the groups counted into the workgroups of a candidate -- but NOT the same table: no eight-phase kernel, no
    // 128 x 32 / 128 x 64 tiles (at most 64 columns always take 64 x 64), no BK / tile-mode terms.  The differences are kept as they are.
    if (N > 128 && wgs(256, 256) >= 200) tile = tile_id_b(256, 256);
    else if (N > 64 && wgs(128, 128) >= 512) tile = tile_id_b(128, 128);
    else if (N > 64 && wgs(64, 128) >= 256) tile = tile_id_b(64, 128);
    else tile = tile_id_b(64, 64);
  } else {
    // the eight-phase kernel (conv_bf16_8ph.h): whole 64-deep reduction tiles, 8-byte output stores, no split reduction
    // (narrower outputs reach it only for its fused output stage: the UNet's 64-channel layers, half of the 128-column tile masked off.
    // With that stage on this kernel is taken whatever the tile count -- it is the only one that has the stage -- so a deep, small map at
    // a small batch runs on a handful of workgroups: a throughput compromise of the one-launch eval form, not a tuned choice.)
    bool ok8 = in.BK == 64 && mode != 1 && mode != 2 && N % 4 == 0 && (N > 64 || act);
    for (int p = 0; p < nph && ok8; ++p) ok8 = in.K[p] % 64 == 0 && in.taps[p] <= 32 && in.vec[p] && (!in.colscale || in.colscale_al16);
    if (act && !ok8) return refused;
    const bool wide = N > 128;
    if (ok8 && (mode == 8 || act || (wide ? wgs(256, 256) : wgs(512, 128)) >= 200)) {
      tile = wide ? tile_id_b(256, 256, true) : tile_id_b(512, 128, true);
    } else if (N <= 32) {
      tile = tile_id_b(128, 32);
    } else if (N <= 64) {
      tile = wgs(128, 64) >= 384 ? tile_id_b(128, 64) : tile_id_b(64, 64);
    } else {
      // measured (512 -> 512 at 64^2, 256 -> 256 at 128^2): 256x256 / 2 stages 870-990 TFLOP/s, 128x128 690-820, 256x256 with BK 32 and
      // four stages 780-900; for N = 128 the 256x128 tile loses to 128x128 (660 vs 690)
      if (in.BK == 64 && mode != 1 && N > 128 && wgs(256, 256) >= 200) tile = tile_id_b(256, 256);
      else if (wgs(128, 128) >= 512) tile = tile_id_b(128, 128);
      else if (wgs(64, 128) >= 256) tile = tile_id_b(64, 128);
      else tile = tile_id_b(64, 64);
    }
  }
  ConvPlanB pl{};
  pl.tile = tile;
  const int64_t tn = plan_ceil_div(N, tile_bn_b(tile));
  int64_t tmax = 0, tsum = 0;
  for (int p = 0; p < nph; ++p) {
    const int64_t t = plan_ceil_div(in.M[p], tile_bm_b(tile)) * tn;
    if (t > 0x7fffffffLL) return refused;
    pl.tiles[p] = (int)t;
    tsum += t;
    if (t > tmax) tmax = t;
  }
  // the masked adjoint: 64-deep reduction tiles and at least 64 output columns
  if (in.stage == STAGE_MASK_B && !tile_8p_b(tile) && !(in.BK == 64 && tile_bn_b(tile) >= 64)) return refused;
  // small feature maps with a deep reduction (the 4^2 .. 16^2 layers: 2 - 32 output tiles) split the reduction over workgroups; the plain
  // stage of conv_bf16_kernel only, and never in reproducible mode or under a per-sample column scale
  int64_t ks = 1;
  if (in.stage == STAGE_PLAIN_B && !tile_8p_b(tile) && in.split_ws && !in.colscale && !in.det && tsum < 128 && Kmax >= 1024) {
    ks = plan_ceil_div(256, tsum);
    if (ks > Kmax / 256) ks = Kmax / 256;
  }
  pl.tiles_n = (int)tn;
  pl.ksplit = (int)ks;
  pl.grid[0] = (unsigned)tmax;
  pl.grid[1] = (unsigned)(in.stage == STAGE_GROUP_B ? in.groups : nph);
  pl.grid[2] = (unsigned)ks;
  return pl;
}

// weight gradient
struct WgradPlanInB {
  int Mrows, Kout, P;  // rows = taps x input channels, output channels, pixels (the reduction)
  int64_t x_elems;     // N H W x_cstride: the eight-phase kernel addresses x with 32-bit offsets
  bool det;
  int tile_mode;
};
static inline ConvPlanB wgrad_plan_b(const WgradPlanInB& in) {
  ConvPlanB pl{};
  pl.grid[1] = pl.grid[2] = 1;
  const int64_t P = in.P;
  // the eight-phase kernel (wgrad_bf16_8ph.h): 256 x 256 tiles, one workgroup per CU -- for wide layers with a long pixel range
  const int64_t tm8 = plan_ceil_div(in.Mrows, 256), tn8 = plan_ceil_div(in.Kout, 256);
  const bool fits = in.Kout >= 256 && tn8 * 256 - in.Kout <= in.Kout / 8 && tm8 * 256 - in.Mrows <= in.Mrows / 8 && tm8 * tn8 <= 256 &&
                    P >= 4096 && (int64_t)in.Mrows < (1ll << 30) && in.x_elems < (1ll << 31);
  if (fits && !in.det && in.tile_mode != 1 && in.tile_mode != 2) {
    pl.tile = tile_id_b(256, 256, true);
    pl.tiles[0] = (int)(tm8 * tn8);
    pl.tiles_n = (int)tn8;
    int64_t ks = 256 / pl.tiles[0];
    if (ks > P / 1024) ks = P / 1024;
    if (ks < 1) ks = 1;
    pl.kchunk = (int)(plan_ceil_div(plan_ceil_div(P, ks), 64) * 64);
    pl.ksplit = (int)plan_ceil_div(P, pl.kchunk);
    pl.grid[0] = (unsigned)(pl.tiles[0] * pl.ksplit);
    return pl;
  }
  // the 8-wave 256x256 tile (the kernel takes it: WPP = 2) measured SLOWER here than 128x128 (574 vs 770 TFLOP/s at 512 -> 512, 64^2):
  // one workgroup per CU and a 16-accumulator atomic epilogue per split leave the CU idle between tiles
  const int bn = in.Kout <= 32 ? 32 : (in.Kout <= 64 ? 64 : 128);
  const int64_t tm = plan_ceil_div(in.Mrows, 128), tn = plan_ceil_div(in.Kout, bn);
  int64_t ksplit = 2048 / (tm * tn);
  const int64_t kmax = P / 1024;
  if (ksplit > kmax) ksplit = kmax;
  if (ksplit < 1) ksplit = 1;
  if (ksplit > 65535) ksplit = 65535;
  if (ksplit >= 6) ksplit = (ksplit + 4) / 8 * 8;  // splits are dealt to the 8 XCDs in groups of 8: keep the groups full
  if (in.det) ksplit = 1;                          // reproducible mode
  pl.kchunk = (int)(plan_ceil_div(plan_ceil_div(P, ksplit), 64) * 64);
  ksplit = plan_ceil_div(P, pl.kchunk);
  pl.tile = tile_id_b(128, bn);
  pl.tiles[0] = (int)(tm * tn);
  pl.tiles_n = (int)tn;
  pl.ksplit = (int)ksplit;
  pl.xcd_splits = ksplit >= 8 ? 1 : 0;
  const int64_t nwg = pl.xcd_splits ? tm * tn * plan_ceil_div(ksplit, 8) * 8 : tm * tn;
  if (nwg > 0x7fffffffLL) {
    pl = ConvPlanB{};
    pl.status = FMI_ERR_UNSUPPORTED;
    return pl;
  }
  pl.grid[0] = (unsigned)nwg;
  pl.grid[1] = pl.xcd_splits ? 1u : (unsigned)ksplit;
  return pl;
}
