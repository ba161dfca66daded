// 3x3 stride-1 zero-padded convolution (forward and adjoint) on the LDS-DMA pipeline with TAP REUSE along x.
//
// The generic implicit GEMM (gemm_core.h) fetches one 16-channel operand tile per tap: the three taps of a kernel row read
// the SAME pixels shifted by one, so 2/3 of that traffic (and 2/3 of the barriers) are redundant.  Here a k-step is one
// (kernel row ky, 16-channel chunk): the A image holds BM + 2 consecutive pixels of the flattened [N][H][W] order, taken from
// image row y + ky - 1, and the three kx taps read fragment rows shifted by 0 / 1 / 2; three weight tiles ride along.  Per
// barrier a wave runs 3 x 8 x TM x TN MFMAs instead of 8 x TM x TN.
//   LDS row r  <->  anchor m0 - 1 + r (pixel (n, y, x) of the flattened order) read at image row y + ky - 1; rows outside the
//                   image are zero chunks.  Anchor i, tap kx reads LDS row i + kx = pixel x + kx - 1; where that wrapped
//                   around a row end (x = 0 with kx = 0, x = W-1 with kx = 2) the fragment is zeroed in registers.
//   adjoint    :    dx = conv(dy, flipped taps) with reduction over the conv's output channels: same kernel, tap index 8 - t.
//   pair       :    X2 = true (conv_pair.h): after the last (channel chunk, ky) step of x the loop goes on over 16-channel chunks of a second
//                   dense image x2 at the CENTRE tap only (the ResBlock's 1x1 bypass), with that convolution's own weight pack: one A image
//                   read at ky = 1, one weight tile, the kx = 1 fragments.  The single-source instantiations take C3Args / ConvEp as before.
#pragma once
#include "gemm_core.h"
#include "conv_pair.h"

#ifndef FMI_HOST_EMU
struct C3Args {
  const float* x;  // gathered image [N][H][W] pixel pitch cs, C reduction channels used
  const float* w;  // packed weights [9][C][Nout]
  int N, H, W, C, cs, Nout, flip;
  FastDiv dW, dHW;
  const uint16_t* w3;  // W3 kernels: the same weights as bf16 pieces [3][9][C / 8][Nout][8] (ConvWX3 in gemm_core.h)
};

struct C3Args2 : C3Args {  // the pair: second activation source and its 1x1 weight pack (fp32 [C2][Nout], pieces [3][C2 / 8][Nout][8])
  const float* x2;
  const float* w2;
  const uint16_t* w3b;
  int C2, cs2;
};

// W3: the weight tiles arrive as bf16 piece images ([3 kx][3 pieces][2 channel groups][BN] 16-byte chunks per stage) and are read as
// ready B fragments; only the activation fragments are split in registers.
// FL: blocked accumulation (a second accumulator set, flushed every 10 steps = 480 reduction elements), see conv_p3.h
template <class T, bool W3, bool FL = false, bool X2 = false>
__global__ void __launch_bounds__(256) conv3x3_dma_kernel(std::conditional_t<X2, C3Args2, C3Args> a, std::conditional_t<X2, ConvEp2, ConvEp> ep, int M,
                                                          int tiles_n, int ksplit, int it_chunk) {
  const float* const zchunk = fmi_zero_chunk_ptr();  // the zero chunk's address: read from the GOT ONCE (see fmi_zero_chunk_ptr)
  constexpr int BM = T::BM, BN = T::BN, BK = 16;
  constexpr int RA = ((BM + 2 + 15) / 16) * 16;  // rows of the A image (multiple of the 16 rows one wave instruction writes)
  constexpr int NIA = RA / 16;                   // wave instructions of an A image
  constexpr int NIB = W3 ? 9 * BN / 32 : 3 * BN / 16;  // wave instructions of the three B tiles ([3][16 k][BN] floats, or [3][3][2][BN] chunks)
  constexpr int NLA = (NIA + 3) / 4, NLB = (NIB + 3) / 4;
  constexpr int STAGE = RA * BK + (W3 ? 3 * 3 * BN * 8 : 3 * BK * BN);  // floats
  __shared__ __attribute__((aligned(1024))) float lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = lid / tiles_n, tile_n = lid - tile_m * tiles_n;
  const int zs = blockIdx.y;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int cchunks = a.C >> 4, nit1 = 3 * cchunks;
  int nit_all = nit1;
  if constexpr (X2) nit_all += a.C2 >> 4;
  const int it_begin = zs * it_chunk;
  int it_end = it_begin + it_chunk;
  if (it_end > nit_all) it_end = nit_all;
  const int wm = (wid / T::WN) * T::TM * 32, wn = (wid % T::WN) * T::TN * 32;
  const int HW = a.H * a.W;

  // A copy slots of this thread: wave instruction j*4 + wid covers LDS rows 16*(j*4+wid) .. +15, 4 lanes (k-quarters) per row
  int64_t abase[NLA], abase2[X2 ? NLA : 1];
  int ay[NLA];
#pragma unroll
  for (int j = 0; j < NLA; ++j) {
    const int r = (j * 4 + wid) * 16 + (lane >> 2);
    const int kq = ((lane & 3) ^ ((r >> 2) & 3)) * 4;
    const int an = m0 - 1 + r;
    ay[j] = -0x20000000;
    abase[j] = 0;
    if (an >= 0 && an < M && r < BM + 2) {
      const uint32_t n = fdiv((uint32_t)an, a.dHW);
      const uint32_t rem = (uint32_t)an - n * (uint32_t)HW;
      ay[j] = (int)fdiv(rem, a.dW);
      abase[j] = (int64_t)an * a.cs + kq;
      if constexpr (X2) abase2[j] = (int64_t)an * a.cs2 + kq;
    }
  }
  // B copy slots: chunk p of [3][16][BN/4]
  int boff[NLB], bkx[NLB];
#pragma unroll
  for (int j = 0; j < NLB; ++j) {
    const int p = (j * 4 + wid) * 64 + lane;
    if (W3) {  // chunk p of [3 kx][3 pieces][2 channel groups][BN]; boff = element offset inside a piece image, piece in the high bits of bkx
      const int per_tap = 3 * 2 * BN;
      const int kx = p / per_tap, q = p - kx * per_tap;
      const int piece = q / (2 * BN), r = q - piece * (2 * BN), kg = r / BN, n = r - kg * BN;
      bkx[j] = kx | (piece << 2);
      boff[j] = (n0 + n < a.Nout && kx < 3) ? (kg * a.Nout + n0 + n) * 8 : -1;
    } else {
      const int per_tap = 16 * (BN / 4);
      const int kx = p / per_tap, q = p - kx * per_tap;
      const int k = q / (BN / 4), n = (q - k * (BN / 4)) * 4;
      bkx[j] = kx;
      boff[j] = (n0 + n < a.Nout && kx < 3) ? k * a.Nout + n0 + n : -1;
    }
  }
  const int na_w = (NIA - wid + 3) / 4, nb_w = (NIB - wid + 3) / 4;  // instructions wave `wid` issues per stage
  // x-wrap masks of this lane's fragment rows
  bool xl[T::TM], xr[T::TM];
#pragma unroll
  for (int i = 0; i < T::TM; ++i) {
    const uint32_t an = (uint32_t)(m0 + wm + i * 32 + l31);
    const uint32_t rem = an - fdiv(an, a.dHW) * (uint32_t)HW;
    const uint32_t x = rem - fdiv(rem, a.dW) * (uint32_t)a.W;
    xl[i] = x == 0;
    xr[i] = x == (uint32_t)a.W - 1;
  }

  f32x16 acc[T::TM][T::TN];
#pragma unroll
  for (int i = 0; i < T::TM; ++i)
#pragma unroll
    for (int j = 0; j < T::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
  auto glds16 = [&](const float* g, uint32_t dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(dst)
                 : "memory");
  };
  auto issue = [&](int it, int st) {
    // channel chunk OUTER, kernel row INNER: the three kernel rows re-read one channel chunk of neighbouring image rows while it is still in
    // the XCD's L2 (with the kernel row outer every activation byte came three times from beyond L2)
    const int cc_ = it / 3, ky = it - 3 * cc_, c0 = cc_ * 16;  // wave-uniform
    const uint32_t sa = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(st * STAGE) * 4u + (uint32_t)wid * 1024u);  // + this wave's slot
    const uint32_t sb = sa + RA * BK * 4;
    if constexpr (X2) {
      if (it >= nit1) {  // wave-uniform: 16 channels of x2 at the centre tap
        const int c2 = (it - nit1) * 16;
#pragma unroll
        for (int j = 0; j < NLA; ++j) {
          if (j >= na_w) break;
          glds16(ay[j] >= 0 ? a.x2 + abase2[j] + c2 : zchunk, sa + (uint32_t)(j * 4096));
        }
#pragma unroll
        for (int j = 0; j < NLB; ++j) {
          if (j >= nb_w) break;
          if ((bkx[j] & 3) != 1) continue;  // only the kx = 1 tile is read back
          const float* g;
          if (W3)
            g = boff[j] >= 0 ? (const float*)(a.w3b + (int64_t)(bkx[j] >> 2) * a.C2 * a.Nout + (int64_t)(c2 >> 3) * a.Nout * 8 + boff[j]) : zchunk;
          else
            g = boff[j] >= 0 ? a.w2 + (int64_t)c2 * a.Nout + boff[j] : zchunk;
          glds16(g, sb + (uint32_t)(j * 4096));
        }
        return;
      }
    }
    const int64_t aoff = (int64_t)(ky - 1) * a.W * a.cs + c0;
#pragma unroll
    for (int j = 0; j < NLA; ++j) {
      if (j >= na_w) break;
      const bool ok = (unsigned)(ay[j] + ky - 1) < (unsigned)a.H;
      const float* g = ok ? a.x + abase[j] + aoff : zchunk;
      glds16(g, sa + (uint32_t)(j * 4096));
    }
#pragma unroll
    for (int j = 0; j < NLB; ++j) {
      if (j >= nb_w) break;
      const int tap = ky * 3 + (bkx[j] & 3);
      const float* g;
      if (W3)
        g = boff[j] >= 0 ? (const float*)(a.w3 + (int64_t)(bkx[j] >> 2) * 9 * a.C * a.Nout + (((int64_t)(a.flip ? 8 - tap : tap) * a.C + c0) >> 3) * a.Nout * 8 + boff[j])
                         : zchunk;
      else
        g = boff[j] >= 0 ? a.w + ((int64_t)(a.flip ? 8 - tap : tap) * a.C + c0) * a.Nout + boff[j] : zchunk;
      glds16(g, sb + (uint32_t)(j * 4096));
    }
  };
  auto compute = [&](int st, bool centre) {  // centre (wave-uniform, pair only): an x2 step, only the kx = 1 tile and fragments
    const float* sa = lds + st * STAGE;
    const float* sb = sa + RA * BK;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      if constexpr (X2) {
        if (centre && kx != 1) continue;
      }
      float fa[T::TM][8], fb[T::TN][8];
#pragma unroll
      for (int i = 0; i < T::TM; ++i) {
        const int r = wm + i * 32 + l31 + kx, sw = (r >> 2) & 3;
        float4 v0 = *reinterpret_cast<const float4*>(sa + r * 16 + ((2 * lh) ^ sw) * 4);
        float4 v1 = *reinterpret_cast<const float4*>(sa + r * 16 + ((2 * lh + 1) ^ sw) * 4);
        if ((kx == 0 && xl[i]) || (kx == 2 && xr[i])) v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
        fa[i][0] = v0.x, fa[i][1] = v0.y, fa[i][2] = v0.z, fa[i][3] = v0.w;
        fa[i][4] = v1.x, fa[i][5] = v1.y, fa[i][6] = v1.z, fa[i][7] = v1.w;
      }
      if (!W3) {
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
          for (int s = 0; s < 8; ++s) fb[j][s] = sb[(kx * 16 + 8 * lh + s) * BN + wn + j * 32 + l31];
      }
      bf16x8_t pa[T::TM][3], pb[T::TN][3];
#pragma unroll
      for (int i = 0; i < T::TM; ++i) split3_bf16(fa[i], pa[i]);
#pragma unroll
      for (int j = 0; j < T::TN; ++j) {
        if (W3) {
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)
            pb[j][pc] = *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const unsigned char*>(sb) + ((kx * 3 + pc) * 2 * BN + lh * BN + wn + j * 32 + l31) * 16);
        } else {
          split3_bf16(fb[j], pb[j]);
        }
      }
#pragma unroll
      for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j) acc[i][j] = mfma_x6(pa[i], pb[j], acc[i][j]);
    }
  };

  if (it_begin < it_end) issue(it_begin, 0);
  int st = 0, since = 0;
  f32x16 acc2[FL ? T::TM : 1][FL ? T::TN : 1];
  if constexpr (FL) {
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
      for (int j = 0; j < T::TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
  }
  for (int it = it_begin; it < it_end; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's copies of step `it` have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (it + 1 < it_end) issue(it + 1, st ^ 1);
    compute(st, X2 && it >= nit1);
    st ^= 1;
    if constexpr (FL) {
      if (++since == 10 || it + 1 == it_end) {
#pragma unroll
        for (int i = 0; i < T::TM; ++i)
#pragma unroll
          for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              acc2[i][j][r] += acc[i][j][r];
              acc[i][j][r] = 0.f;
            }
        since = 0;
      }
    }
  }
  if constexpr (FL) {
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
      for (int j = 0; j < T::TN; ++j) acc[i][j] = acc2[i][j];
  }
  store_tile<std::conditional_t<X2, ConvEp2, ConvEp>, T>(ep, acc, M, a.Nout, m0 + wm, n0 + wn, lh, l31);
}

using Tile128x64w = TileCfg<4, 1, 1, 2>;  // 128 x 64 with every wave spanning both column tiles: one activation split per 12 MFMAs

// reduction steps of a launch: 3 per 16-channel chunk of x, one per 16-channel chunk of the pair's x2
static int c3_steps(const C3Args& a) { return 3 * (a.C >> 4); }
static int c3_steps(const C3Args2& a) { return 3 * (a.C >> 4) + (a.C2 >> 4); }

// launches what the plan says (c3_plan_f of conv_f32_plan.h: eligibility is conv3x3_eligible_f there)
template <class ARGS, class EP>
static int launch_conv3x3(const ARGS& a, const EP& ep, int M, const LaunchPlanF& pl, hipStream_t st) {
  constexpr bool X2 = std::is_same<ARGS, C3Args2>::value;
  static_assert(std::is_same<EP, std::conditional_t<X2, ConvEp2, ConvEp>>::value, "the pair launches with ConvEp2");
  if (pl.status) return pl.status;
  const dim3 grid(pl.grid[0], pl.grid[1]);
  auto launch = [&](auto tile, auto w3) {
    using TILE = decltype(tile);
    constexpr bool W3 = decltype(w3)::value;
    if (pl.fl) {
      hipLaunchKernelGGL((conv3x3_dma_kernel<TILE, W3, true, X2>), grid, dim3(256), 0, st, a, ep, M, pl.tiles_n, pl.ksplit, pl.chunk);
      record_launch_f(W3 ? ROUTE_C3_W3_F : ROUTE_C3_F, false, true, TILE::BM, TILE::BN);
    } else {
      hipLaunchKernelGGL((conv3x3_dma_kernel<TILE, W3, false, X2>), grid, dim3(256), 0, st, a, ep, M, pl.tiles_n, pl.ksplit, pl.chunk);
      record_launch_f(W3 ? ROUTE_C3_W3_F : ROUTE_C3_F, false, false, TILE::BM, TILE::BN);
    }
  };
  if (pl.route == ROUTE_C3_W3_F) {
    launch(Tile128x64w{}, std::true_type{});
  } else {
    switch (pl.tile) {
      case tile_id_f(128, 32): launch(Tile128x32{}, std::false_type{}); break;
      case tile_id_f(128, 64): launch(Tile128x64{}, std::false_type{}); break;
      case tile_id_f(64, 64): launch(Tile64x64{}, std::false_type{}); break;
      case tile_id_f(128, 128): launch(Tile128x128{}, std::false_type{}); break;
      default: launch(Tile64x128{}, std::false_type{}); break;
    }
  }
  return fmi_launch_status();
}
#endif
