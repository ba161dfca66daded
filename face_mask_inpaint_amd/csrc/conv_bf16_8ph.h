// bf16 implicit-GEMM convolution, forward / adjoint, for the decoder's large layers: eight waves, every wave 128 pixels x 64 output
// channels of fp32 accumulators (128 registers), reduction tile 64, v_mfma_f32_16x16x32_bf16, the whole LDS as a two-tile ring
// that is filled in HALF-IMAGES several phases ahead of its use.  Included by conv_bf16.hip (loaders ConvKB / ConvWKB / ConvEpB).
//
// Schedule ("phases"; stylegan2/model.py:241-279 is what the launches compute, the schedule is this file's own):
//  * a reduction tile is four phases, one per 64 x 32 quadrant of the wave's accumulators: (i0,j0) (i0,j1) (i1,j1) (i1,j0) -- a Gray
//    path, each step replaces ONE operand: phase 0 reads the pixel half i0 (8 ds_read_b128) and the channel half j0 (4), phase 1 j1
//    (4), phase 2 i1 (8), phase 3 nothing; 16 MFMAs per phase.
//  * the LDS images are cut by WHEN they are read, not by which wave reads them: A0 = the i0 rows of every wave (read in phase 0
//    only), B0 = the j0 columns (phase 0), B1 = j1 (phase 1), A1 = i1 (phase 2).  Every half-image therefore has ONE reading phase,
//    and it can be refilled two phases later: phase 4u+0 fills B1 of tile u+1, 4u+1 A1 of u+1, 4u+2 A0 of u+2, 4u+3 B0 of u+2 --
//    each at least five phases before its read, four half-images (2 NA + 2 NB LDS-DMA instructions per thread) in flight behind
//    every counted s_waitcnt vmcnt, never vmcnt(0) inside the loop.
//  * two barriers per phase and the second four waves one barrier behind the first four: a SIMD's two waves alternate between
//    "LDS reads + DMA issue" and "16 MFMAs", so the matrix pipe of every SIMD always has one wave in its MFMA section.
//  * ordering: a half-image is waited for (each wave its own DMA instructions) in the phase BEFORE the one that reads it, so a
//    barrier lies between any wave's wait and any wave's read -- also across the one-barrier stagger; a half-image is refilled
//    at least two phases after its reading phase, so every wave's lgkmcnt(0) of those reads lies before the refill is issued.
//  * source-side swizzle (the DMA writes lane-linear): chunk column ^ ((row >> 1) & 7); the 16-lane groups of a ds_read_b128 of the
//    16x16x32 operand layout (rows l & 15, chunk l >> 4) then cover the 64 banks once.
//  * operands are passed (weights, pixels), so a lane's four accumulator registers are four consecutive CHANNELS of one pixel
//    (D row = 4 (l >> 4) + r, column = l & 15): 8-byte bf16 stores.
//  * one output tile per workgroup.  Persistent workgroups with the DMA streams running across output tiles were built and measured
//    slower (tools/bench_tools/experiments/conv_bf16_8ph_persistent.h: scalar-register pressure); what remains exposed is the
//    output stage and its store burst -- 6 % / 13 % / 24 % of the launch at 72 / 36 / 18 reduction tiles per output tile.  Starting
//    the first round of workgroups spread over 8 us (so that the rounds' store bursts do not coincide) measured 1-3 % slower.
#pragma once
#include <type_traits>

template <int WM_, int WN_>
struct Tile8P {
  static constexpr int WM = WM_, WN = WN_, BM = WM * 128, BN = WN * 64, NT = 512;
  static constexpr int NA = BM / 128, NB = BN / 128;                // LDS-DMA instructions per thread and half-image
  static constexpr int AH = BM / 2 * 128, BH = BN / 2 * 128;        // bytes of a half-image ([rows][64 bf16])
  static constexpr int STAGE = 2 * AH + 2 * BH;                     // A0 | A1 | B0 | B1
  static_assert(WM * WN == 8 && NB >= 1, "eight waves");
};
using T8P256x256 = Tile8P<2, 4>;
using T8P512x128 = Tile8P<4, 2>;  // the 128-channel layers; 2 x 80 KB = the whole LDS

typedef float f32x4v __attribute__((ext_vector_type(4)));

// fused output stage of a StyledConv (stylegan2/model.py:250-252 demodulation, :305-311 NoiseInjection, op/fused_act.py:30-37
// FusedLeakyReLU): y = lrelu(acc * colscale[n][c] + nw * noise[n][oy][ox] + bias[c]) * gain
struct EpActB {
  const float* noise;  // [N][OH][OW] or null
  const float* nw;     // one float (device)
  const float* bias;   // [Nout] or null
  float slope, gain;
  int on;
};

typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// CH: the output stage -- EpActB (plain when its `on` is 0) or EpMaskB (conv_bf16.hip: y = a > 0 ? acc : 0, the masked adjoint)
template <class T, class CH = EpActB>
__global__ void __launch_bounds__(512) conv_bf16_8ph_kernel(ConvSetB set, CH act) {
  constexpr bool MASK = std::is_same<CH, EpMaskB>::value;
  constexpr int BM = T::BM, BN = T::BN, NA = T::NA, NB = T::NB, AH = T::AH, BH = T::BH, STAGE = T::STAGE;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  if (lid >= set.ph[blockIdx.y].tiles) return;  // whole workgroup
  const ConvKB la = set.ph[blockIdx.y].la;
  const ConvWKB lb = set.ph[blockIdx.y].lb;
  const int K = set.ph[blockIdx.y].K, tiles_n = set.tiles_n;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / T::WN, wc = wid % T::WN, grp = wid >> 2;
  const int tile_m = lid / tiles_n, tile_n = lid - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- staging contexts: thread tid fills chunk position tid & 7 of local rows (tid >> 3) + 64 j of every half-image.
  // A section of the loop may hold about sixty instructions per wave (a wave issues one instruction every four cycles; the other
  // wave of the SIMD needs 16 MFMAs x 16 cycles), so everything per-row is decided here: a pixel row keeps its byte address and a
  // bit per tap ("this tap lies inside the image"), a weight row its byte address and an all-ones / zero mask for the tap offset.
  const ConvGeom& g = la.g;
  const int r0 = tid >> 3, kq = (((tid & 7) ^ ((tid >> 4) & 7)) << 3);
  const void* zp = fmi_chunk_zero;  // read from the GOT once and pinned in scalar registers (re-read per DMA it put an s_waitcnt
  asm volatile("" : "+s"(zp));      // lgkmcnt(0), which also waits for every LDS read in flight, in front of each issue)
  const unsigned char* pa[2][NA];
  uint32_t ma[2][NA];
  const unsigned char* pb[2][NB];
  uint32_t mb[2][NB];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const ConvKB::DCtx d = la.dprep(m0 + j * 128 + sub * 64 + r0, kq);
      pa[sub][j] = reinterpret_cast<const unsigned char*>(la.p + d.boff);
      uint32_t ym = 0, xm = 0;  // taps whose row / column lies inside the image
      for (int i = 0; i < g.nty; ++i)
        if ((unsigned)(d.ry + g.ystep * i) < (unsigned)g.IH) ym |= 1u << i;
      for (int jj = 0; jj < g.ntx; ++jj)
        if ((unsigned)(d.rx + g.xstep * jj) < (unsigned)g.IW) xm |= 1u << jj;
      uint32_t m = 0;
      for (int i = 0; i < g.nty; ++i)
        if (ym >> i & 1) m |= xm << (i * g.ntx);
      ma[sub][j] = m;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int lr = r0 + 64 * j;
      const ConvWKB::DCtx d = lb.dprep(n0 + (lr >> 5) * 64 + sub * 32 + (lr & 31), kq);
      pb[sub][j] = d.off >= 0 ? reinterpret_cast<const unsigned char*>(lb.p + d.off) : reinterpret_cast<const unsigned char*>(zp);
      mb[sub][j] = d.off >= 0 ? 0xffffffffu : 0u;
    }
  }

  // ---- the reduction tile the DMA streams are at (scalar): tap (ti, tj) of channel chunk ch, the order of ConvKB::tile.  Stepping
  // it is additions of six constants (bytes): next tap in a row, first tap of the next row, first tap of the next channel chunk.
  const int ntx = g.ntx, nty = g.nty;
  const int a_dx = g.xstep * g.cstride * 2, a_dy = (g.ystep * g.IW - (ntx - 1) * g.xstep) * g.cstride * 2;
  const int a_dc = 128 - ((nty - 1) * g.ystep * g.IW + (ntx - 1) * g.xstep) * g.cstride * 2;
  const int b_dx = g.kwstep * g.C * 2, b_dy = (g.khstep * g.kw - (ntx - 1) * g.kwstep) * g.C * 2;
  const int b_dc = 128 - ((nty - 1) * g.khstep * g.kw + (ntx - 1) * g.kwstep) * g.C * 2;
  struct TileAt {
    int ti, tj;
    uint32_t bit;  // 1 << tap
    int64_t ua;    // byte offset of the tap's pixel and the chunk's channels from a row's anchor
    uint32_t ub;   // byte offset of (tap, chunk) inside a packed weight row
  };
  auto advance = [&](TileAt& t) {
    if (++t.tj == ntx) {
      t.tj = 0;
      if (++t.ti == nty) t.ti = 0, t.bit = 1u, t.ua += a_dc, t.ub += (uint32_t)b_dc;
      else t.bit <<= 1, t.ua += a_dy, t.ub += (uint32_t)b_dy;
    } else {
      t.bit <<= 1, t.ua += a_dx, t.ub += (uint32_t)b_dx;
    }
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
  // one half-image = NA (NB) LDS-DMA instructions of this thread, 8 KB apart; M0 (the LDS base) is saved and restored once per group
  auto dma = [&](const void* const (&gp)[4], int n, uint32_t dst) {
    unsigned keep;
    if (n == 1)
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gp[0]), "s"(dst) : "memory");
    else if (n == 2)
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                   "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gp[0]), "v"(gp[1]), "s"(dst), "s"(dst + 8192) : "memory");
    else
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                   "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                   "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, off\n\t"
                   "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(gp[0]), "v"(gp[1]), "v"(gp[2]), "v"(gp[3]), "s"(dst), "s"(dst + 8192), "s"(dst + 16384), "s"(dst + 24576)
                   : "memory");
  };
  static_assert(NA == 2 || NA == 4, "dma() groups");
  static_assert(NB == 1 || NB == 2, "dma() groups");
  auto issueA = [&](int sub, const TileAt& t, int st) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(st * STAGE + sub * AH) + (uint32_t)wid * 1024u);
    const void* gp[4] = {zp, zp, zp, zp};
#pragma unroll
    for (int j = 0; j < NA; ++j) gp[j] = (ma[sub][j] & t.bit) ? (const void*)(pa[sub][j] + t.ua) : zp;
    dma(gp, NA, dst);
  };
  auto issueB = [&](int sub, const TileAt& t, int st) {
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(st * STAGE + 2 * AH + sub * BH) + (uint32_t)wid * 1024u);
    const void* gp[4] = {zp, zp, zp, zp};
#pragma unroll
    for (int j = 0; j < NB; ++j) gp[j] = (const void*)(pb[sub][j] + (t.ub & mb[sub][j]));
    dma(gp, NB, dst);
  };

  // ---- fragment read addresses (bytes from the start of a stage)
  const int l15 = lane & 15, c0 = (lane >> 4) ^ ((lane >> 1) & 7);
  const uint32_t a_off0 = (uint32_t)(wr * 8192 + l15 * 128 + c0 * 16), a_off1 = a_off0 ^ 64u;
  const uint32_t b_off0 = (uint32_t)(2 * AH + wc * 4096 + l15 * 128 + c0 * 16), b_off1 = b_off0 ^ 64u;

  f32x4v acc[2][2][4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[i][j][r][c] = f32x4v{0.f, 0.f, 0.f, 0.f};
  bf16x8 ax[4][2] = {}, bw0[2][2] = {}, bw1[2][2] = {};

  const int nt = K >> 6;  // reduction tiles (K % 64 == 0 is the host's condition for this kernel)
  auto read_a = [&](int st, int sub) {
    const unsigned char* p0 = lds + st * STAGE + sub * AH + a_off0;
    const unsigned char* p1 = lds + st * STAGE + sub * AH + a_off1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ax[r][0] = *reinterpret_cast<const bf16x8*>(p0 + r * 2048);
      ax[r][1] = *reinterpret_cast<const bf16x8*>(p1 + r * 2048);
    }
  };
  auto read_b = [&](int st, int sub, bf16x8 (&bw)[2][2]) {
    const unsigned char* p0 = lds + st * STAGE + sub * BH + b_off0;
    const unsigned char* p1 = lds + st * STAGE + sub * BH + b_off1;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      bw[c][0] = *reinterpret_cast<const bf16x8*>(p0 + c * 2048);
      bw[c][1] = *reinterpret_cast<const bf16x8*>(p1 + c * 2048);
    }
  };
  auto mfmas = [&](f32x4v (&d)[4][2], const bf16x8 (&bw)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) d[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[c][s], ax[r][s], d[r][c], 0, 0, 0);
  };
#define FMI_8P_MID()                                  \
  __builtin_amdgcn_s_barrier();                       \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  \
  __builtin_amdgcn_sched_barrier(0);                  \
  __builtin_amdgcn_s_setprio(1)
#define FMI_8P_END()                 \
  __builtin_amdgcn_s_setprio(0);     \
  __builtin_amdgcn_sched_barrier(0); \
  __builtin_amdgcn_s_barrier();      \
  asm volatile("" ::: "memory")
#define FMI_8P_WAIT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
  constexpr int WFULL = 2 * NA + 2 * NB;

  if (nt > 0) {
    // prologue: tile 0 whole, A0 / B0 of tile 1 -- the order the loop issues in
    TileAt t1{0, 0, 1u, 0, 0}, t2;  // t1: the tile phases 0 / 1 fill (u + 1), t2: the tile phases 2 / 3 fill (u + 2)
    t1.ub = (uint32_t)((g.kh0 * g.kw + g.kw0) * g.C) * 2u;
    issueA(0, t1, 0);
    issueB(0, t1, 0);
    issueB(1, t1, 0);
    issueA(1, t1, 0);
    advance(t1);
    if (nt > 1) {
      issueA(0, t1, 1);
      issueB(0, t1, 1);
      FMI_8P_WAIT(WFULL);
    } else {
      FMI_8P_WAIT(NA + NB);
    }
    t2 = t1;
    advance(t2);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (grp) __builtin_amdgcn_s_barrier();  // the second four waves run one barrier behind
    int st = 0;
    // ONE loop body for every reduction tile (two specialised copies -- steady state / last two tiles -- double the code for two
    // scalar branches per phase; a persistent variant with both copies made the allocator shuffle accumulators where they met)
    for (int u = 0; u < nt; ++u) {
      const bool n1 = u + 1 < nt, n2 = u + 2 < nt;
      // phase 0: quadrant (i0, j0)
      read_b(st, 0, bw0);
      __builtin_amdgcn_sched_barrier(0);
      read_a(st, 0);
      if (n1) {
        issueB(1, t1, st ^ 1);
        FMI_8P_WAIT(WFULL);
      } else {
        FMI_8P_WAIT(NA);
      }
      FMI_8P_MID();
      mfmas(acc[0][0], bw0);
      FMI_8P_END();
      // phase 1: (i0, j1)
      read_b(st, 1, bw1);
      if (n1) {
        issueA(1, t1, st ^ 1);
        FMI_8P_WAIT(WFULL);
      } else {
        FMI_8P_WAIT(0);
      }
      FMI_8P_MID();
      mfmas(acc[0][1], bw1);
      FMI_8P_END();
      // phase 2: (i1, j1)
      read_a(st, 1);
      if (n2) issueA(0, t2, st);
      FMI_8P_MID();
      mfmas(acc[1][1], bw1);
      FMI_8P_END();
      // phase 3: (i1, j0)
      t1 = t2;
      if (n2) {
        issueB(0, t2, st);
        advance(t2);
        FMI_8P_WAIT(WFULL);
      } else if (n1) {
        FMI_8P_WAIT(NA + NB);
      } else {
        FMI_8P_WAIT(0);
      }
      FMI_8P_MID();
      mfmas(acc[1][0], bw0);
      FMI_8P_END();
      st ^= 1;
    }
    if (!grp) __builtin_amdgcn_s_barrier();
  }
#undef FMI_8P_MID
#undef FMI_8P_END
#undef FMI_8P_WAIT

  // ---- output: lane = pixel (l & 15) of each 16-pixel group, four consecutive channels 4 (l >> 4) .. + 3 of each 16-channel group
  const ConvEpB ep = set.ph[blockIdx.y].ep;
  const int M = set.ph[blockIdx.y].M, N = set.N;
  const int cl = 4 * (lane >> 4);
  float nwv = 0.f;
  if constexpr (!MASK) nwv = (act.on && act.noise) ? act.nw[0] : 0.f;
  // a plain stride-1 convolution writes anchor row r to pixel r: no decode of (sample, y, x) per row -- eight of them per lane were a
  // quarter of this stage's instructions; the sample index is only needed for the per-sample column scale
  const bool linear = ep.OS == 1 && ep.GH == ep.OHt && ep.GW == ep.OWt;
  // the lane's four column groups are the same for all of its eight rows: bias once, the per-sample column scale once per sample
  // (a tile straddles a sample boundary at most once) -- reloaded per (row, group) they were 64 loads per lane
  float4 bsv[2][2], csv[2][2];
  int n_cached = -1;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = n0 + wc * 64 + j * 32 + c * 16 + cl;
      bsv[j][c] = make_float4(0.f, 0.f, 0.f, 0.f);
      csv[j][c] = make_float4(1.f, 1.f, 1.f, 1.f);
      if constexpr (!MASK)
        if (act.on && act.bias && col < N) bsv[j][c] = *reinterpret_cast<const float4*>(act.bias + col);
    }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wr * 128 + i * 64 + r * 16 + l15;
      if (row >= M) continue;
      int n_s = 0;
      int64_t pix;
      if (linear) {
        pix = row;
        if (ep.colscale) n_s = (int)fdiv((uint32_t)row, ep.dG);
      } else {
        pix = ep.row_pix(row, n_s);
      }
      const int64_t off = pix * ep.cstride;
      if (ep.colscale && n_s != n_cached) {
        n_cached = n_s;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int col = n0 + wc * 64 + j * 32 + c * 16 + cl;
            if (col < N) csv[j][c] = *reinterpret_cast<const float4*>(ep.colscale + (int64_t)n_s * ep.Nout + col);
          }
      }
      float nz = 0.f;
      if constexpr (!MASK)
        if (act.on && act.noise) nz = nwv * act.noise[pix];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int col = n0 + wc * 64 + j * 32 + c * 16 + cl;
          if (col >= N) continue;
          f32x4v a = acc[i][j][r][c];
          if (ep.colscale) a[0] *= csv[j][c].x, a[1] *= csv[j][c].y, a[2] *= csv[j][c].z, a[3] *= csv[j][c].w;
          if constexpr (MASK) {  // 8-byte load of the activated map beside the 8-byte store
            ep_mask4(*reinterpret_cast<const uint2*>(act.a + off + col), a);
          } else if (act.on) {
            const float bb[4] = {bsv[j][c].x, bsv[j][c].y, bsv[j][c].z, bsv[j][c].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = a[e] + nz + bb[e];
              a[e] = (v < 0.f ? v * act.slope : v) * act.gain;
            }
          }
          const bf16x2v lo = __builtin_convertvector((f32x2v){a[0], a[1]}, bf16x2v), hi = __builtin_convertvector((f32x2v){a[2], a[3]}, bf16x2v);
          uint2 v;
          v.x = *reinterpret_cast<const uint32_t*>(&lo);
          v.y = *reinterpret_cast<const uint32_t*>(&hi);
          *reinterpret_cast<uint2*>(ep.y + off + col) = v;
        }
      }
    }
  }
}
