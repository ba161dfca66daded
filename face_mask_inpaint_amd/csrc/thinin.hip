// fp32 convolutions with a THIN INPUT (C <= 4 channels: the image-facing first layers of the encoders, the discriminator and VGG16),
// 3x3 pad 1 or 1x1 pad 0, stride 1, K = 8 .. 64 output channels.  As a GEMM their reduction is 27 (or 3) long against a 16/32-deep
// MFMA k-step, so the matrix-core kernels mostly multiply padding; by shape they are streaming kernels (y or dy is the only large
// tensor) and 27 FMAs per output value fit under the memory time on the vector pipe.  Plain fp32 FMAs, no operand split.
//
// Entries: fmi_conv2d_thin_in_fwd_f32, fmi_conv2d_thin_in_wgrad_f32 (+ _ws_bytes) and, behind fmi_conv2d_thin_input_dgrad_f32 of
// thinconv.hip, the input gradient (described at its kernel below).  fmi_conv2d_thin_in_supported is the class the entries accept,
// fmi_conv2d_thin_in_routed the part of it (maps of TI_MIN_PIXELS and more) that the dispatch of conv.hip and functional.py sends here.
//
//   lane layout (forward and weight gradient): a thread owns a RUN of 4 consecutive pixels of one image row x one chunk of output
//   channels (8 in the forward, 4 in the weight gradient); the lanes of a pixel run are consecutive, so a wave's 16-byte accesses cover
//   whole rows of y / dy.
//   The 3 x 6 input pixels under a run are loaded once (one C-dword load per pixel) and serve all nine taps; cells outside the image
//   and pixels past the end of a ragged row are zeros in registers.
//   forward : the weights sit in LDS as [chunk][tap * C + c][8]: one pair of ds_read_b128 per (tap, c) serves the four pixels of the
//             run (32 FMAs).  One barrier after the weights are staged, none in the pixel loop.
//   wgrad   : persistent workgroups (one round of resident ones) stride over tiles of 256 / (K/4) runs; a thread keeps its
//             taps * C x 4 sums of x * dy and 4 sums of dy in registers over all its tiles.  At the end the lanes that share a channel
//             chunk are combined by shuffles, the four waves through LDS, and the workgroup stores ONE row of partial sums;
//             sum_parts_kernel adds the rows in a fixed order: no atomics, nothing to zero, the same bits in either mode.
#include "sum_parts.h"
#ifndef FMI_HOST_EMU

namespace {

constexpr int TI_RUN = 4;          // pixels of a run
constexpr int TI_MAX_ROWS = 1024;  // upper bound of the weight gradient's grid (= rows of its workspace)
// The library's own dispatch sends a shape of the class here from this many pixels (N H W) on: 8 x 128 x 128, the smallest map at which
// the kernels were timed against the generic path (profiles/thin_in.txt).  Smaller maps are launch-bound and keep the path they had.
constexpr int64_t TI_MIN_PIXELS = 1 << 17;

typedef float ti_f2 __attribute__((ext_vector_type(2)));

template <int C>
struct __attribute__((packed, aligned(4))) TiPix {
  float e[C];
};

// v or zero.  The value passes through an empty asm so that the load in front of it stays unconditional: as the operand of a plain select
// it is sunk into a branch of its own, and the loads of a window then wait for each other
__device__ __forceinline__ float ti_keep(float v, bool ok) {
  asm("" : "+v"(v));
  return ok ? v : 0.f;
}

template <int TAPS>
struct TiWin {
  static constexpr int HALO = TAPS == 9 ? 1 : 0, R = 2 * HALO + 1, WC = TI_RUN + 2 * HALO;
};

// the input window of the run that starts at column x0 of image row (n, yy): rows yy - HALO .., columns x0 - HALO ..; zeros outside
template <int C, int TAPS>
__device__ __forceinline__ void ti_load_window(const float* __restrict__ x, int n, int yy, int x0, int H, int W,
                                               float (&win)[TiWin<TAPS>::R][TiWin<TAPS>::WC][C]) {
  typedef TiWin<TAPS> TW;
#pragma unroll
  for (int r = 0; r < TW::R; ++r) {
    const int iy = yy + r - TW::HALO;
    const bool rok = (unsigned)iy < (unsigned)H;
    const float* rowp = x + (int64_t)(n * H + (rok ? iy : 0)) * W * C;
#pragma unroll
    for (int j = 0; j < TW::WC; ++j) {
      const int ix = x0 + j - TW::HALO;
      const bool ok = rok && (unsigned)ix < (unsigned)W;
      const TiPix<C> v = *reinterpret_cast<const TiPix<C>*>(rowp + (ok ? ix : 0) * C);  // always a load of an image cell
#pragma unroll
      for (int c = 0; c < C; ++c) win[r][j][c] = ti_keep(v.e[c], ok);
    }
  }
}

struct TiRun {
  int n, yy, x0, row;  // row = n * H + yy
};
__device__ __forceinline__ TiRun ti_run(int r, int runs, int H) {  // r = row * runs + run
  TiRun t;
  t.row = r / runs;
  t.x0 = (r - t.row * runs) * TI_RUN;
  t.n = t.row / H;
  t.yy = t.row - t.n * H;
  return t;
}

struct TiFwdArgs {
  const float* x;     // [N,H,W,C]
  const float* w;     // wf[TAPS][C][K]
  const float* bias;  // [K] or null
  const float* res;   // layout of y, or null
  float* y;           // [N,H,W,K]
  int H, W, K, act, cbits, runs;
  int64_t nruns;  // N * H * runs
};

// lane = (run slot, chunk c8 of 8 output channels); K/8 is padded to a power of two (the lanes of the padding idle)
template <int C, int TAPS>
__global__ void __launch_bounds__(256) thin_in_fwd_kernel(TiFwdArgs a) {
  typedef TiWin<TAPS> TW;
  constexpr int TC = TAPS * C, WSTR = 8 * (TC | 1);  // an odd number of 32-byte groups between chunks: the chunks' b128 reads miss each other's banks
  __shared__ __attribute__((aligned(16))) float wl[8 * WSTR];  // [c8][tap * C + c][8]
  __shared__ __attribute__((aligned(16))) float bl[64];
  for (int i = threadIdx.x; i < TC * a.K; i += 256) {
    const int tc = i / a.K, k = i - tc * a.K;
    wl[(k >> 3) * WSTR + tc * 8 + (k & 7)] = a.w[i];
  }
  if ((int)threadIdx.x < a.K) bl[threadIdx.x] = a.bias ? a.bias[threadIdx.x] : 0.f;
  __syncthreads();
  const int c8 = threadIdx.x & ((1 << a.cbits) - 1), slot = threadIdx.x >> a.cbits, spb = 256 >> a.cbits;
  if (8 * c8 >= a.K) return;
  const float* wp = wl + c8 * WSTR;
  for (int64_t rr = (int64_t)blockIdx.x * spb + slot; rr < a.nruns; rr += (int64_t)gridDim.x * spb) {
    // the weights are read from LDS again for every run: hoisted out of the loop they would take 8 * TAPS * C registers
    asm volatile("" ::: "memory");
    const TiRun t = ti_run((int)rr, a.runs, a.H);
    float win[TW::R][TW::WC][C];
    ti_load_window<C, TAPS>(a.x, t.n, t.yy, t.x0, a.H, a.W, win);
    ti_f2 acc[TI_RUN][4];
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] = ti_f2{0.f, 0.f};
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float4 w0 = *reinterpret_cast<const float4*>(wp + (tp * C + c) * 8), w1 = *reinterpret_cast<const float4*>(wp + (tp * C + c) * 8 + 4);
        const ti_f2 wv[4] = {ti_f2{w0.x, w0.y}, ti_f2{w0.z, w0.w}, ti_f2{w1.x, w1.y}, ti_f2{w1.z, w1.w}};
#pragma unroll
        for (int j = 0; j < TI_RUN; ++j) {
          const float xv = win[tp / 3][j + tp % 3][c];
          const ti_f2 xx = ti_f2{xv, xv};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][e] = __builtin_elementwise_fma(xx, wv[e], acc[j][e]);
        }
      }
    }
    // all four pixels are finished here: without this the sums of pixel j are sunk into the `ox < W` branch of its stores, one FMA block per
    // pixel, and every block reads the whole weight set again (or keeps it in registers)
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j) asm volatile("" : "+v"(acc[j][0]), "+v"(acc[j][1]), "+v"(acc[j][2]), "+v"(acc[j][3]));
    const float4 b0 = *reinterpret_cast<const float4*>(bl + 8 * c8), b1 = *reinterpret_cast<const float4*>(bl + 8 * c8 + 4);
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j) {
      const int ox = t.x0 + j;
      if (ox >= a.W) break;
      const int64_t o = ((int64_t)t.row * a.W + ox) * a.K + 8 * c8;
      float r[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[2 * e] = acc[j][e].x + bv[2 * e], r[2 * e + 1] = acc[j][e].y + bv[2 * e + 1];
      if (a.res) {
        const float4 r0 = *reinterpret_cast<const float4*>(a.res + o), r1 = *reinterpret_cast<const float4*>(a.res + o + 4);
        r[0] += r0.x, r[1] += r0.y, r[2] += r0.z, r[3] += r0.w, r[4] += r1.x, r[5] += r1.y, r[6] += r1.z, r[7] += r1.w;
      }
      if (a.act == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = tanhf(r[e]);
      } else if (a.act == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = fmaxf(r[e], 0.f);
      }
      *reinterpret_cast<float4*>(a.y + o) = make_float4(r[0], r[1], r[2], r[3]);
      *reinterpret_cast<float4*>(a.y + o + 4) = make_float4(r[4], r[5], r[6], r[7]);
    }
  }
}

struct TiWgradArgs {
  const float* x;   // [N,H,W,C]
  const float* dy;  // [N,H,W,K]
  float* ws_w;      // [gridDim.x][TAPS * C * K]
  float* ws_b;      // [gridDim.x][K]
  int H, W, K, kbits, runs, ntiles;
  int64_t nruns;
};

// lane = (run slot, chunk k4 of 4 output channels); K/4 is padded to a power of two.  A tile = 256 >> kbits consecutive runs.
template <int C, int TAPS>
__global__ void __launch_bounds__(256) thin_in_wgrad_kernel(TiWgradArgs a) {
  typedef TiWin<TAPS> TW;
  constexpr int TC = TAPS * C, NACC = 4 * TC + 4;
  __shared__ float red[4][NACC][16];  // [wave][value][k4]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int k4 = tid & ((1 << a.kbits) - 1), slot = tid >> a.kbits, rpw = 256 >> a.kbits;
  const bool chan_ok = 4 * k4 < a.K;
  ti_f2 acc[TC + 1][2];  // channel pairs (packed FMAs); [TC] = the bias gradient
#pragma unroll
  for (int i = 0; i <= TC; ++i) acc[i][0] = acc[i][1] = ti_f2{0.f, 0.f};
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t rr = (int64_t)tile * rpw + slot;
    if (rr >= a.nruns || !chan_ok) continue;
    const TiRun t = ti_run((int)rr, a.runs, a.H);
    float win[TW::R][TW::WC][C];
    ti_load_window<C, TAPS>(a.x, t.n, t.yy, t.x0, a.H, a.W, win);
    ti_f2 g[TI_RUN][2];
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j) {
      const int ox = t.x0 + j;
      const bool live = ox < a.W;  // a pixel past the end of a ragged row: the run's last live pixel is read again and counts as zero
      const float4 v = *reinterpret_cast<const float4*>(a.dy + ((int64_t)t.row * a.W + (live ? ox : a.W - 1)) * a.K + 4 * k4);
      g[j][0] = ti_f2{ti_keep(v.x, live), ti_keep(v.y, live)}, g[j][1] = ti_f2{ti_keep(v.z, live), ti_keep(v.w, live)};
      acc[TC][0] += g[j][0], acc[TC][1] += g[j][1];
    }
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < TI_RUN; ++j) {
          const float xv = win[tp / 3][j + tp % 3][c];
          const ti_f2 xx = ti_f2{xv, xv};
#pragma unroll
          for (int e = 0; e < 2; ++e) acc[tp * C + c][e] = __builtin_elementwise_fma(xx, g[j][e], acc[tp * C + c][e]);
        }
  }
  // over the wave's lanes that share k4, then the four waves through LDS; the workgroup's sums are one row of the workspace
  for (int m = 1 << a.kbits; m < 64; m <<= 1)
#pragma unroll
    for (int i = 0; i <= TC; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) acc[i][e] += ti_f2{__shfl_xor(acc[i][e].x, m, 64), __shfl_xor(acc[i][e].y, m, 64)};
  if (lane == k4) {
#pragma unroll
    for (int i = 0; i <= TC; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) red[wid][4 * i + 2 * e][k4] = acc[i][e].x, red[wid][4 * i + 2 * e + 1][k4] = acc[i][e].y;
  }
  __syncthreads();
  for (int i = tid; i < (NACC << a.kbits); i += 256) {
    const int v = i >> a.kbits, kk = i & ((1 << a.kbits) - 1);
    if (4 * kk >= a.K) continue;
    const float s = (red[0][v][kk] + red[1][v][kk]) + (red[2][v][kk] + red[3][v][kk]);
    const int tc = v >> 2, k = 4 * kk + (v & 3);
    if (tc < TC) a.ws_w[((int64_t)blockIdx.x * TC + tc) * a.K + k] = s;
    else a.ws_b[(int64_t)blockIdx.x * a.K + k] = s;
  }
}

// ---- input gradient: dx[q][c] = sum_{tap, k} dy[q + 1 - tap][k] wt[tap][k][c] ----------------------------------------------------
// lane = (run of 4 pixels, chunk k4 of 4 dy channels), K/4 a power of two; the TAPS x C x 4 weights of a lane's chunk stay in registers
// for the whole launch, so the pixel loop reads no weights at all.  A workgroup owns a band of DG_BH image rows x a segment of
// 4 * (256 / (K/4)) pixels and walks down the band: three dy rows (segment + a pixel each side, all K channels: 16 KB each) sit in a
// ring in LDS, written by 16-byte global loads that cover the rows contiguously; the row after them is loaded into registers before
// the FMAs of the current one and stored to the ring slot that falls free behind them.  A lane reads its 3 x 6 window cells as
// ds_read_b128 (the lanes of a run read 16 K/4 contiguous bytes), accumulates 4 pixels x C sums over its channels with packed FMAs,
// and the K/4 lanes of a run are combined by shuffles; lane 0 of the run stores the 4 pixels.
constexpr int DG_BH = 8;                 // rows of a band
constexpr int DG_ROW = 4096 + 2 * 64;    // floats of a ring slot: (4 * 256 / K4 + 2) pixels x K channels = 4096 + 2 K

// four consecutive dy channels as fp32: a 16-byte load of the fp32 map, or an 8-byte load of the bf16 map widened (exact)
__device__ __forceinline__ float4 ti_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ti_ld4(const uint16_t* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}

template <typename DT = float>  // element type of dy: float, or uint16_t = bf16 bits (fmi_conv2d_thin_input_dgrad_bf16); the ring, the FMAs and dx are fp32
struct TiDgradArgs {
  const DT* dy;     // [N,H,W,K]
  const float* wt;  // wt[TAPS][K][C]
  float* dx;        // [N,H,W,C]
  int H, W, K, kbits, segs, bands;
};

template <int C, typename DT = float>
__global__ void __launch_bounds__(256) thin_in_dgrad_kernel(TiDgradArgs<DT> a) {
  __shared__ __attribute__((aligned(16))) float ring[3][DG_ROW];
  const int tid = threadIdx.x;
  const int K4 = 1 << a.kbits, k4 = tid & (K4 - 1), rn = tid >> a.kbits, segw = TI_RUN * (256 >> a.kbits);
  int task = blockIdx.x;
  const int seg = task % a.segs;
  task /= a.segs;
  const int band = task % a.bands, n = task / a.bands;
  const int x0 = seg * segw, y0 = band * DG_BH, yend = min(y0 + DG_BH, a.H);
  const int nv = (segw + 2) << a.kbits;  // 16-byte chunks of a staged row
  constexpr int NL = 5;                  // (1024 + 2 K4 + 255) / 256
  // the chunks `tid + 256 l` of image row r (pixels x0 - 1 ..): zeros outside the image
  auto stage = [&](int r, float4 (&st)[NL]) {
    const bool rok = (unsigned)r < (unsigned)a.H;
    const DT* rowp = a.dy + (int64_t)(n * a.H + (rok ? r : 0)) * a.W * a.K;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int idx = tid + 256 * l, gx = x0 - 1 + (idx >> a.kbits);
      const bool ok = rok && idx < nv && (unsigned)gx < (unsigned)a.W;
      const float4 v = ti_ld4(rowp + (int64_t)(ok ? gx : 0) * a.K + 4 * (idx & (K4 - 1)));
      st[l] = make_float4(ti_keep(v.x, ok), ti_keep(v.y, ok), ti_keep(v.z, ok), ti_keep(v.w, ok));
    }
  };
  auto commit = [&](int r, const float4 (&st)[NL]) {
    float* slot = ring[(r + 3) % 3];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int idx = tid + 256 * l;
      if (idx < nv) *reinterpret_cast<float4*>(slot + 4 * idx) = st[l];
    }
  };
  {
    float4 s0[NL], s1[NL], s2[NL];
    stage(y0 - 1, s0);
    stage(y0, s1);
    stage(y0 + 1, s2);
    commit(y0 - 1, s0);
    commit(y0, s1);
    commit(y0 + 1, s2);
  }
  // wr[t][c] = wt[t][4 k4 .. 4 k4 + 3][c]
  ti_f2 wr[9][C][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* wp = a.wt + ((int64_t)t * a.K + 4 * k4) * C + c;
      wr[t][c][0] = ti_f2{wp[0], wp[C]}, wr[t][c][1] = ti_f2{wp[2 * C], wp[3 * C]};
    }
  __syncthreads();
  for (int y = y0; y < yend; ++y) {
    float4 nxt[NL];
    const bool more = y + 1 < yend;
    if (more) stage(y + 2, nxt);
    ti_f2 acc[TI_RUN][C];
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[j][c] = ti_f2{0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* rowl = ring[(y + r + 2) % 3] + ((TI_RUN * rn) << (a.kbits + 2)) + 4 * k4;  // image row y - 1 + r, window column 0
#pragma unroll
      for (int jj = 0; jj < TI_RUN + 2; ++jj) {
        const float4 g = *reinterpret_cast<const float4*>(rowl + (jj << (a.kbits + 2)));
        const ti_f2 g0 = ti_f2{g.x, g.y}, g1 = ti_f2{g.z, g.w};
#pragma unroll
        for (int j = 0; j < TI_RUN; ++j) {
          if (jj - j < 0 || jj - j > 2) continue;
          const int t = (2 - r) * 3 + (2 - (jj - j));  // pixel j sees window cell (r, jj) through tap (2 - r, 2 - (jj - j))
#pragma unroll
          for (int c = 0; c < C; ++c) {
            acc[j][c] = __builtin_elementwise_fma(g0, wr[t][c][0], acc[j][c]);
            acc[j][c] = __builtin_elementwise_fma(g1, wr[t][c][1], acc[j][c]);
          }
        }
      }
    }
    float tot[TI_RUN][C];
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) tot[j][c] = acc[j][c].x + acc[j][c].y;
    for (int m = 1; m < K4; m <<= 1)
#pragma unroll
      for (int j = 0; j < TI_RUN; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) tot[j][c] += __shfl_xor(tot[j][c], m, 64);
    if (k4 == 0) {
      const int ox0 = x0 + TI_RUN * rn;
      float* orow = a.dx + ((int64_t)(n * a.H + y) * a.W) * C;
#pragma unroll
      for (int j = 0; j < TI_RUN; ++j) {
        if (ox0 + j < a.W) {
          TiPix<C> o;
#pragma unroll
          for (int c = 0; c < C; ++c) o.e[c] = tot[j][c];
          *reinterpret_cast<TiPix<C>*>(orow + (int64_t)(ox0 + j) * C) = o;
        }
      }
    }
    if (!more) break;
    __syncthreads();  // every wave is done with row y - 1: its slot takes row y + 2
    commit(y + 2, nxt);
    __syncthreads();
  }
}

// 1x1: no halo, every lane reads its own 16 bytes of dy; pixels are taken flat (N H W), a run = 4 consecutive ones
template <int C, typename DT = float>
__global__ void __launch_bounds__(256) thin_in_dgrad_k1_kernel(TiDgradArgs<DT> a, int64_t npix) {
  const int tid = threadIdx.x;
  const int K4 = 1 << a.kbits, k4 = tid & (K4 - 1), rn = tid >> a.kbits, rpb = 256 >> a.kbits;
  ti_f2 wr[C][2];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* wp = a.wt + (int64_t)4 * k4 * C + c;
    wr[c][0] = ti_f2{wp[0], wp[C]}, wr[c][1] = ti_f2{wp[2 * C], wp[3 * C]};
  }
  const int64_t nruns = (npix + TI_RUN - 1) / TI_RUN;
  for (int64_t run = (int64_t)blockIdx.x * rpb + rn; run < nruns; run += (int64_t)gridDim.x * rpb) {
    float tot[TI_RUN][C];
#pragma unroll
    for (int j = 0; j < TI_RUN; ++j) {
      const int64_t p = run * TI_RUN + j;
      const bool live = p < npix;
      const float4 g = ti_ld4(a.dy + (live ? p : npix - 1) * a.K + 4 * k4);
      const ti_f2 g0 = ti_f2{ti_keep(g.x, live), ti_keep(g.y, live)}, g1 = ti_f2{ti_keep(g.z, live), ti_keep(g.w, live)};
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const ti_f2 s = __builtin_elementwise_fma(g1, wr[c][1], g0 * wr[c][0]);
        tot[j][c] = s.x + s.y;
      }
    }
    for (int m = 1; m < K4; m <<= 1)
#pragma unroll
      for (int j = 0; j < TI_RUN; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) tot[j][c] += __shfl_xor(tot[j][c], m, 64);
    if (k4 == 0) {
#pragma unroll
      for (int j = 0; j < TI_RUN; ++j) {
        const int64_t p = run * TI_RUN + j;
        if (p < npix) {
          TiPix<C> o;
#pragma unroll
          for (int c = 0; c < C; ++c) o.e[c] = tot[j][c];
          *reinterpret_cast<TiPix<C>*>(a.dx + p * C) = o;
        }
      }
    }
  }
}

template <typename F>
int ti_resident_grid(F kernel) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  (void)hipGetLastError();
  return per_cu * cus;
}
template <int C, int TAPS>
int ti_wgrad_resident_grid() {
  static const int g = ti_resident_grid(thin_in_wgrad_kernel<C, TAPS>);
  return g;
}

bool ti_ok(const fmi_conv_desc* d) {
  const bool k3 = d->kh == 3 && d->kw == 3 && d->pad == 1, k1 = d->kh == 1 && d->kw == 1 && d->pad == 0;
  return d->N > 0 && d->H > 0 && d->W > 0 && d->C >= 1 && d->C <= 4 && d->x_cstride == d->C && d->K % 8 == 0 && d->K >= 8 && d->K <= 64 &&
         d->y_cstride == d->K && (k3 || k1) && d->stride == 1 && d->dil <= 1 && d->pad_mode == 0 && d->OH == d->H && d->OW == d->W &&
         (int64_t)d->N * d->H * d->W < (1ll << 31);
}
bool ti_routed(const fmi_conv_desc* d) { return ti_ok(d) && (int64_t)d->N * d->H * d->W >= TI_MIN_PIXELS; }
int ti_taps(const fmi_conv_desc* d) { return d->kh * d->kw; }
int ti_pow2_bits(int chunks) {  // chunks padded to a power of two >= 2
  int b = 1;
  while ((1 << b) < chunks) ++b;
  return b;
}
int64_t ti_nruns(const fmi_conv_desc* d) { return (int64_t)d->N * d->H * ((d->W + TI_RUN - 1) / TI_RUN); }
int64_t ti_wgrad_tiles(const fmi_conv_desc* d) { return ceil_div64(ti_nruns(d), 256 >> ti_pow2_bits(d->K / 4)); }
int ti_wgrad_width(const fmi_conv_desc* d) { return ti_taps(d) * d->C * d->K + d->K; }

}  // namespace

#define TI_DISPATCH(CALL)                                  \
  switch (d->C * 2 + (ti_taps(d) == 9 ? 1 : 0)) {          \
    case 2: CALL(1, 1); break;                             \
    case 3: CALL(1, 9); break;                             \
    case 4: CALL(2, 1); break;                             \
    case 5: CALL(2, 9); break;                             \
    case 6: CALL(3, 1); break;                             \
    case 7: CALL(3, 9); break;                             \
    case 8: CALL(4, 1); break;                             \
    default: CALL(4, 9); break;                            \
  }

extern "C" int fmi_conv2d_thin_in_supported(const fmi_conv_desc* d) { return d && ti_ok(d) ? 1 : 0; }
extern "C" int fmi_conv2d_thin_in_routed(const fmi_conv_desc* d) { return d && ti_routed(d) ? 1 : 0; }

extern "C" int fmi_conv2d_thin_in_fwd_f32(const fmi_conv_desc* d, const float* x, const float* wf, const float* bias, const float* residual,
                                          float* y, int act, void* stream) {
  if (!d || !x || !wf || !y || act < 0 || act > 2) return FMI_ERR_BAD_ARG;
  if (!ti_ok(d)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)x | (uintptr_t)wf | (uintptr_t)bias) & 3) || !fmi_al16(y) || !fmi_al16(residual)) return FMI_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  TiFwdArgs a{x, wf, bias, residual, y, d->H, d->W, d->K, act, ti_pow2_bits(d->K / 8), (d->W + TI_RUN - 1) / TI_RUN, ti_nruns(d)};
  const int grid = fmi_bw_grid(a.nruns << a.cbits, 256);
#define TI_FWD(CC, TT) hipLaunchKernelGGL((thin_in_fwd_kernel<CC, TT>), dim3(grid), dim3(256), 0, st, a)
  TI_DISPATCH(TI_FWD)
#undef TI_FWD
  return fmi_launch_status();
}

extern "C" int fmi_conv2d_thin_in_wgrad_ws_bytes(const fmi_conv_desc* d) {
  if (!d || !ti_ok(d)) return 0;
  const int64_t nt = ti_wgrad_tiles(d);
  return (int)(nt < TI_MAX_ROWS ? nt : TI_MAX_ROWS) * ti_wgrad_width(d) * (int)sizeof(float);
}

extern "C" int fmi_conv2d_thin_in_wgrad_f32(const fmi_conv_desc* d, const float* x, const float* dy, float* dwf, float* dbias, void* ws,
                                            int64_t ws_bytes, void* stream) {
  if (!d || !x || !dy || !dwf || !ws || ws_bytes <= 0) return FMI_ERR_BAD_ARG;
  if ((((uintptr_t)dwf | (uintptr_t)dbias) & 3) || !fmi_al16(ws)) return FMI_ERR_BAD_ARG;
  if (!ti_ok(d)) return FMI_ERR_UNSUPPORTED;
  if (((uintptr_t)x & 3) || !fmi_al16(dy)) return FMI_ERR_UNSUPPORTED;
  const int width = ti_wgrad_width(d), nw = width - d->K;
  const int64_t rows = ws_bytes / ((int64_t)width * (int64_t)sizeof(float)), nt = ti_wgrad_tiles(d);
  if (rows < 1) return FMI_ERR_BAD_ARG;  // shorter than one row; fewer rows than workgroups only lower the grid
  int64_t grid = TI_MAX_ROWS;
#define TI_RES(CC, TT) grid = ti_wgrad_resident_grid<CC, TT>()
  TI_DISPATCH(TI_RES)
#undef TI_RES
  if (grid > TI_MAX_ROWS) grid = TI_MAX_ROWS;
  if (grid > nt) grid = nt;
  if (grid > rows) grid = rows;
  hipStream_t st = (hipStream_t)stream;
  float* wsf = (float*)ws;
  TiWgradArgs a{x, dy, wsf, wsf + grid * nw, d->H, d->W, d->K, ti_pow2_bits(d->K / 4), (d->W + TI_RUN - 1) / TI_RUN, (int)nt, ti_nruns(d)};
#define TI_WG(CC, TT) hipLaunchKernelGGL((thin_in_wgrad_kernel<CC, TT>), dim3((unsigned)grid), dim3(256), 0, st, a)
  TI_DISPATCH(TI_WG)
#undef TI_WG
  launch_sum_parts<float>(a.ws_w, dwf, (int)grid, nw, 1, st);
  if (dbias) launch_sum_parts<float>(a.ws_b, dbias, (int)grid, d->K, 1, st);
  return fmi_launch_status();
}

// The streaming input gradient of a shape the caller has checked (ti_ok, K/4 a power of two, alignment): 1x1 flat over the pixels, 3x3 by
// bands and segments.
template <typename DT>
static int ti_dgrad_launch(const fmi_conv_desc* d, const DT* dy, const float* wt, float* dx, hipStream_t st) {
  const int kbits = ti_pow2_bits(d->K / 4), segw = TI_RUN * (256 >> kbits);
  TiDgradArgs<DT> a{dy, wt, dx, d->H, d->W, d->K, kbits, (d->W + segw - 1) / segw, (d->H + DG_BH - 1) / DG_BH};
  if (ti_taps(d) == 1) {
    const int64_t npix = (int64_t)d->N * d->H * d->W;
    const int grid = fmi_bw_grid(((npix + TI_RUN - 1) / TI_RUN) << kbits, 256);
    switch (d->C) {
      case 1: hipLaunchKernelGGL((thin_in_dgrad_k1_kernel<1, DT>), dim3(grid), dim3(256), 0, st, a, npix); break;
      case 2: hipLaunchKernelGGL((thin_in_dgrad_k1_kernel<2, DT>), dim3(grid), dim3(256), 0, st, a, npix); break;
      case 3: hipLaunchKernelGGL((thin_in_dgrad_k1_kernel<3, DT>), dim3(grid), dim3(256), 0, st, a, npix); break;
      default: hipLaunchKernelGGL((thin_in_dgrad_k1_kernel<4, DT>), dim3(grid), dim3(256), 0, st, a, npix); break;
    }
    return fmi_launch_status();
  }
  const int64_t tasks = (int64_t)d->N * a.bands * a.segs;  // < 2^31: fewer than pixels
  switch (d->C) {
    case 1: hipLaunchKernelGGL((thin_in_dgrad_kernel<1, DT>), dim3((unsigned)tasks), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((thin_in_dgrad_kernel<2, DT>), dim3((unsigned)tasks), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL((thin_in_dgrad_kernel<3, DT>), dim3((unsigned)tasks), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((thin_in_dgrad_kernel<4, DT>), dim3((unsigned)tasks), dim3(256), 0, st, a); break;
  }
  return fmi_launch_status();
}

// The streaming form of fmi_conv2d_thin_input_dgrad_f32 (thinconv.hip calls it first): FMI_ERR_UNSUPPORTED for what it leaves to the
// kernels there -- 3x3 maps below TI_MIN_PIXELS among them; the 1x1 form has no other kernel behind that entry and is taken at any
// size.  dy rows 16-byte aligned, dx 4-byte aligned, K/4 a power of two.
int fmi_thin_in_dgrad_try(const fmi_conv_desc* d, const float* dy, const float* wt, float* dx, void* stream) {
  const int k4 = d->K / 4;
  if (!ti_ok(d) || (k4 & (k4 - 1)) || !fmi_al16(dy) || (((uintptr_t)wt | (uintptr_t)dx) & 3)) return FMI_ERR_UNSUPPORTED;
  if (ti_taps(d) == 9 && !ti_routed(d)) return FMI_ERR_UNSUPPORTED;
  return ti_dgrad_launch<float>(d, dy, wt, dx, (hipStream_t)stream);
}

/* The same adjoint reading a bf16 gradient (VGG16's first layer behind the bf16 trunk of VGGLoss, modules/loss.py:33-52 of the reference):
 * dy16 [N,H,W,K] bf16 is widened as it is staged, the FMAs and dx [N,H,W,C<=4] are fp32.  The whole class of the streaming kernels
 * (fmi_conv2d_thin_in_supported with K/4 a power of two), at ANY map size: there is no other bf16-reading kernel behind it. */
extern "C" int fmi_conv2d_thin_input_dgrad_bf16(const fmi_conv_desc* d, const uint16_t* dy16, const float* wt, float* dx, void* stream) {
  if (!d || !dy16 || !wt || !dx) return FMI_ERR_BAD_ARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->pad < 0 ||
      d->OH != (d->H + 2 * d->pad - d->kh) / d->stride + 1 || d->OW != (d->W + 2 * d->pad - d->kw) / d->stride + 1)
    return FMI_ERR_BAD_ARG;
  const int k4 = d->K / 4;
  if (!ti_ok(d) || (k4 & (k4 - 1)) || !fmi_al16(dy16) || (((uintptr_t)wt | (uintptr_t)dx) & 3)) return FMI_ERR_UNSUPPORTED;
  return ti_dgrad_launch<uint16_t>(d, dy16, wt, dx, (hipStream_t)stream);
}

#endif  // FMI_HOST_EMU
