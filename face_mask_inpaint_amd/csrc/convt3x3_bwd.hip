// Whole backward of  y = ConvTranspose2d(x1, W1) + ConvTranspose2d(x2, W2) + bias  (kernel 3, stride 2, padding 1, output_padding 1, NHWC
// fp32, 32 output channels) from ONE read of the gradient gy: the ResBlockDecoder pair whose forward is convt3x3.h.
//
// For input pixel (i, j) and tap (ky, kx) let G = gy[2i - 1 + ky][2j - 1 + kx][.] (zero outside the image).  Then
//     gx[i][j][c]     = sum over taps, o of  G[o] * W[tap][o][c]          (contraction over o: gy's channels are contiguous)
//     gW[tap][o][c]  += x[i][j][c] * G[o]                                  (contraction over pixels)
//     gb[o]           = sum of gy[.][o]
// with c running over the channels of x1 followed by those of x2.  A workgroup (four waves) stages the gy window (9 x 33 pixels) and the
// x tile (4 x 16 pixels, all channels) of one tile in LDS as fp32 and computes all five results from it with v_mfma_f32_16x16x32_bf16 on
// the exact three-way split (x6.h):
//   input gradient:  D[c][pixel] = W^T (A: ready piece chunks of the packs' wf3 images, from global memory) x G (B: 8 channels of a pixel).
//                    wave (ph, ch) = (two of the four tile rows, half of the channels).
//   weight gradient: D[c][o] = x^T (A) x G_tap (B), the contraction slot e of lane group kg standing for tile pixel ks * 32 + e * 4 + kg
//                    (any order serves, A and B use the same); the LDS pixel pitches make the eight 4-byte reads of a fragment
//                    conflict-free.  wave (oh, ch) = (16 of the 32 output channels, half of the input channels) keeps its 9 x CT/32
//                    accumulator blocks in registers across ALL tiles of the persistent workgroup.
// Each workgroup writes one row of partial sums (weight gradients + bias column sums of its tiles' own pixels, never the halo) and a
// finishing launch adds the rows in a fixed order: no atomics, nothing to zero, bit-identical from run to run in either mode.
#include "common.h"
#include "x6.h"

#ifndef FMI_HOST_EMU
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PB_TH = 4, PB_TW = 16;              // tile: 4 x 16 input pixels
constexpr int PB_WR = 2 * PB_TH + 1, PB_WC = 2 * PB_TW + 1;  // its gy window: 9 x 33 pixels
constexpr int PB_GP = 40;                         // window pixel pitch in floats: 2 * 40 = 16 (mod 64), see the weight gradient's reads
constexpr int PB_CB = 32;                         // output channels
constexpr int PB_MAX_ROWS = 512;

struct PairBwdArgs {
  const float *x1, *x2, *gy;
  const uint16_t *w1, *w2;  // wf3 images [3][9][32 / 8][cs][8]
  float *gx1, *gx2, *ws;
  int N, h, w, cs1, cs2;
  int tiles_x, tiles_y, ntiles;
};

__device__ __forceinline__ f32x4 mfma16_x6(const bf16x8_t (&a)[3], const bf16x8_t (&b)[3], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  return c;
}

// CT = cs1 + cs2 (64, 96 or 128); a wave's half of the channels is NB = CT / 32 blocks of 16
template <int CT>
__global__ void __launch_bounds__(256, CT <= 96 ? 2 : 1) convt_pair_bwd_kernel(PairBwdArgs a) {
  constexpr int NB = CT / 32, CH = CT / 2;
  constexpr int XP = CT + 16;  // x tile pixel pitch in floats: = 16 or 48 (mod 64)
  constexpr int NG4 = PB_WR * PB_WC * (PB_CB / 4), NX4 = PB_TH * PB_TW * (CT / 4);
  constexpr int GIT = (NG4 + 255) / 256, XIT = NX4 / 256;
  static_assert(NX4 % 256 == 0, "x tile copies evenly");
  __shared__ __attribute__((aligned(16))) float sg[PB_WR * PB_WC * PB_GP];
  __shared__ __attribute__((aligned(16))) float sx[PB_TH * PB_TW * XP];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int oh = wid & 1, ch = wid >> 1;
  const int H2 = 2 * a.h, W2 = 2 * a.w;

  f32x4 wacc[9][NB];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) wacc[t][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);  // channels 4 (tid & 7) .. + 3 of gy, over this thread's share of the tiles' own pixels

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int tx = tile % a.tiles_x, tyn = tile / a.tiles_x, ty = tyn % a.tiles_y, n = tyn / a.tiles_y;
    const int i0 = ty * PB_TH, j0 = tx * PB_TW;

    // ---- stage the gy window and the x tile (fp32); out-of-image cells are zero ----
    // (two rounds, x first: both in flight at once, next to the weight gradient's accumulators, do not fit the 256 registers of two
    // workgroups per CU)
    int st = tid;
    asm volatile("" : "+v"(st));  // the copy slots' index algebra is redone per tile: hoisted out of the loop it would live in scratch
    {
      float4 xv[XIT];
#pragma unroll
      for (int k = 0; k < XIT; ++k) {
        const int f = st + k * 256, px = f / (CT / 4), c = (f - px * (CT / 4)) * 4;
        const int i = i0 + (px >> 4), j = j0 + (px & 15);
        xv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < a.h && j < a.w) {
          const int64_t p = ((int64_t)n * a.h + i) * a.w + j;
          xv[k] = *reinterpret_cast<const float4*>(c < a.cs1 ? a.x1 + p * a.cs1 + c : a.x2 + p * a.cs2 + (c - a.cs1));
        }
      }
      __syncthreads();  // the previous tile's readers are done
#pragma unroll
      for (int k = 0; k < XIT; ++k) {
        const int f = st + k * 256, px = f / (CT / 4), c = (f - px * (CT / 4)) * 4;
        *reinterpret_cast<float4*>(sx + px * XP + c) = xv[k];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      float4 gv[GIT];
#pragma unroll
      for (int k = 0; k < GIT; ++k) {
        const int f = st + k * 256, px = f >> 3, q = f & 7;
        const int wr = px / PB_WC, wc = px - wr * PB_WC;
        const int R = 2 * i0 - 1 + wr, Cc = 2 * j0 - 1 + wc;
        gv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f < NG4 && R >= 0 && R < H2 && Cc >= 0 && Cc < W2)
          gv[k] = *reinterpret_cast<const float4*>(a.gy + (((int64_t)n * H2 + R) * W2 + Cc) * PB_CB + q * 4);
      }
#pragma unroll
      for (int k = 0; k < GIT; ++k) {
        const int f = st + k * 256, px = f >> 3, q = f & 7;
        if (f < NG4) {
          *reinterpret_cast<float4*>(sg + px * PB_GP + q * 4) = gv[k];
          const int wr = px / PB_WC, wc = px - wr * PB_WC;
          if (wr >= 1 && wc >= 1) {  // the tile's own output pixels (cells outside the image hold zeros)
            bsum.x += gv[k].x, bsum.y += gv[k].y, bsum.z += gv[k].z, bsum.w += gv[k].w;
          }
        }
      }
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);

    // ---- input gradient: wave (ph = oh, ch): tile rows 2 ph, 2 ph + 1 x channels ch * CH .. + CH ----
    {
      f32x4 dacc[2][NB];
#pragma unroll
      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) dacc[pb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap) {  // not unrolled: nothing here is indexed by the tap, and the registers belong to the weight gradient
        const int ky = tap / 3, kx = tap - ky * 3;
        bf16x8_t gb[2][3];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          const int r = 2 * oh + pb;
          const float* s = sg + ((2 * r + ky) * PB_WC + 2 * l15 + kx) * PB_GP + kg * 8;
          const float4 v0 = *reinterpret_cast<const float4*>(s), v1 = *reinterpret_cast<const float4*>(s + 4);
          const float f8[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          split3_bf16(f8, gb[pb]);
        }
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          const int c = ch * CH + cb * 16 + l15;
          const bool first = c < a.cs1;
          const uint16_t* wp = first ? a.w1 : a.w2;
          const int cs = first ? a.cs1 : a.cs2, cl = first ? c : c - a.cs1;
          bf16x8_t wa[3];
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)
            wa[pc] = *reinterpret_cast<const bf16x8_t*>(wp + ((int64_t)((pc * 9 + tap) * (PB_CB / 8) + kg) * cs + cl) * 8);
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) dacc[pb][cb] = mfma16_x6(wa, gb[pb], dacc[pb][cb]);
        }
      }
      // D[c = 4 kg + r][pixel = l15]
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const int i = i0 + 2 * oh + pb, j = j0 + l15;
        if (i < a.h && j < a.w) {
          const int64_t p = ((int64_t)n * a.h + i) * a.w + j;
#pragma unroll
          for (int cb = 0; cb < NB; ++cb) {
            const int c = ch * CH + cb * 16 + 4 * kg;
            const f32x4 v = dacc[pb][cb];
            float* dst = c < a.cs1 ? (a.gx1 ? a.gx1 + p * a.cs1 + c : nullptr) : (a.gx2 ? a.gx2 + p * a.cs2 + (c - a.cs1) : nullptr);
            if (dst) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
    }

    __builtin_amdgcn_sched_barrier(0);
    // ---- weight gradient: wave (oh, ch): output channels oh * 16 .. + 16 x channels ch * CH .. + CH, every tap ----
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t xa[NB][3];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        float f8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f8[e] = sx[(ks * 32 + e * 4 + kg) * XP + ch * CH + cb * 16 + l15];
        split3_bf16(f8, xa[cb]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        float f8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int r = 2 * ks + (e >> 2), c = (e & 3) * 4 + kg;
          f8[e] = sg[((2 * r + ky) * PB_WC + 2 * c + kx) * PB_GP + oh * 16 + l15];
        }
        bf16x8_t gb[3];
        split3_bf16(f8, gb);
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) wacc[tap][cb] = mfma16_x6(xa[cb], gb, wacc[tap][cb]);
        __builtin_amdgcn_sched_barrier(0);  // keep the next taps' reads from piling up in registers
      }
    }
  }

  // ---- this workgroup's row of partial sums: [9][32][CT] weight gradients (c = x1's channels, then x2's), then 32 bias sums ----
  constexpr int RW = 9 * PB_CB * CT + PB_CB;
  float* row = a.ws + (int64_t)blockIdx.x * RW;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {  // D[c = 4 kg + r][o = l15]
      const f32x4 v = wacc[tap][cb];
      *reinterpret_cast<float4*>(row + (tap * PB_CB + oh * 16 + l15) * CT + ch * CH + cb * 16 + 4 * kg) = make_float4(v[0], v[1], v[2], v[3]);
    }
  __syncthreads();
  float4* sb = reinterpret_cast<float4*>(sg);
  sb[tid] = bsum;
  __syncthreads();
  if (tid < PB_CB) {
    float s = 0.f;
    for (int k = 0; k < 32; ++k) s += sg[(k * 8 + (tid >> 2)) * 4 + (tid & 3)];
    row[9 * PB_CB * CT + tid] = s;
  }
}

// out[i] = sum over the rows of ws[rows][width] in a fixed order (the pattern of thin_sum_rows_kernel): 32 interleaved slices per value,
// each over its rows in four interleaved chains, then the slices one after the other.  Column (tap, o, c) goes to gw1 or gw2.
__global__ void __launch_bounds__(1024) convt_pair_sum_rows_kernel(const float* __restrict__ ws, float* __restrict__ gw1, float* __restrict__ gw2,
                                                                   float* __restrict__ gb, int rows, int width, int cs1, int cs2) {
  __shared__ float part[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + tx;
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < width) {
    int r = ty;
    for (; r + 96 < rows; r += 128) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s4[u] += ws[(int64_t)(r + 32 * u) * width + i];
    }
    for (int u = 0; r < rows; r += 32, ++u) s4[u] += ws[(int64_t)r * width + i];
  }
  part[ty][tx] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  __syncthreads();
  if (ty == 0 && i < width) {
    float t = 0.f;
#pragma unroll
    for (int l = 0; l < 32; ++l) t += part[l][tx];
    const int ct = cs1 + cs2, nw = 9 * PB_CB * ct;
    if (i < nw) {
      const int to = i / ct, c = i - to * ct;
      if (c < cs1) {
        if (gw1) gw1[to * cs1 + c] = t;
      } else if (gw2) gw2[to * cs2 + (c - cs1)] = t;
    } else if (gb) gb[i - nw] = t;
  }
}

template <int CT>
int pair_bwd_resident_grid() {
  static const int g = [] {
    int per_cu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, convt_pair_bwd_kernel<CT>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    (void)hipGetLastError();
    const int g = per_cu * cus;
    return g < PB_MAX_ROWS ? g : PB_MAX_ROWS;
  }();
  return g;
}

bool pair_bwd_ok(const fmi_conv_desc* d, int cs1, int cs2) {
  return d->kh == 3 && d->kw == 3 && d->stride == 2 && d->pad == 1 && d->dil <= 1 && d->pad_mode == 0 && d->C == PB_CB && d->x_cstride == PB_CB &&
         d->K == cs1 && d->y_cstride == cs1 && d->OH > 0 && d->OW > 0 && d->H == 2 * d->OH && d->W == 2 * d->OW && (cs1 == 32 || cs1 == 64) &&
         (cs2 == 32 || cs2 == 64) && (int64_t)d->N * d->H * d->W < (1ll << 31) / 2;
}
int64_t pair_bwd_tiles(const fmi_conv_desc* d) {
  return (int64_t)d->N * ((d->OH + PB_TH - 1) / PB_TH) * ((d->OW + PB_TW - 1) / PB_TW);
}
int pair_bwd_width(int cs1, int cs2) { return 9 * PB_CB * (cs1 + cs2) + PB_CB; }

}  // namespace
#endif

/* 1 if fmi_conv_transpose2d_pair_bwd_f32 takes this pair: d as for fmi_conv_transpose2d_pair_f32 (d->C = 32 output channels, d->K = cs1) */
extern "C" int fmi_conv_transpose2d_pair_bwd_supported(const fmi_conv_desc* d, int cs1, int cs2) {
#ifndef FMI_HOST_EMU
  return d && pair_bwd_ok(d, cs1, cs2) ? 1 : 0;
#else
  return 0;
#endif
}

extern "C" int fmi_conv_transpose2d_pair_bwd_ws_bytes(const fmi_conv_desc* d, int cs1, int cs2) {
#ifndef FMI_HOST_EMU
  if (!d || !pair_bwd_ok(d, cs1, cs2)) return 0;
  const int64_t nt = pair_bwd_tiles(d);
  return (int)(nt < PB_MAX_ROWS ? nt : PB_MAX_ROWS) * pair_bwd_width(cs1, cs2) * (int)sizeof(float);
#else
  return 0;
#endif
}

extern "C" int fmi_conv_transpose2d_pair_bwd_f32(const fmi_conv_desc* d, const float* x1, const float* x2, int cs2, const float* dy,
                                                 const void* wf3a, const void* wf3b, float* dx1, float* dx2, float* dwf1, float* dwf2,
                                                 float* dbias, void* ws, int64_t ws_bytes, void* stream) {
  if (!d || !x1 || !x2 || !dy || !wf3a || !wf3b || !ws || cs2 <= 0 || ws_bytes <= 0) return FMI_ERR_BAD_ARG;
#ifndef FMI_HOST_EMU
  const int cs1 = d->K;
  if (!pair_bwd_ok(d, cs1, cs2)) return FMI_ERR_UNSUPPORTED;
  const uintptr_t al = (uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)dy | (uintptr_t)wf3a | (uintptr_t)wf3b | (uintptr_t)dx1 | (uintptr_t)dx2 | (uintptr_t)ws;
  if (al & 15) return FMI_ERR_BAD_ARG;
  const int64_t nt = pair_bwd_tiles(d);
  const int width = pair_bwd_width(cs1, cs2);
  const int ct = cs1 + cs2;
  int64_t rows = ws_bytes / ((int64_t)width * (int64_t)sizeof(float));
  if (rows < 1) return FMI_ERR_BAD_ARG;
  int64_t grid = ct == 64 ? pair_bwd_resident_grid<64>() : (ct == 96 ? pair_bwd_resident_grid<96>() : pair_bwd_resident_grid<128>());
  if (grid > nt) grid = nt;
  if (grid > rows) return FMI_ERR_BAD_ARG;  // a workspace shorter than fmi_conv_transpose2d_pair_bwd_ws_bytes
  hipStream_t st = (hipStream_t)stream;
  PairBwdArgs a{x1, x2, dy, (const uint16_t*)wf3a, (const uint16_t*)wf3b, dx1, dx2, (float*)ws, d->N, d->OH, d->OW, cs1, cs2,
                (d->OW + PB_TW - 1) / PB_TW, (d->OH + PB_TH - 1) / PB_TH, (int)nt};
  if (ct == 64) hipLaunchKernelGGL((convt_pair_bwd_kernel<64>), dim3((unsigned)grid), dim3(256), 0, st, a);
  else if (ct == 96) hipLaunchKernelGGL((convt_pair_bwd_kernel<96>), dim3((unsigned)grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((convt_pair_bwd_kernel<128>), dim3((unsigned)grid), dim3(256), 0, st, a);
  if (dwf1 || dwf2 || dbias)
    hipLaunchKernelGGL(convt_pair_sum_rows_kernel, dim3((width + 31) / 32), dim3(1024), 0, st, (const float*)ws, dwf1, dwf2, dbias, (int)grid, width,
                       cs1, cs2);
  return fmi_launch_status();
#else
  return FMI_ERR_UNSUPPORTED;
#endif
}
