// Fused self-attention forward for the PICNet attention blocks (example_guided_att.py:21-33, base_function.py:420-437):
//      A = softmax_j(q_i . q_j)   (queries = keys, no scaling)      O = A V        V = [V1 | V2] along channels
// in exact fp32 on the matrix cores, flash style: the [T x T] map (1 GiB per image at T = 16384) is never formed.
//
// MI355X mapping of the forward, attn_fwd_x6_kernel (the backward kernels are described where they stand)
//  * one workgroup = NW waves (2, 4 or 8: fmi_attention_fwd_waves) = NW x 32 queries; each wave owns 32 queries, ONE PER LANE COLUMN:
//    the score tile is computed transposed, S^T[key][query] = K Q^T (A = K tile from LDS, B = the wave's Q fragment held in registers
//    for the whole kernel), so a lane holds 16 keys of its own query.  Row max / row sum are then in-lane reductions plus one
//    exchange with lane^32, and the exponentiated tile is ALREADY the B operand of the second product
//    O^T[c][query] += V^T[c][key] P^T[key][query] (k-index permuted identically on both operands): P never touches LDS.
//  * every product runs on the bf16 matrix pipe: six bf16 MFMAs of K = 16 on exact three-way splits of the fp32 operands (x6.h).  The
//    Q pieces stay in registers, P is cut in registers, the K / V pieces lie in LDS.
//  * O^T accumulators: C/32 tiles x 16 registers per lane (128 for 256 channels); one workgroup per CU, so a wave may use the
//    512-register budget (launch_bounds(NW * 64, 1)).
//  * a stage is the three bf16 piece images of 32 keys' K and V rows, double buffered in dynamic LDS (opted in: up to 82 KB), one barrier
//    per tile.  The two- and four-wave forms cut the pieces on the way from the staging registers into LDS (the loads of tile t+1 are
//    issued before the MFMAs of tile t); the eight-wave form streams a key-tile image, cut once per pass, by LDS-DMA.
//  * online softmax with a LAZY reference maximum: the accumulators are rescaled only when a tile's maximum exceeds the
//    reference by more than 20 (fp32 has the range; p <= e^20), which happens in the first tiles only; the branch is
//    wave-uniform.
#include "common.h"
#include "x6.h"
#include <cstdlib>
#include <type_traits>

#define ATT_THR 20.0f


template <int D, int CT, int NKL, int NVL, int NTH>
__device__ __forceinline__ void att_gload(float4 (&rk)[NKL], float4 (&rv)[NVL], const float* __restrict__ qb,
                                          const float* __restrict__ v1b, const float* __restrict__ v2b, int C1, int C2, int k0,
                                          int tid) {
#pragma unroll
  for (int i = 0; i < NKL; ++i) {
    const int f = tid + NTH * i;
    const int key = f / (D / 4), dq = f % (D / 4);
    rk[i] = (f < 8 * D) ? *reinterpret_cast<const float4*>(qb + (int64_t)(k0 + key) * D + dq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < NVL; ++i) {
    const int f = tid + NTH * i;
    const int key = f / (CT / 4), c = (f % (CT / 4)) * 4;
    rv[i] = (c < C1) ? *reinterpret_cast<const float4*>(v1b + (int64_t)(k0 + key) * C1 + c)
                     : *reinterpret_cast<const float4*>(v2b + (int64_t)(k0 + key) * C2 + (c - C1));
  }
}

// =====================================================================================================
// Forward on the bf16 matrix pipe (x6.h): the flash structure above, every product as six bf16 MFMAs of K = 16 on exact three-way
// splits of the fp32 operands.
//  * the K / V tile of 32 keys is split into three bf16 images each -- on its way from the staging registers into LDS (IMG = false: the
//    two- and four-wave forms, D = 16), or once per pass into the key-tile image that the eight-wave form streams by LDS-DMA (IMG = true,
//    AttKImg below; T16384 d64 C256 b8: 5.64 ms with the cutting pass against 5.91, profiles/attn_pieces.txt):
//      K pieces  [32 keys][D bf16],  row pitch 2 D + 16 bytes: the A fragment (key = lane, 8 consecutive d) is one ds_read_b128;
//      V pieces  [32 keys][CT bf16], row pitch 2 CT + 64 bytes: the A fragment of O^T += V^T P^T (channel = lane, keys in the
//                reduction) is two ds_read_b64_tr_b16 -- the hardware transposes a 4-key x 16-channel block per 16 lanes;
//  * Q pieces stay in registers (B operand of S^T = K Q^T), and the exponentiated tile, still one query per lane column, is cut
//    into its three pieces in registers: element j of lane half h of k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3), the order
//    the score tile's registers already have, so the V reads simply address those keys;
//  * per 32-key tile and wave: 6 x (D / 16 + 2 NCT) MFMAs (120 at D = 64, C = 256: 3 840 matrix-pipe cycles against 10 240 for the
//    160 fp32 MFMAs), ~110 VALU instructions for the K / V split and 88 for P.
// =====================================================================================================
// ---- key-tile image (IMG instantiations): the K / V pieces of every 32-key tile, cut ONCE per pass by attn_cut_ktile_kernel instead of
// once per workgroup (T / 256 times), in exactly the bytes of one LDS stage:
//      [0, 3 KIMG)            K pieces [3][32 keys][2 D + 16 bytes]   (the last 16 bytes of a row are padding)
//      [3 KIMG, 3 KIMG + 3 VIMG)  V pieces [3][32 keys][2 CT + 64 bytes], V = [V1 | V2]   (the last 64 bytes of a row are padding)
//      .. BLK                 padding to whole KiB
// Padding is never written and never read.  Block b = n (T / 32) + tile starts at byte b * BLK; a tile load is BLK / 1024
// global_load_lds_dwordx4 per workgroup, issued at the top of the iteration BEFORE the one that consumes it: no staging registers, no
// split and no ds_write in the loop.
template <int D, int CT>
struct AttKImg {
  static constexpr int KP = 2 * D + 16, VP = 2 * CT + 64, KIMG = 32 * KP, VIMG = 32 * VP;
  static constexpr int BLK = (3 * KIMG + 3 * VIMG + 1023) / 1024 * 1024;
};
// 8 consecutive fp32 values -> one 16-byte chunk in each of the three piece images (`step` bytes apart)
__device__ __forceinline__ void att_cut8(const float* __restrict__ src, unsigned char* __restrict__ dst, int step) {
  const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
  uint32_t w[3][4];
  split3_pair(a.x, a.y, w[0][0], w[1][0], w[2][0]);
  split3_pair(a.z, a.w, w[0][1], w[1][1], w[2][1]);
  split3_pair(b.x, b.y, w[0][2], w[1][2], w[2][2]);
  split3_pair(b.z, b.w, w[0][3], w[1][3], w[2][3]);
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<uint4*>(dst + pc * step) = make_uint4(w[pc][0], w[pc][1], w[pc][2], w[pc][3]);
}
template <int D, int CT>
__global__ void __launch_bounds__(256) attn_cut_ktile_kernel(const float* __restrict__ q, const float* __restrict__ v1,
                                                             const float* __restrict__ v2, unsigned char* __restrict__ img, int C1, int C2) {
  typedef AttKImg<D, CT> I;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  unsigned char* blk = img + (int64_t)blockIdx.x * I::BLK;
  for (int f = threadIdx.x; f < 32 * (D / 8); f += 256) {
    const int row = f / (D / 8), ch = f % (D / 8);
    att_cut8(q + (row0 + row) * D + 8 * ch, blk + row * I::KP + 16 * ch, I::KIMG);
  }
  for (int f = threadIdx.x; f < 32 * (CT / 8); f += 256) {
    const int row = f / (CT / 8), ch = f % (CT / 8), c = 8 * ch;
    const float* src = (c < C1) ? v1 + (row0 + row) * C1 + c : v2 + (row0 + row) * C2 + (c - C1);
    att_cut8(src, blk + 3 * I::KIMG + row * I::VP + 16 * ch, I::VIMG);
  }
}

// NW waves per workgroup, each owning 32 queries; all share the staged key / value tiles.  NW = 8 for long sequences: the 82 KB of LDS
// allow one workgroup per CU, and with four waves every SIMD held ONE wave whose softmax (exp, max, rescale) left the matrix pipe
// idle; eight waves put two on each SIMD.  NW = 2 for short ones (T = 1024: 64 workgroups of four waves filled a quarter of the chip).
// Dynamic LDS: two stages, each the three K and three V piece images of 32 keys, or one block of the key-tile image.
template <int D, int NCT, bool IMG>
constexpr int attn_fwd_x6_lds = IMG ? 2 * AttKImg<D, NCT * 32>::BLK : 2 * 3 * 32 * ((2 * D + 16) + (2 * NCT * 32 + 64));

template <int D, int NCT, int NW, bool IMG>
__global__ void __launch_bounds__(NW * 64, 1) attn_fwd_x6_kernel(const float* __restrict__ q, const float* __restrict__ v1,
                                                                 const float* __restrict__ v2, const unsigned char* __restrict__ img,
                                                                 float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ lse,
                                                                 int T, int C1, int C2) {
  constexpr int CT = NCT * 32;
  constexpr int KP = 2 * D + 16, VP = 2 * CT + 64;          // row pitches (bytes)
  constexpr int KIMG = 32 * KP, VIMG = 32 * VP;             // one piece image
  constexpr int STAGE = IMG ? AttKImg<D, CT>::BLK : 3 * KIMG + 3 * VIMG;   // bytes per stage
  constexpr int NTH = NW * 64;
  constexpr int NKL = (8 * D + NTH - 1) / NTH;              // float4 loads per thread for a K tile
  constexpr int NVL = (8 * CT) / NTH;                       // float4 loads per thread for a V tile
  static_assert((8 * CT) % NTH == 0, "whole float4 passes over the V tile");
  static_assert(D % 16 == 0, "whole bf16 k-steps");
  static_assert(1 * STAGE + STAGE == attn_fwd_x6_lds<D, NCT, IMG>, "the host passes the bytes this carve ends at");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_x6[];  // [2][STAGE]
  typedef __attribute__((address_space(3))) unsigned char* lds_ptr;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr)smem_x6;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y;
  const int q0 = blockIdx.x * (NW * 32) + wid * 32;
  const float* qb = q + (int64_t)n * T * D;
  const float* v1b = v1 + (int64_t)n * T * C1;
  const float* v2b = v2 ? v2 + (int64_t)n * T * C2 : nullptr;

  // this lane's query pieces: B[k = d][col = query], d = 16 kk + 8 lh + j
  bf16x8_t qp[D / 16][3];
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk) {
    const float4 a = *reinterpret_cast<const float4*>(qb + (int64_t)(q0 + l31) * D + 16 * kk + 8 * lh);
    const float4 b = *reinterpret_cast<const float4*>(qb + (int64_t)(q0 + l31) * D + 16 * kk + 8 * lh + 4);
    const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split3_bf16(f, qp[kk]);
  }

  f32x16 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float mref = -INFINITY, lsum = 0.f;

  // staging: split each float4 into three 8-byte pieces and store them into the images of stage `st`
  float4 rk[NKL], rv[NVL];
  auto lstore = [&](int st) {
    unsigned char* base = smem_x6 + st * STAGE;
#pragma unroll
    for (int i = 0; i < NKL; ++i) {
      const int f = tid + NTH * i;
      if (f < 8 * D) {
        const int key = f / (D / 4), dq = f % (D / 4);
        uint32_t a0, a1, a2, b0, b1, b2;
        split3_pair(rk[i].x, rk[i].y, a0, a1, a2);
        split3_pair(rk[i].z, rk[i].w, b0, b1, b2);
        unsigned char* d = base + key * KP + dq * 8;
        *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(d + KIMG) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(d + 2 * KIMG) = make_uint2(a2, b2);
      }
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + NTH * i;
      const int key = f / (CT / 4), c4 = f % (CT / 4);
      uint32_t a0, a1, a2, b0, b1, b2;
      split3_pair(rv[i].x, rv[i].y, a0, a1, a2);
      split3_pair(rv[i].z, rv[i].w, b0, b1, b2);
      unsigned char* d = base + 3 * KIMG + key * VP + c4 * 8;
      *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
      *reinterpret_cast<uint2*>(d + VIMG) = make_uint2(a1, b1);
      *reinterpret_cast<uint2*>(d + 2 * VIMG) = make_uint2(a2, b2);
    }
  };
  // transposed V fragment reads: lane 4 q + p of a 16-lane group addresses key row q, channels 4 p .. 4 p + 3 of the group's 16
  const int i16 = lane & 15;
  const uint32_t vlane = (uint32_t)((4 * lh + (i16 >> 2)) * VP + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2);
  const uint32_t klane = (uint32_t)(l31 * KP + 16 * lh);

  // IMG: key tile k0's block goes global -> LDS stage `st` directly, wave w taking the KiB chunks w, w + NW, ..
  const unsigned char* imgl = IMG ? img + (int64_t)n * (T / 32) * STAGE + lane * 16 : nullptr;
  const int widu = __builtin_amdgcn_readfirstlane(wid);
  auto dma_tile = [&](int k0, int st) {
    constexpr int NCH = STAGE / 1024;
    const unsigned char* src = imgl + (int64_t)(k0 >> 5) * STAGE + widu * 1024;
    const uint32_t dst = lds0 + (uint32_t)(st * STAGE) + (uint32_t)widu * 1024u;
#pragma unroll
    for (int c = 0; c < (NCH + NW - 1) / NW; ++c) {
      if (NW * c + NW - 1 < NCH || NW * c + widu < NCH) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src + c * (NW * 1024)), "s"(dst + (uint32_t)(c * (NW * 1024)))
                     : "memory");
      }
    }
  };
  if constexpr (IMG) {
    dma_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    att_gload<D, CT, NKL, NVL, NTH>(rk, rv, qb, v1b, v2b, C1, C2, 0, tid);
    lstore(0);
  }
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < T; k0 += 32) {
    if constexpr (IMG) {
      // stage buf ^ 1 was read in the iteration before; every wave passed the barrier that ended it (the last iteration re-reads its own tile)
      dma_tile(k0 + 32 < T ? k0 + 32 : k0, buf ^ 1);
    } else {
      // unconditional prefetch (the last iteration re-reads its own tile): a conditional one sends rk/rv to scratch
      att_gload<D, CT, NKL, NVL, NTH>(rk, rv, qb, v1b, v2b, C1, C2, k0 + 32 < T ? k0 + 32 : k0, tid);
    }
    const uint32_t kimg = lds0 + (uint32_t)(buf * STAGE) + klane;
    const uint32_t vimg = lds0 + (uint32_t)(buf * STAGE + 3 * KIMG) + vlane;
    // S^T[key][query] for 32 keys x this wave's 32 queries
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) {
      bf16x8_t kp[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) {
        typedef __attribute__((address_space(3))) bf16x8_t* lp8;
        kp[pc] = *(lp8)(uintptr_t)(kimg + (uint32_t)(pc * KIMG + kk * 32));
      }
      st = mfma_x6(kp, qp[kk], st);
    }
    // online softmax, one query per lane column (keys split over the lane pair l, l^32)
    float tmax = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    if (__any(tmax > mref + ATT_THR)) {
      const float mnew = fmaxf(mref, tmax);
      const float alpha = __expf(mref - mnew);
#pragma unroll
      for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] *= alpha;
      lsum *= alpha;
      mref = mnew;
    }
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = __expf(st[r] - mref);
      psum += st[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    lsum += psum;
    // O^T[c][query] += V^T[c][key] P^T[key][query]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8_t pp[3];
      {
        const float f[8] = {st[8 * s], st[8 * s + 1], st[8 * s + 2], st[8 * s + 3], st[8 * s + 4], st[8 * s + 5], st[8 * s + 6], st[8 * s + 7]};
        split3_bf16(f, pp);
      }
#pragma unroll
      for (int c = 0; c < NCT; ++c) {
        bf16x8_t vp[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          typedef short s16x4_t __attribute__((ext_vector_type(4)));
          typedef __attribute__((address_space(3))) s16x4_t* lp4;
          const uint32_t ad = vimg + (uint32_t)(pc * VIMG + 16 * s * VP + 64 * c);
          union {
            s16x4_t h[2];
            bf16x8_t v;
          } u;
          u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)ad);
          u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)(ad + 8 * VP));
          vp[pc] = u.v;
        }
        acc[c] = mfma_x6(vp, pp, acc[c]);
      }
    }
    if constexpr (IMG)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's chunks of the next tile have landed (issued a whole tile ago)
    else
      lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: register r of tile c is channel c*32 + (r&3) + 8*(r>>2) + 4*lh of query q0 + l31
  const float inv = 1.f / lsum;
  const int64_t row = (int64_t)n * T + q0 + l31;
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int cbase = c * 32;
    float* ob = (cbase < C1) ? o1 + row * C1 + cbase : o2 + row * C2 + (cbase - C1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 o;
      o.x = acc[c][4 * g + 0] * inv;
      o.y = acc[c][4 * g + 1] * inv;
      o.z = acc[c][4 * g + 2] * inv;
      o.w = acc[c][4 * g + 3] * inv;
      *reinterpret_cast<float4*>(ob + 8 * g + 4 * lh) = o;
    }
  }
  if (lh == 0 && lse) lse[row] = mref + logf(lsum);
}

// The (D, C / 32) pairs the kernels are instantiated for, in one place: calls f(D, C / 32) with the two values as
// std::integral_constant<int, ..>; false: not a supported pair.  FWD16: also the two D = 16 pairs, which only the forward has.
template <bool FWD16, class F>
static bool att_dispatch(int D, int nct, F&& f) {
  using std::integral_constant;
  if (D == 64 && nct == 8) return f(integral_constant<int, 64>{}, integral_constant<int, 8>{}), true;
  if (D == 32 && nct == 8) return f(integral_constant<int, 32>{}, integral_constant<int, 8>{}), true;
  if (D == 32 && nct == 4) return f(integral_constant<int, 32>{}, integral_constant<int, 4>{}), true;
  if (D == 64 && nct == 4) return f(integral_constant<int, 64>{}, integral_constant<int, 4>{}), true;
  if constexpr (FWD16) {
    if (D == 16 && nct == 2) return f(integral_constant<int, 16>{}, integral_constant<int, 2>{}), true;
    if (D == 16 && nct == 4) return f(integral_constant<int, 16>{}, integral_constant<int, 4>{}), true;
  }
  return false;
}

// The forward's shape dispatch, in one place: waves per workgroup (each owns 32 queries).  Eight where whole 256-query workgroups still
// fill the chip, two where even 128-query ones would not, else four.  Pure host arithmetic; the tests assert it per shape.
extern "C" int fmi_attention_fwd_waves(int N, int T) {
  if (T % 256 == 0 && (int64_t)(T / 256) * N >= 256) return 8;
  return (int64_t)(T / 128) * N < 256 ? 2 : 4;
}

extern "C" int fmi_attention_fwd_f32(const float* q, const float* v1, const float* v2, float* o1, float* o2, float* lse,
                                     int N, int T, int D, int C1, int C2, void* stream) {
  if (!q || !v1 || !o1 || N <= 0 || T <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && (!v2 || !o2))) return FMI_ERR_BAD_ARG;
  if (T % 128 != 0 || C1 % 32 != 0 || C2 % 32 != 0 || N > 65535) return FMI_ERR_UNSUPPORTED;
  const int nw = fmi_attention_fwd_waves(N, T);
  if ((((uintptr_t)q | (uintptr_t)v1 | (uintptr_t)v2 | (uintptr_t)o1 | (uintptr_t)o2) & 15) != 0) return FMI_ERR_BAD_ARG;
  const int nct = (C1 + C2) / 32;
  const dim3 grid(T / (nw * 32), N), block(nw * 64);
  hipStream_t st = (hipStream_t)stream;
  int rc = FMI_OK;
  const bool known = att_dispatch<true>(D, nct, [&](auto d, auto n) {
    constexpr int DD = decltype(d)::value, NN = decltype(n)::value;
    auto launch = [&](auto w) {
      rc = fmi_launch_lds<attn_fwd_x6_kernel<DD, NN, decltype(w)::value, false>>(grid, block, attn_fwd_x6_lds<DD, NN, false>, st, q, v1, v2,
                                                                                 (const unsigned char*)nullptr, o1, o2, lse, T, C1, C2);
    };
    if (nw == 8) launch(std::integral_constant<int, 8>{});
    else if (nw == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 4>{});
  });
  if (!known) return FMI_ERR_UNSUPPORTED;
  if (rc != FMI_OK) return rc;
  return fmi_launch_status();
}

// =====================================================================================================
// Backward.  With P = softmax(q q^T), O_i = P V_i, upstream gO_i:
//   dV = P^T gO      dP = gO V^T      dS = P o (dP - delta),  delta_q = sum_c gO[q][c] O[q][c]
//   dQ[q] += sum_key dS[q][key] q[key]   (query side)       dQ[key] += sum_q dS[q][key] q[q]   (key side; K = Q)
// One workgroup owns a block of 32 KEYS (dV and the key-side dQ of those keys stay in registers for the whole kernel)
// and streams all query tiles; P is recomputed from the saved log-sum-exp.  The four waves of the workgroup split the
// REDUCTION dimension of dP -- the value channels -- and exchange their 32x32 partial tiles through LDS; the score tile
// is computed whole by every wave, on the bf16 pipe in the forward's arithmetic (see the comment at its pieces below):
//   per (32 queries x 32 keys) pair and wave:  S 6 D/16 bf16 + dP part 32 + dV (own 64 channels) 32 + dK or dQ tile 16 MFMAs.
// Scores are computed with the key on the lane, so P and dS are directly the B operands of the dV / dK products; only
// the query-side product needs dS transposed, through a private 4 KB LDS tile.  The query-side dQ tiles are added with
// fp32 atomics (whole 128-byte rows per wave instruction).
// =====================================================================================================
// dynamic LDS of attn_bwd_kernel: the resident key block and one query tile (V / gO and K / Q rows at odd pitches, lse and delta), the
// four waves' exchange tiles and two transposed dS tiles
template <int D, int NCT>
constexpr int attn_bwd_lds = (int)sizeof(float) * (2 * 32 * (NCT * 32 + 1) + 2 * 32 * (D + 1) + 64 + 4 * 2 * 1024 + 2 * 32 * 33);

template <int D, int NCT>  // NCT = (C1 + C2) / 32, multiple of 4
__global__ void __launch_bounds__(256, 1) attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ v1,
                                                          const float* __restrict__ v2, const float* __restrict__ g1,
                                                          const float* __restrict__ g2, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, float* __restrict__ gv1,
                                                          float* __restrict__ gv2, float* __restrict__ gq, int T, int C1, int C2, int kb0) {
  constexpr int CT = NCT * 32, CW = CT / 4, NCW = CW / 32;
  constexpr int LDV = CT + 1, LDQ = D + 1;
  constexpr int NQL = (8 * D) / 256 > 0 ? (8 * D) / 256 : 1, NVL = (8 * CT) / 256;
  constexpr int NDT = D / 32;  // 32-wide d tiles (1 or 2)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KJ = 32 * LDV, DOI = KJ + 32 * LDQ, QI = DOI + 32 * LDV, LSE = QI + 32 * LDQ, DEL = LSE + 32, EXO = DEL + 32,
                DST = EXO + 4 * 2 * 1024;  // offsets (floats)
  static_assert((int)sizeof(float) * (DST + 2 * 32 * 33) == attn_bwd_lds<D, NCT>, "the host passes the bytes this carve ends at");
  float* Vj = smem;                   // [32][LDV]
  float* Kj = smem + KJ;              // [32][LDQ]
  float* dOi = smem + DOI;            // [32][LDV]
  float* Qi = smem + QI;              // [32][LDQ]
  float* lse_i = smem + LSE;          // [32]
  float* del_i = smem + DEL;          // [32]
  float* EX = smem + EXO;             // [4][2][16][64]: the second [16][64] of a wave holds its partial dP tile (the first is unused)
  float* dsT = smem + DST;            // [2][32][33]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y, j0 = ((int)blockIdx.x + kb0) * 32;  // kb0: key-block offset of this launch (reproducible mode: one key block per launch)
  const float* qb = q + (int64_t)n * T * D;
  const float* v1b = v1 + (int64_t)n * T * C1;
  const float* v2b = v2 ? v2 + (int64_t)n * T * C2 : nullptr;
  const float* g1b = g1 + (int64_t)n * T * C1;
  const float* g2b = g2 ? g2 + (int64_t)n * T * C2 : nullptr;
  const float* lseb = lse + (int64_t)n * T;
  const float* delb = delta + (int64_t)n * T;

  // resident key block: V_j, K_j (row-major, odd pitch: conflict-free both along a row and down a column)
  for (int f = tid; f < 8 * CT; f += 256) {
    const int key = f / (CT / 4), c = (f % (CT / 4)) * 4;
    const float4 v = (c < C1) ? *reinterpret_cast<const float4*>(v1b + (int64_t)(j0 + key) * C1 + c)
                              : *reinterpret_cast<const float4*>(v2b + (int64_t)(j0 + key) * C2 + (c - C1));
    float* d = Vj + key * LDV + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  for (int f = tid; f < 8 * D; f += 256) {
    const int key = f / (D / 4), dd = (f % (D / 4)) * 4;
    const float4 v = *reinterpret_cast<const float4*>(qb + (int64_t)(j0 + key) * D + dd);
    float* d = Kj + key * LDQ + dd;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }

  f32x16 acc_dv[NCW], acc_dk;
#pragma unroll
  for (int c = 0; c < NCW; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_dv[c][r] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc_dk[r] = 0.f;
  const int cbase = wid * CW;            // this wave's value-channel slice
  const bool dk_role = wid < NDT;        // waves 0..NDT-1: key-side tile wid;  waves 2..2+NDT-1: query-side tile wid-2
  const bool dq_role = wid >= 2 && wid - 2 < NDT;
  const int dt = dk_role ? wid : wid - 2;

  float4 rq[NQL], rg[NVL];
  float rl = 0.f, rd = 0.f;
  auto gload = [&](int i0) {
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + 256 * i;
      const int row = f / (D / 4), dd = (f % (D / 4)) * 4;
      rq[i] = (f < 8 * D) ? *reinterpret_cast<const float4*>(qb + (int64_t)(i0 + row) * D + dd) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + 256 * i;
      const int row = f / (CT / 4), c = (f % (CT / 4)) * 4;
      rg[i] = (c < C1) ? *reinterpret_cast<const float4*>(g1b + (int64_t)(i0 + row) * C1 + c)
                       : *reinterpret_cast<const float4*>(g2b + (int64_t)(i0 + row) * C2 + (c - C1));
    }
    rl = lseb[i0 + (tid & 31)];
    rd = delb[i0 + (tid & 31)];
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + 256 * i;
      if (f < 8 * D) {
        float* d = Qi + (f / (D / 4)) * LDQ + (f % (D / 4)) * 4;
        d[0] = rq[i].x; d[1] = rq[i].y; d[2] = rq[i].z; d[3] = rq[i].w;
      }
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + 256 * i;
      float* d = dOi + (f / (CT / 4)) * LDV + (f % (CT / 4)) * 4;
      d[0] = rg[i].x; d[1] = rg[i].y; d[2] = rg[i].z; d[3] = rg[i].w;
    }
    if (tid < 32) {
      lse_i[tid] = rl;
      del_i[tid] = rd;
    }
  };

  gload(0);
  lstore();
  __syncthreads();
  // The score tile is the forward's product, not a plain fp32 one: P = exp(S - lse) is exact to fp32 rounding only while S carries the
  // rounding that lse saw.  |S| in the thousands has an ulp of 2^-12, and a d-split fp32 sum a few ulp off the forward's left a one-hot
  // row's P, and with it that key's dV, 6e-4 off.  So every wave computes the WHOLE tile as attn_fwd_x6_kernel does -- bf16 pieces, one
  // accumulator chained over d in steps of 16, the same six products per step -- which makes a key's score with itself (the entry that
  // dominates a sharp row) the same bits as in the forward.  The resident keys' pieces stay in registers.
  bf16x8_t kpc[D / 16][3];
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = Kj[l31 * LDQ + 16 * kk + 8 * lh + j];
    split3_bf16(f, kpc[kk]);
  }
  for (int i0 = 0; i0 < T; i0 += 32) {
    gload(i0 + 32 < T ? i0 + 32 : i0);  // unconditional prefetch of the next query tile into registers
    // ---- 1. score tile (whole, per wave) and the partial dP tile over this wave's slice of the value channels; lane = key, registers = queries
    f32x16 sp, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sp[r] = 0.f;
      dp[r] = 0.f;
    }
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = Qi[l31 * LDQ + 16 * kk + 8 * lh + j];
      bf16x8_t qpc[3];
      split3_bf16(f, qpc);
      sp = mfma_x6(qpc, kpc[kk], sp);
    }
#pragma unroll
    for (int s = 0; s < CW / 2; ++s)
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dOi[l31 * LDV + cbase + 2 * s + lh], Vj[l31 * LDV + cbase + 2 * s + lh], dp, 0, 0, 0);
    // ---- 2. exchange: every wave needs the full dP tile
    {
      float* ex = EX + wid * 2048 + lane;
#pragma unroll
      for (int r = 0; r < 16; ++r) ex[1024 + r * 64] = dp[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float b = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) b += EX[w * 2048 + 1024 + r * 64 + lane];
      dp[r] = b;
    }
    // ---- 3. P and dS (register r of half lh is query (r&3) + 8*(r>>2) + 4*lh)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float p = __expf(sp[r] - lse_i[qi]);
      sp[r] = p;
      dp[r] = p * (dp[r] - del_i[qi]);
    }
    // ---- 4. dV^T[c][key] += gO^T[c][q] P[q][key] for this wave's channels
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int qi = (s & 3) + 8 * (s >> 2) + 4 * lh;
#pragma unroll
      for (int c = 0; c < NCW; ++c)
        acc_dv[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(dOi[qi * LDV + cbase + c * 32 + l31], sp[s], acc_dv[c], 0, 0, 0);
    }
    // ---- 5. key side (dK^T[d][key] += Q^T[d][q] dS[q][key]) or query side (dQ[q][d] = dS[q][key] K[key][d])
    if (dk_role) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int qi = (s & 3) + 8 * (s >> 2) + 4 * lh;
        acc_dk = __builtin_amdgcn_mfma_f32_32x32x2f32(Qi[qi * LDQ + dt * 32 + l31], dp[s], acc_dk, 0, 0, 0);
      }
    } else if (dq_role) {
      float* t = dsT + (wid - 2) * (32 * 33);
#pragma unroll
      for (int r = 0; r < 16; ++r) t[((r & 3) + 8 * (r >> 2) + 4 * lh) * 33 + l31] = dp[r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave wrote it; LDS operations of a wave complete in order
      f32x16 dq;
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 16; ++s) dq = __builtin_amdgcn_mfma_f32_32x32x2f32(t[l31 * 33 + 2 * s + lh], Kj[(2 * s + lh) * LDQ + dt * 32 + l31], dq, 0, 0, 0);
      float* gqb = gq + ((int64_t)n * T + i0) * D + dt * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) atomicAdd(gqb + (int64_t)((r & 3) + 8 * (r >> 2) + 4 * lh) * D, dq[r]);
    }
    __syncthreads();   // all reads of the current query tile are done
    lstore();
    __syncthreads();
  }

  // all query-side atomics of this workgroup have COMPLETED before its key-side ones start: where both touch one row (the last query
  // tile of the last key block) their order is then fixed, which the reproducible mode relies on
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ---- epilogue: dV rows (plain stores, this workgroup is their only writer) and the key-side dQ (atomics)
  {
    const int64_t row = (int64_t)n * T + j0 + l31;
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
      const int ch = cbase + c * 32;
      float* ob = (ch < C1) ? gv1 + row * C1 + ch : gv2 + row * C2 + (ch - C1);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(ob + 8 * g + 4 * lh) =
            make_float4(acc_dv[c][4 * g], acc_dv[c][4 * g + 1], acc_dv[c][4 * g + 2], acc_dv[c][4 * g + 3]);
    }
    if (dk_role) {
      float* gqb = gq + row * D + dt * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) atomicAdd(gqb + (r & 3) + 8 * (r >> 2) + 4 * lh, acc_dk[r]);
    }
  }
}

// =====================================================================================================
// Backward, second structure (used when it fits), on the bf16 matrix pipe (x6.h): every wave owns its OWN block of 32 keys with ALL
// value channels and keeps that key block's V rows in registers, so
//  * nothing is exchanged between waves before the softmax backward (the first structure above exchanges partial tiles),
//  * one query tile staged in LDS feeds four key blocks (4x fewer L2 reads of gO / Q),
//  * the query-side dQ tiles of the four key blocks are summed through LDS first: 4x fewer fp32 atomics
//    (rocprofv3 WRITE_SIZE showed 17 GB of atomic traffic per launch for the first structure at T = 16384).
// Every product is six bf16 MFMAs of K = 16:
//  * the query tile (Q_i, gO_i) is cut into its three bf16 pieces on the way from the staging registers into LDS (IMG = false, reached through
//    fmi_attention_bwd_f32) or, IMG = true (fmi_attention_bwd_pieces_f32, what the library's callers dispatch to), once per pass by
//    attn_cut_qtile_kernel into the query-tile image (AttQImg below), whose blocks go global -> LDS by LDS-DMA: the copy of tile i + 1 is
//    issued behind a barrier that follows every wave's last read of tile i (the transposed Q reads of the dK phase), runs under the rest of
//    dK and the dQ phase, and is waited for in front of the barrier that ends the tile.  Three barriers a tile instead of two, no split, no
//    ds_write and no staging registers (212 VGPRs instead of 240): 15.16 ms against 16.11 at T16384 d64 C256 b8, cutting pass included.
//      gO pieces [32 q][CT], 16-byte chunks XOR-swizzled (chunk ^ (((q & 3) << 2) | ((q >> 2) & 3)) inside each 256-byte window) so
//      that the SAME image serves the row fragments of dP = gO V^T (ds_read_b128) and the transposed fragments of dV^T = gO^T P
//      (ds_read_b64_tr_b16), both conflict-free;
//      Q pieces  [32 q][D], 192-byte rows: row fragments for S, transposed fragments for dK^T = Q^T dS;
//  * the wave's own K / V rows stay fp32 in registers, laid out as B fragments (8 consecutive reduction indices per lane), and
//    are split on the fly next to the MFMAs that consume them: three-piece copies of V would need 192 registers on top of the
//    160 accumulator registers;
//  * P and dS (lane = key, registers = queries) are split in registers: they are the B operands of dV^T and dK^T as they stand;
//    for the query-side product dQ = dS K the three dS pieces go through a private [key][q] LDS image and come back transposed
//    (ds_read_b64_tr_b16) as A fragments;
//  * the query-side tiles of the four key blocks are summed in LDS (ds_add_f32) before the global atomics.
// Per query tile and wave: 264 bf16 MFMAs (8 448 matrix-pipe cycles; the fp32-MFMA kernel it replaced: 352 MFMAs, 22 528 cycles).
// =====================================================================================================
// With all 8 channel tiles in one launch the 128 dV + 32 dK accumulator registers leave no room for the V pieces (192 registers): V stays
// fp32 and is split per tile (700 VALU instructions of ~2 400).  (A two-launch form that kept the V pieces in registers -- 288 instead of
// 264 MFMAs per tile pair -- measured 14.9 + 5.6 ms against 17.6 ms for the single launch.)
#ifdef FMI_ATT_STAMP  // diagnostic build only (tools/bench_tools/build_flags.sh attstamp -DFMI_ATT_STAMP): cycle stamps of the phases of ONE query tile
__device__ unsigned long long fmi_att_stamps[16];
extern "C" int fmi_debug_attn_stamps(unsigned long long* host16) {
  return hipMemcpyFromSymbol(host16, HIP_SYMBOL(fmi_att_stamps), sizeof(unsigned long long) * 16) == hipSuccess ? FMI_OK : FMI_ERR_LAUNCH;
}
#define ATT_STAMP(i)                                                                                   \
  do {                                                                                                 \
    if (blockIdx.x == 0 && blockIdx.y == 0 && i0 == 32 * 100 && wid == 0 && lane == 0)                   \
      fmi_att_stamps[i] = __builtin_amdgcn_s_memtime();                                                \
  } while (0)
#else
#define ATT_STAMP(i)
#endif
// ---- query-tile image: the bf16 pieces of gO = [gO1 | gO2] and Q, cut ONCE per backward pass instead of once per workgroup (T / 128 times)
// and stored in exactly the bytes the kernel below keeps in LDS, one block per 32 query rows:
//      [0, 3 GIMG)        gO pieces [3][32 q][2 CT bytes], the 16-byte chunks of a row XOR-swizzled as in Gs (below)
//      [3 GIMG, LSE)      Q pieces  [3][32 q][192 bytes]; bytes 2 D .. 191 of a row are padding, never written and never read
//      [LSE, LSE + 256)   lse[32], delta[32] of the rows (fp32)
//      [LSE + 256, BLK)   padding to whole KiB, never written and never read
// so a tile load is BLK / 1024 global_load_lds_dwordx4 per workgroup (1 KiB per wave instruction, lane-linear in LDS: pitch and swizzle
// are applied here, on the global side).  Block b = n (T / 32) + tile starts at byte b * BLK.
template <int D, int CT>
struct AttQImg {
  static constexpr int GP = 2 * CT, GIMG = 32 * GP, QP = 192, QIMG = 32 * QP;
  static constexpr int LSE = 3 * GIMG + 3 * QIMG;
  static constexpr int BLK = (LSE + 256 + 1023) / 1024 * 1024;
  static_assert(2 * D <= QP, "Q row fits its pitch");
};
__device__ __forceinline__ int att_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
// one workgroup per block (32 rows of the flattened [N T] row axis; T % 32 == 0).  Pure bandwidth: 4 B read, 6 B written per element.
template <int D, int CT>
__global__ void __launch_bounds__(256) attn_cut_qtile_kernel(const float* __restrict__ q, const float* __restrict__ g1,
                                                             const float* __restrict__ g2, const float* __restrict__ lse,
                                                             const float* __restrict__ delta, unsigned char* __restrict__ img, int C1, int C2) {
  typedef AttQImg<D, CT> I;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  unsigned char* blk = img + (int64_t)blockIdx.x * I::BLK;
  for (int f = threadIdx.x; f < 32 * (CT / 8); f += 256) {
    const int row = f / (CT / 8), ch = f % (CT / 8), c = 8 * ch;
    const float* src = (c < C1) ? g1 + (row0 + row) * C1 + c : g2 + (row0 + row) * C2 + (c - C1);
    att_cut8(src, blk + row * I::GP + 16 * ((ch & ~15) | ((ch ^ att_swz(row)) & 15)), I::GIMG);
  }
  for (int f = threadIdx.x; f < 32 * (D / 8); f += 256) {
    const int row = f / (D / 8), ch = f % (D / 8);
    att_cut8(q + (row0 + row) * D + 8 * ch, blk + 3 * I::GIMG + row * I::QP + 16 * ch, I::QIMG);
  }
  if (threadIdx.x < 64) {
    const int r = threadIdx.x & 31;
    reinterpret_cast<float*>(blk + I::LSE)[threadIdx.x] = threadIdx.x < 32 ? lse[row0 + r] : delta[row0 + r];
  }
}

// dynamic LDS of attn_bwd2_x6_kernel: the query tile's gO and Q piece images with lse / delta (IMG: one block of the query-tile image),
// the four waves' key-block piece images and their dS^T / partial-dQ slots
template <int D, int NCT, bool IMG>
constexpr int attn_bwd2_x6_lds = (IMG ? AttQImg<D, NCT * 32>::BLK : 3 * 32 * 2 * NCT * 32 + 3 * 32 * 192 + 64 * 4) + 4 * 3 * 32 * (2 * D + 16) +
                                 4 * ((D / 32) * 4096 > 6144 ? (D / 32) * 4096 : 6144);

template <int D, int NCT, bool IMG>
__global__ void __launch_bounds__(256, 1) attn_bwd2_x6_kernel(const float* __restrict__ q, const float* __restrict__ v1,
                                                              const float* __restrict__ v2, const float* __restrict__ g1,
                                                              const float* __restrict__ g2, const float* __restrict__ lse,
                                                              const float* __restrict__ delta, const unsigned char* __restrict__ img,
                                                              float* __restrict__ gv1, float* __restrict__ gv2, float* __restrict__ gq,
                                                              int T, int C1, int C2, int kb0) {
  constexpr int CT = NCT * 32, LDQ = D + 1, NDT = D / 32;
  constexpr int NQL = (8 * D) / 256 > 0 ? (8 * D) / 256 : 1, NVL = (8 * CT) / 256;
  constexpr int GP = 2 * CT, GIMG = 32 * GP;   // gO piece image: row pitch, bytes per piece
  constexpr int QP = 192, QIMG = 32 * QP;      // Q piece image
  constexpr int TIMG = 32 * 64;                // dS^T piece image: [32 keys][32 q] bf16
  constexpr int KP = 2 * D + 16, KIMG = 32 * KP;  // key-block piece image: row pitch (conflict-free row reads), bytes per piece
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  unsigned char* Gs = smem_b;                                     // [3][32][GP]
  unsigned char* Qs = Gs + 3 * GIMG;                              // [3][32][QP]
  float* lse_i = reinterpret_cast<float*>(Qs + 3 * QIMG);         // [32]
  float* del_i = lse_i + 32;                                      // [32]
  // IMG: Gs .. del_i are one block of the query-tile image (AttQImg), copied as it stands; its last KiB holds lse / delta and padding
  constexpr int KS = IMG ? AttQImg<D, CT>::BLK : 3 * GIMG + 3 * QIMG + 256, TS = KS + 4 * 3 * KIMG;  // offsets (bytes)
  unsigned char* Ks = smem_b + KS;                                // [4][3][32][KP]  each wave's key block as bf16 pieces: B operand of S (row reads) and of dQ = dS K (transposed reads)
  unsigned char* Ts = smem_b + TS;                                // [4][WSLOT]  per wave: the transposed dS pieces [3][32][64 B], then (same bytes) its query-side partial tiles
  // a wave's partial dQ tiles [NDT][16][64] overwrite its own dS^T image once its transposed reads are done; the other waves read them between
  // the two barriers that follow, and the image is rewritten only after the second one.  (LDS float atomics instead of partial tiles: ~250
  // cycles per wave instruction, measured.)
  constexpr int WSLOT = (NDT * 16 * 64 * 4 > 3 * TIMG) ? NDT * 16 * 64 * 4 : 3 * TIMG;
  static_assert(TS + 4 * WSLOT == attn_bwd2_x6_lds<D, NCT, IMG>, "the host passes the bytes this carve ends at");
  typedef __attribute__((address_space(3))) unsigned char* lds_ptr;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr)smem_b;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y, j0 = ((int)blockIdx.x + kb0) * 128 + wid * 32;   // this wave's keys (kb0: key-block offset of this launch)
  const float* qb = q + (int64_t)n * T * D;
  const float* v1b = v1 + (int64_t)n * T * C1;
  const float* v2b = v2 ? v2 + (int64_t)n * T * C2 : nullptr;
  const float* g1b = g1 + (int64_t)n * T * C1;
  const float* g2b = g2 ? g2 + (int64_t)n * T * C2 : nullptr;
  const float* lseb = lse + (int64_t)n * T;
  const float* delb = delta + (int64_t)n * T;

  unsigned char* ks = Ks + wid * 3 * KIMG;
  for (int f = lane; f < 8 * D; f += 64) {
    const int key = f / (D / 4), dq4 = f % (D / 4);
    const float4 v = *reinterpret_cast<const float4*>(qb + (int64_t)(j0 + key) * D + dq4 * 4);
    uint32_t a0, a1, a2, b0, b1, b2;
    split3_pair(v.x, v.y, a0, a1, a2);
    split3_pair(v.z, v.w, b0, b1, b2);
    unsigned char* d = ks + key * KP + dq4 * 8;
    *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
    *reinterpret_cast<uint2*>(d + KIMG) = make_uint2(a1, b1);
    *reinterpret_cast<uint2*>(d + 2 * KIMG) = make_uint2(a2, b2);
  }
  // B fragments of this wave's keys, V[key = l31][16 kk + 8 lh + j], in registers (the K fragments are read from the piece image per tile)
  float vfrag[CT / 16][8];
#pragma unroll
  for (int kk = 0; kk < CT / 16; ++kk) {
    const int c = 16 * kk + 8 * lh;
    const float* src = (c < C1) ? v1b + (int64_t)(j0 + l31) * C1 + c : v2b + (int64_t)(j0 + l31) * C2 + (c - C1);
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    vfrag[kk][0] = a.x, vfrag[kk][1] = a.y, vfrag[kk][2] = a.z, vfrag[kk][3] = a.w;
    vfrag[kk][4] = b.x, vfrag[kk][5] = b.y, vfrag[kk][6] = b.z, vfrag[kk][7] = b.w;
  }

  f32x16 acc_dv[NCT], acc_dk[NDT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_dv[c][r] = 0.f;
#pragma unroll
  for (int c = 0; c < NDT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_dk[c][r] = 0.f;

  // IMG: tile i0's block of the image goes global -> LDS directly, wave w taking the KiB chunks w, w + 4, ..; no staging registers
  const unsigned char* imgl = IMG ? img + (int64_t)n * (T / 32) * AttQImg<D, CT>::BLK + lane * 16 : nullptr;
  const int widu = __builtin_amdgcn_readfirstlane(wid);
  auto dma_tile = [&](int i0) {
    constexpr int NCH = AttQImg<D, CT>::BLK / 1024;
    const unsigned char* src = imgl + (int64_t)(i0 >> 5) * AttQImg<D, CT>::BLK + widu * 1024;
    const uint32_t dst = lds0 + (uint32_t)widu * 1024u;
#pragma unroll
    for (int c = 0; c < (NCH + 3) / 4; ++c) {
      if (4 * c + 3 < NCH || 4 * c + widu < NCH) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(src + c * 4096), "s"(dst + (uint32_t)(c * 4096))
                     : "memory");
      }
    }
  };
  float4 rq[NQL], rg[NVL];
  float rl = 0.f, rd = 0.f;
  auto gload = [&](int i0) {
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + 256 * i;
      const int row = f / (D / 4), dd = (f % (D / 4)) * 4;
      rq[i] = (f < 8 * D) ? *reinterpret_cast<const float4*>(qb + (int64_t)(i0 + row) * D + dd) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + 256 * i;
      const int row = f / (CT / 4), c = (f % (CT / 4)) * 4;
      rg[i] = (c < C1) ? *reinterpret_cast<const float4*>(g1b + (int64_t)(i0 + row) * C1 + c)
                       : *reinterpret_cast<const float4*>(g2b + (int64_t)(i0 + row) * C2 + (c - C1));
    }
    rl = lseb[i0 + (tid & 31)];
    rd = delb[i0 + (tid & 31)];
  };
  auto swz = [](int row) { return att_swz(row); };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + 256 * i;
      if (f < 8 * D) {
        uint32_t a0, a1, a2, b0, b1, b2;
        split3_pair(rq[i].x, rq[i].y, a0, a1, a2);
        split3_pair(rq[i].z, rq[i].w, b0, b1, b2);
        unsigned char* d = Qs + (f / (D / 4)) * QP + (f % (D / 4)) * 8;
        *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(d + QIMG) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(d + 2 * QIMG) = make_uint2(a2, b2);
      }
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + 256 * i;
      const int row = f / (CT / 4), c4 = f % (CT / 4), ch = c4 >> 1;
      uint32_t a0, a1, a2, b0, b1, b2;
      split3_pair(rg[i].x, rg[i].y, a0, a1, a2);
      split3_pair(rg[i].z, rg[i].w, b0, b1, b2);
      unsigned char* d = Gs + row * GP + 16 * ((ch & ~15) | ((ch ^ swz(row)) & 15)) + 8 * (c4 & 1);
      *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
      *reinterpret_cast<uint2*>(d + GIMG) = make_uint2(a1, b1);
      *reinterpret_cast<uint2*>(d + 2 * GIMG) = make_uint2(a2, b2);
    }
    if (tid < 32) {
      lse_i[tid] = rl;
      del_i[tid] = rd;
    }
  };
  typedef short s16x4_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4_t* lp4;
  typedef __attribute__((address_space(3))) bf16x8_t* lp8;
  auto tr2 = [&](uint32_t a0, uint32_t a1) {  // two transposed 4 x 16 blocks -> one 8-element fragment
    union {
      s16x4_t h[2];
      bf16x8_t v;
    } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)a0);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)a1);
    // the return data must land in an architectural VGPR: with 160 accumulator registers the allocator also hands out AGPRs as LDS
    // destinations, and an LDS read into an AGPR stalls the LDS return path (SQ_LDS_DATA_FIFO_FULL 1e10 cycles: 38.7 -> 18.9 ms)
    asm volatile("" : "+v"(u.v));
    return u.v;
  };
  // the same read with the pin left to the caller (pin3 below): a pin is also the point where the wave WAITS for the data, so a fragment
  // that is read one step ahead gets pinned only after the MFMAs of the current step have been issued
  auto tr2_nowait = [&](uint32_t a0, uint32_t a1) {
    union {
      s16x4_t h[2];
      bf16x8_t v;
    } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)a0);
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)a1);
    return u.v;
  };
  auto pin3 = [&](bf16x8_t (&a)[3]) { asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2])); };
  // per-lane address parts
  const int i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3, gb = (lane >> 4) & 1;
  const uint32_t g_row = lds0 + (uint32_t)(l31 * GP);                  // row fragments of gO: + piece, + swizzled chunk
  const int g_rx = (lh ^ swz(l31)) & 15;                               // chunk (2 kk + lh) ^ swz(row) = (2 kk) ^ g_rx on the low four bits
  const uint32_t g_tr = lds0 + (uint32_t)((4 * lh + tq) * GP + 8 * (tp & 1));   // transposed fragments of gO: query rows 16 s + 4 lh + tq (+ 8)
  const int g_tx = (2 * gb + (tp >> 1)) ^ ((tq << 2) | lh);            // chunk 4 ct + 2 gb + (tp >> 1), swizzle of that row ((+8: ^ 2)
  const uint32_t q_row = lds0 + (uint32_t)(3 * GIMG + l31 * QP + 16 * lh);
  const uint32_t q_tr = lds0 + (uint32_t)(3 * GIMG + (4 * lh + tq) * QP + (16 * gb + 4 * tp) * 2);
  const uint32_t k_base = lds0 + (uint32_t)(Ks - smem_b) + (uint32_t)(wid * 3 * KIMG);
  const uint32_t k_row = k_base + (uint32_t)(l31 * KP + 16 * lh);                              // row fragments: key l31, + piece, + 32 kk
  const uint32_t k_tr = k_base + (uint32_t)((8 * lh + tq) * KP + (16 * gb + 4 * tp) * 2);      // transposed: key rows 16 s + 8 lh + tq (+ 4), + 64 c
  const uint32_t t_base = (uint32_t)(Ts - smem_b) + (uint32_t)(wid * WSLOT);
  float* RBw = reinterpret_cast<float*>(Ts + wid * WSLOT);
  // dS^T image: row = key (64 bytes = 8 slots of four queries); slot (2 g + lh) of key k is stored at slot ^ ((k >> 1) & 7): the 16 keys
  // one ds_write_b64 group covers then fall on 16 different bank pairs (unswizzled: two)
  const uint32_t t_wr = lds0 + t_base + (uint32_t)(l31 * 64);                    // + piece, + 8 * ((2 g + lh) ^ t_wx)
  const int t_wx = (l31 >> 1) & 7;
  const uint32_t t_tr = lds0 + t_base + (uint32_t)((8 * lh + tq) * 64);          // key rows 16 s + 8 lh + tq (+ 4): + 8 * ((4 gb + tp) ^ swizzle of that row)
  const int t_rx = (4 * lh) | (tq >> 1);                                         // ((row >> 1) & 7) of the first row; the row 4 further: + 2

  if constexpr (IMG) {
    dma_tile(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    gload(0);
    lstore();
  }
  __syncthreads();
  for (int i0 = 0; i0 < T; i0 += 32) {
    ATT_STAMP(0);
    // ---- S[q][key], dP[q][key]: lane = key, registers = queries
    f32x16 sp, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sp[r] = 0.f;
      dp[r] = 0.f;
    }
    {  // fragments of step kk + 1 are read before the MFMAs of step kk are issued
      auto s_frag = [&](int kk, bf16x8_t (&a)[3], bf16x8_t (&b)[3]) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) a[pc] = *(lp8)(uintptr_t)(q_row + (uint32_t)(pc * QIMG + kk * 32));
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) b[pc] = *(lp8)(uintptr_t)(k_row + (uint32_t)(pc * KIMG + kk * 32));
      };
      bf16x8_t a[3], b[3], an[3], bn[3];
      s_frag(0, a, b);
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk) {
        if (kk + 1 < D / 16) s_frag(kk + 1, an, bn);
        __builtin_amdgcn_sched_barrier(0);
        sp = mfma_x6(a, b, sp);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          a[pc] = an[pc];
          b[pc] = bn[pc];
        }
      }
    }
    ATT_STAMP(1);
    // The swizzled chunk offsets of the fragment reads are two instructions each.  Computed from the plain lane constants they are
    // loop-invariant, and the optimiser keeps all of them (one per step: ~48 registers) across the tile loop -- parked in AGPRs and
    // fetched with v_accvgpr_read at best, spilled to scratch and reloaded in front of the read at worst.  The asm makes the lane
    // constant opaque at each use, so the offset is recomputed where it is needed.
    auto gt_frag = [&](int s, int c, bf16x8_t (&a)[3]) {  // gO^T fragment: channels 32 c .., queries 16 s ..
      int tx = g_tx;
      asm volatile("" : "+v"(tx));
      const uint32_t ch0 = (uint32_t)(16 * (((4 * c) & 15) ^ tx) + 16 * ((4 * c) & ~15));
      const uint32_t ch1 = (uint32_t)(16 * (((4 * c) & 15) ^ tx ^ 2) + 16 * ((4 * c) & ~15));
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
        a[pc] = tr2_nowait(g_tr + (uint32_t)(pc * GIMG + 16 * s * GP) + ch0, g_tr + (uint32_t)(pc * GIMG + (16 * s + 8) * GP) + ch1);
    };
    {
      // ---- P first (it needs S only), then ONE loop over the channel steps that carries both products whose reduction runs over the
      // channels / whose output is channels: dP[q][key] += gO[q][c] V[key][c] (step kk: 16 channels; the V pieces are split per step,
      // ~45 VALU instructions) and dV^T[c][key] += gO^T[c][q] P[q][key] (step j = kk: one 32-channel tile of one 16-query half; no VALU).
      // Alone, the dP steps are bound by the split (an MFMA gap hides about five vector instructions: 309 cycles a step against 192 of
      // MFMA) while the dV steps leave their gaps empty; together a step has 12 MFMAs for the same 45 instructions.  Every fragment of
      // step kk + 1 is read / split before the MFMAs of step kk are issued and waited for (pinned) after them.
#pragma unroll
      for (int r = 0; r < 16; ++r) sp[r] = __expf(sp[r] - lse_i[(r & 3) + 8 * (r >> 2) + 4 * lh]);
      bf16x8_t pp[2][3];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float f[8] = {sp[8 * s], sp[8 * s + 1], sp[8 * s + 2], sp[8 * s + 3], sp[8 * s + 4], sp[8 * s + 5], sp[8 * s + 6], sp[8 * s + 7]};
        split3_bf16(f, pp[s]);
      }
      auto g_frag = [&](int kk, bf16x8_t (&a)[3]) {
        int rx = g_rx;
        asm volatile("" : "+v"(rx));
        const uint32_t ad = g_row + (uint32_t)(16 * (((2 * kk) & 15) ^ rx) + 16 * ((2 * kk) & ~15));
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) a[pc] = *(lp8)(uintptr_t)(ad + (uint32_t)(pc * GIMG));
      };
      // half h of the split of V step kk: values 4 h .. 4 h + 3 -> words 2 h, 2 h + 1 of the three piece fragments
      auto v_split_half = [&](int kk, int h, u32x4_t (&w)[3]) {
#pragma unroll
        for (int e = 2 * h; e < 2 * h + 2; ++e) {
          uint32_t w0, w1, w2;
          split3_pair(vfrag[kk][2 * e], vfrag[kk][2 * e + 1], w0, w1, w2);
          w[0][e] = w0, w[1][e] = w1, w[2][e] = w2;
        }
      };
      // The V values must not look loop-invariant to the optimiser: it would hoist all 192 piece registers out of the tile loop and
      // spill.  An empty asm that "modifies" them is free only while the value stays in the register class the constraint names: the
      // accumulators take 192 of the 256 AGPRs, so half of the V fragments live in VGPRs ("+v") and half in the remaining AGPRs ("+a";
      // with "+v" on all of them each use cost a v_accvgpr_read AND a v_accvgpr_write back)
      auto v_touch = [&](int kk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (kk < (CT / 16) / 2)
            asm volatile("" : "+v"(vfrag[kk][j]));
          else
            asm volatile("" : "+a"(vfrag[kk][j]));
        }
      };
      auto ds_make = [&](int s, bf16x8_t (&ds)[3]) {
        const float e[8] = {dp[8 * s], dp[8 * s + 1], dp[8 * s + 2], dp[8 * s + 3], dp[8 * s + 4], dp[8 * s + 5], dp[8 * s + 6], dp[8 * s + 7]};
        split3_bf16(e, ds);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {  // registers 8 s .. 8 s + 3 are queries 16 s + 4 lh .., registers 8 s + 4 .. + 7 queries 16 s + 8 + 4 lh ..
          typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
          typedef __attribute__((address_space(3))) u32x2_t* lpu2;
          const u32x4_t w = __builtin_bit_cast(u32x4_t, ds[pc]);
          *(lpu2)(uintptr_t)(t_wr + (uint32_t)(pc * TIMG + 8 * (((4 * s) | lh) ^ t_wx))) = u32x2_t{w[0], w[1]};      // g = 2 s
          *(lpu2)(uintptr_t)(t_wr + (uint32_t)(pc * TIMG + 8 * (((4 * s + 2) | lh) ^ t_wx))) = u32x2_t{w[2], w[3]};  // g = 2 s + 1
        }
      };
      auto qt_frag = [&](int s, bf16x8_t (&aq)[NDT][3]) {
#pragma unroll
        for (int c = 0; c < NDT; ++c)
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)
            aq[c][pc] = tr2_nowait(q_tr + (uint32_t)(pc * QIMG + 16 * s * QP + 64 * c), q_tr + (uint32_t)(pc * QIMG + (16 * s + 8) * QP + 64 * c));
      };
      bf16x8_t aq0[NDT][3], aq1[NDT][3], ds0[3], ds1[3];
      constexpr int NDP = CT / 16, NDV = 2 * NCT;   // NDV <= NDP: the dV step of the tile (s, c) = (j / NCT, j % NCT) rides on dP step j
      static_assert(NDV <= NDP, "dV steps ride on the dP steps");
      // A step has two halves of six MFMAs.  First half: dP with the fragments a (gO rows) and b (V pieces) made during the step before;
      // the gO^T fragment t of this step's dV tile is read at its start.  Second half: dV with t; a is dead by then and receives the gO
      // rows of step kk + 1.  The split of V step kk + 1 is spread over both halves, four vector instructions behind each MFMA (an MFMA
      // gap hides vector issue only while it stays within its 32 cycles: about five instructions; left alone the scheduler puts 9 - 16
      // of them between two MFMAs and then issues five MFMAs back to back -- 537 cycles a step against 384 of MFMA, stamps)
      bf16x8_t a[3], b[3], t[3];
      u32x4_t wn[3];
      g_frag(0, a);
      v_touch(0);
      v_split_half(0, 0, wn);
      v_split_half(0, 1, wn);
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) b[pc] = __builtin_bit_cast(bf16x8_t, wn[pc]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < NDP; ++kk) {
        if (kk < NDV) gt_frag(kk / NCT, kk % NCT, t);
        if (kk + 1 < NDP) {
          v_touch(kk + 1);
          v_split_half(kk + 1, 0, wn);
        }
        dp = mfma_x6(a, b, dp);
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kk < NDV) pin3(t);
        if (kk + 1 < NDP) {
          g_frag(kk + 1, a);
          v_split_half(kk + 1, 1, wn);
        }
        if (kk < NDV) acc_dv[kk < NDV ? kk % NCT : 0] = mfma_x6(t, pp[kk < NDV ? kk / NCT : 0], acc_dv[kk < NDV ? kk % NCT : 0]);
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          if (g == 0) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) b[pc] = __builtin_bit_cast(bf16x8_t, wn[pc]);
      }
    ATT_STAMP(2);
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] = sp[r] * (dp[r] - del_i[(r & 3) + 8 * (r >> 2) + 4 * lh]);
    ATT_STAMP(3);
      qt_frag(0, aq0);
      ds_make(0, ds0);
      // ---- dK^T[d][key] += Q^T[d][q] dS[q][key];  dS pieces -> private transposed image (A operand of dQ below).
      // The pieces of the second 16-query half are split and stored behind the MFMAs of the first half, and the next query tile's
      // global loads (address arithmetic: ~70 vector instructions) are issued behind the MFMAs of the second half: their 40 staging
      // registers are live from here on only -- across the dP / dV loop they would not fit (82 registers went to scratch)
#pragma unroll
      for (int c = 0; c < NDT; ++c) pin3(aq0[c]);
      __builtin_amdgcn_sched_barrier(0);
      qt_frag(1, aq1);
      ds_make(1, ds1);
#pragma unroll
      for (int c = 0; c < NDT; ++c) acc_dk[c] = mfma_x6(aq0[c], ds0, acc_dk[c]);
      __builtin_amdgcn_sched_group_barrier(0x100, 6 * NDT, 0);
#pragma unroll
      for (int g = 0; g < 6 * NDT; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < NDT; ++c) pin3(aq1[c]);
    ATT_STAMP(4);
      if constexpr (IMG) {
        // aq1 was this wave's last read of the query tile (the dQ phase reads Ks and Ts only).  Once every wave is here the next tile's
        // block may overwrite Gs / Qs / lse_i / del_i; the copy (the last tile re-reads its own block) runs under the remaining dK
        // MFMAs and the whole dQ phase and is waited for before the barrier that ends the tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        dma_tile(i0 + 32 < T ? i0 + 32 : i0);
#pragma unroll
        for (int c = 0; c < NDT; ++c) acc_dk[c] = mfma_x6(aq1[c], ds1, acc_dk[c]);
      } else {
        gload(i0 + 32 < T ? i0 + 32 : i0);
#pragma unroll
        for (int c = 0; c < NDT; ++c) acc_dk[c] = mfma_x6(aq1[c], ds1, acc_dk[c]);
#pragma unroll
        for (int g = 0; g < 6 * NDT; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      // ---- query side: dQ[q][d] = dS[q][key] K[key][d] for this wave's keys
    ATT_STAMP(5);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the transposed image was written by this wave; a wave's LDS operations complete in order
      f32x16 dqs[NDT];
      auto dq_frag = [&](int j, bf16x8_t (&a)[3], bf16x8_t (&b)[3]) {  // step j = (c, s)
        const int c = j >> 1, s = j & 1;
  #pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          a[pc] = tr2_nowait(t_tr + (uint32_t)(pc * TIMG + 16 * s * 64 + 8 * ((4 * gb + tp) ^ t_rx)),
                             t_tr + (uint32_t)(pc * TIMG + (16 * s + 4) * 64 + 8 * ((4 * gb + tp) ^ (t_rx + 2))));
        }
  #pragma unroll
        for (int pc = 0; pc < 3; ++pc)
          b[pc] = tr2_nowait(k_tr + (uint32_t)(pc * KIMG + 16 * s * KP + 64 * c), k_tr + (uint32_t)(pc * KIMG + (16 * s + 4) * KP + 64 * c));
      };
      bf16x8_t a[3], b[3], an[3], bn[3];
      dq_frag(0, a, b);
      pin3(a);
      pin3(b);
  #pragma unroll
      for (int j = 0; j < 2 * NDT; ++j) {  // same pipeline as above: the fragments of step j + 1 are in flight while step j multiplies
        if (j + 1 < 2 * NDT) dq_frag(j + 1, an, bn);
        __builtin_amdgcn_sched_barrier(0);
        if ((j & 1) == 0) {
  #pragma unroll
          for (int r = 0; r < 16; ++r) dqs[j >> 1][r] = 0.f;
        }
        dqs[j >> 1] = mfma_x6(a, b, dqs[j >> 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (j + 1 < 2 * NDT) {
          pin3(an);
          pin3(bn);
        }
  #pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          a[pc] = an[pc];
          b[pc] = bn[pc];
        }
      }
    ATT_STAMP(6);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's transposed reads of its dS^T image are done: the partial tiles may overwrite it
  #pragma unroll
      for (int c = 0; c < NDT; ++c)
  #pragma unroll
        for (int r = 0; r < 16; ++r) RBw[(c * 16 + r) * 64 + lane] = dqs[c][r];
    ATT_STAMP(7);
      __syncthreads();   // every wave is done with the query tile; the four slots hold the partial dQ tiles
    ATT_STAMP(8);
      // sum the partials: NDT*16 register-rows in all, wave w takes rows [w*NDT*4, (w+1)*NDT*4) and issues the atomics.  All the partials
      // are read first; the next query tile's pieces are split and stored while they are in flight (every wave is past the barrier, so
      // nobody reads the gO / Q images any more), then the sums and the atomics follow
      float part[NDT * 4][4];
  #pragma unroll
      for (int rr = 0; rr < NDT * 4; ++rr)
  #pragma unroll
        for (int w = 0; w < 4; ++w) part[rr][w] = reinterpret_cast<const float*>(Ts + w * WSLOT)[(wid * NDT * 4 + rr) * 64 + lane];
    ATT_STAMP(9);
      if constexpr (IMG)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's chunks of the next tile's block have landed (issued a dQ phase ago)
      else
        lstore();
    ATT_STAMP(10);
  #pragma unroll
      for (int rr = 0; rr < NDT * 4; ++rr) {
        const int row = wid * NDT * 4 + rr;       // = c*16 + r
        const int c = row >> 4, r = row & 15;
        float sum = 0.f;
  #pragma unroll
        for (int w = 0; w < 4; ++w) sum += part[rr][w];
        atomicAdd(gq + ((int64_t)n * T + i0 + (r & 3) + 8 * (r >> 2) + 4 * lh) * D + c * 32 + l31, sum);
      }
    }
    __syncthreads();
    ATT_STAMP(11);
  }

  // all query-side atomics of this workgroup have COMPLETED before its key-side ones start: where both touch one row (the last query
  // tile of the last key block) their order is then fixed, which the reproducible mode relies on
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ---- epilogue: dV rows of this wave's keys (plain stores) and the key-side dQ (atomics)
  const int64_t row = (int64_t)n * T + j0 + l31;
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int ch = c * 32;
    float* ob = (ch < C1) ? gv1 + row * C1 + ch : gv2 + row * C2 + (ch - C1);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(ob + 8 * g + 4 * lh) = make_float4(acc_dv[c][4 * g], acc_dv[c][4 * g + 1], acc_dv[c][4 * g + 2], acc_dv[c][4 * g + 3]);
  }
#pragma unroll
  for (int c = 0; c < NDT; ++c) {
    float* gqb = gq + row * D + c * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) atomicAdd(gqb + (r & 3) + 8 * (r >> 2) + 4 * lh, acc_dk[c][r]);
  }
}

// delta[row] = sum_c a1[row][c] b1[row][c] (+ second pair): one wave per row
__global__ void __launch_bounds__(256) rowdot2_kernel(const float* __restrict__ a1, const float* __restrict__ b1, int C1,
                                                      const float* __restrict__ a2, const float* __restrict__ b2, int C2,
                                                      float* __restrict__ out, int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += a1[row * C1 + c] * b1[row * C1 + c];
  if (a2)
    for (int c = lane; c < C2; c += 64) s += a2[row * C2 + c] * b2[row * C2 + c];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// Launch of a backward kernel over its key blocks (grid.x; `kb`, the key-block offset, is the kernels' last argument).  Reproducible mode:
// the query-side tiles of dQ receive one atomic contribution per KEY BLOCK; launching the key blocks one after the other (stream order)
// fixes the order of those additions -- same kernels, grid.x = 1.
template <auto Kernel, class... A>
static int att_launch_key_blocks(dim3 grid, int lds_bytes, hipStream_t st, A... args) {
  const bool det = fmi_det();
  int rc = FMI_OK;
  for (int kb = 0; kb < (det ? (int)grid.x : 1) && rc == FMI_OK; ++kb)
    rc = fmi_launch_lds<Kernel>(det ? dim3(1, grid.y) : grid, dim3(256), lds_bytes, st, args..., kb);
  return rc;
}

// The backward's shape dispatch, in one place: 2 = the key-block-per-wave structure (attn_bwd2*), where its T / 128 workgroups per image
// fill the chip; 1 = the first structure (attn_bwd_kernel), which has 4x the workgroups.
extern "C" int fmi_attention_bwd_structure(int N, int T) {
  return (T % 128 == 0 && (int64_t)(T / 128) * N >= 128) ? 2 : 1;
}

extern "C" int fmi_attention_bwd_f32(const float* q, const float* v1, const float* v2, const float* o1, const float* o2,
                                     const float* go1, const float* go2, const float* lse, float* delta_scratch, float* gv1,
                                     float* gv2, float* gq_zeroed, int N, int T, int D, int C1, int C2, void* stream) {
  if (!q || !v1 || !o1 || !go1 || !lse || !delta_scratch || !gv1 || !gq_zeroed || N <= 0 || T <= 0 || C1 <= 0 || C2 < 0)
    return FMI_ERR_BAD_ARG;
  if (C2 > 0 && (!v2 || !o2 || !go2 || !gv2)) return FMI_ERR_BAD_ARG;
  // T % 128 as the forward: the kernels take any T % 32 == 0, but P = exp(S - lse) needs the lse of fmi_attention_fwd_f32 (its rounding
  // of the scores, see attn_bwd_kernel), and no forward produces one for the other T
  if (T % 128 != 0 || C1 % 32 != 0 || C2 % 32 != 0 || N > 65535) return FMI_ERR_UNSUPPORTED;
  const int nct = (C1 + C2) / 32;
  if (!att_dispatch<false>(D, nct, [](auto, auto) {})) return FMI_ERR_UNSUPPORTED;  // refused before the delta pass is launched
  if ((((uintptr_t)q | (uintptr_t)v1 | (uintptr_t)v2 | (uintptr_t)go1 | (uintptr_t)go2 | (uintptr_t)gv1 | (uintptr_t)gv2) & 15) != 0)
    return FMI_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(rowdot2_kernel, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, st, go1, o1, C1, C2 ? go2 : nullptr, o2, C2,
                     delta_scratch, rows);
  const bool second = fmi_attention_bwd_structure(N, T) == 2;  // one key block per wave, fragments in registers, 4x fewer atomics
  int rc = FMI_OK;
  att_dispatch<false>(D, nct, [&](auto d, auto n) {
    constexpr int DD = decltype(d)::value, NN = decltype(n)::value;
    if (second)
      rc = att_launch_key_blocks<attn_bwd2_x6_kernel<DD, NN, false>>(dim3(T / 128, N), attn_bwd2_x6_lds<DD, NN, false>, st, q, v1, v2, go1, go2, lse,
                                                                     delta_scratch, (const unsigned char*)nullptr, gv1, gv2, gq_zeroed, T, C1, C2);
    else
      rc = att_launch_key_blocks<attn_bwd_kernel<DD, NN>>(dim3(T / 32, N), attn_bwd_lds<DD, NN>, st, q, v1, v2, go1, go2, lse, delta_scratch, gv1,
                                                          gv2, gq_zeroed, T, C1, C2);
  });
  return rc != FMI_OK ? rc : fmi_launch_status();
}


// =====================================================================================================
// Backward on the query-tile image (AttQImg): the same second-structure kernel, its gO / Q pieces cut once per pass by
// attn_cut_qtile_kernel and streamed by LDS-DMA.  fmi_attention_bwd_uses_pieces is the shape dispatch (the shapes the second structure
// takes above); the entry point itself accepts every shape the kernel can run, so a test may call it below the fill-the-GPU threshold.
// =====================================================================================================
static bool att_pieces_shape(int T, int D, int C1, int C2) {
  return T > 0 && T % 128 == 0 && C1 > 0 && C2 >= 0 && C1 % 32 == 0 && C2 % 32 == 0 && att_dispatch<false>(D, (C1 + C2) / 32, [](auto, auto) {});
}
extern "C" int fmi_attention_bwd_uses_pieces(int N, int T, int D, int C1, int C2) {
  return N > 0 && N <= 65535 && att_pieces_shape(T, D, C1, C2) && fmi_attention_bwd_structure(N, T) == 2;
}
// bytes of the backward's query-tile image (0: the shape has none)
extern "C" int fmi_attention_bwd_image_bytes(int N, int T, int D, int C1, int C2, int64_t* bytes) {
  if (!bytes || N <= 0) return FMI_ERR_BAD_ARG;
  *bytes = 0;
  if (!att_pieces_shape(T, D, C1, C2)) return FMI_OK;
  att_dispatch<false>(D, (C1 + C2) / 32, [&](auto d, auto n) {
    *bytes = (int64_t)N * (T / 32) * AttQImg<decltype(d)::value, decltype(n)::value * 32>::BLK;
  });
  return FMI_OK;
}

extern "C" int fmi_attention_bwd_pieces_f32(const float* q, const float* v1, const float* v2, const float* o1, const float* o2,
                                            const float* go1, const float* go2, const float* lse, float* delta_scratch, void* image,
                                            int64_t image_bytes, float* gv1, float* gv2, float* gq_zeroed, int N, int T, int D, int C1,
                                            int C2, void* stream) {
  if (!q || !v1 || !o1 || !go1 || !lse || !delta_scratch || !image || !gv1 || !gq_zeroed || N <= 0 || T <= 0 || C1 <= 0 || C2 < 0)
    return FMI_ERR_BAD_ARG;
  if (C2 > 0 && (!v2 || !o2 || !go2 || !gv2)) return FMI_ERR_BAD_ARG;
  if (!att_pieces_shape(T, D, C1, C2) || N > 65535) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)v1 | (uintptr_t)v2 | (uintptr_t)go1 | (uintptr_t)go2 | (uintptr_t)gv1 | (uintptr_t)gv2 | (uintptr_t)image) & 15) != 0)
    return FMI_ERR_BAD_ARG;
  int64_t need = 0;
  fmi_attention_bwd_image_bytes(N, T, D, C1, C2, &need);
  if (image_bytes < need) return FMI_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(rowdot2_kernel, dim3((unsigned)ceil_div64(rows, 4)), dim3(256), 0, st, go1, o1, C1, C2 ? go2 : nullptr, o2, C2,
                     delta_scratch, rows);
  unsigned char* img = (unsigned char*)image;
  int rc = FMI_OK;
  att_dispatch<false>(D, (C1 + C2) / 32, [&](auto d, auto n) {
    constexpr int DD = decltype(d)::value, NN = decltype(n)::value;
    hipLaunchKernelGGL((attn_cut_qtile_kernel<DD, NN * 32>), dim3((unsigned)(rows / 32)), dim3(256), 0, st, q, go1, go2, lse,
                       (const float*)delta_scratch, img, C1, C2);
    rc = att_launch_key_blocks<attn_bwd2_x6_kernel<DD, NN, true>>(dim3(T / 128, N), attn_bwd2_x6_lds<DD, NN, true>, st, q, v1, v2, go1, go2, lse,
                                                                  delta_scratch, (const unsigned char*)img, gv1, gv2, gq_zeroed, T, C1, C2);
  });
  return rc != FMI_OK ? rc : fmi_launch_status();
}

// =====================================================================================================
// Forward on the key-tile image (AttKImg): the eight-wave kernel with its K / V pieces cut once per pass and streamed by LDS-DMA.
// fmi_attention_fwd_uses_pieces is the shape dispatch (where fmi_attention_fwd_f32 takes eight waves, D in {32, 64}); the entry point
// itself accepts every T % 256 == 0 of those D / C.
// =====================================================================================================
extern "C" int fmi_attention_fwd_uses_pieces(int N, int T, int D, int C1, int C2) {
  return N > 0 && N <= 65535 && att_pieces_shape(T, D, C1, C2) && fmi_attention_fwd_waves(N, T) == 8;
}
extern "C" int fmi_attention_fwd_image_bytes(int N, int T, int D, int C1, int C2, int64_t* bytes) {
  if (!bytes || N <= 0) return FMI_ERR_BAD_ARG;
  *bytes = 0;
  if (!att_pieces_shape(T, D, C1, C2) || T % 256 != 0) return FMI_OK;
  att_dispatch<false>(D, (C1 + C2) / 32, [&](auto d, auto n) {
    *bytes = (int64_t)N * (T / 32) * AttKImg<decltype(d)::value, decltype(n)::value * 32>::BLK;
  });
  return FMI_OK;
}
extern "C" int fmi_attention_fwd_pieces_f32(const float* q, const float* v1, const float* v2, void* image, int64_t image_bytes, float* o1,
                                            float* o2, float* lse, int N, int T, int D, int C1, int C2, void* stream) {
  if (!q || !v1 || !o1 || !image || N <= 0 || T <= 0 || C1 <= 0 || C2 < 0 || (C2 > 0 && (!v2 || !o2))) return FMI_ERR_BAD_ARG;
  if (!att_pieces_shape(T, D, C1, C2) || T % 256 != 0 || N > 65535) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)v1 | (uintptr_t)v2 | (uintptr_t)o1 | (uintptr_t)o2 | (uintptr_t)image) & 15) != 0) return FMI_ERR_BAD_ARG;
  int64_t need = 0;
  fmi_attention_fwd_image_bytes(N, T, D, C1, C2, &need);
  if (image_bytes < need) return FMI_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* img = (unsigned char*)image;
  int rc = FMI_OK;
  att_dispatch<false>(D, (C1 + C2) / 32, [&](auto d, auto n) {
    constexpr int DD = decltype(d)::value, NN = decltype(n)::value;
    hipLaunchKernelGGL((attn_cut_ktile_kernel<DD, NN * 32>), dim3((unsigned)((int64_t)N * T / 32)), dim3(256), 0, st, q, v1, v2, img, C1, C2);
    rc = fmi_launch_lds<attn_fwd_x6_kernel<DD, NN, 8, true>>(dim3(T / 256, N), dim3(512), attn_fwd_x6_lds<DD, NN, true>, st, q, v1, v2,
                                                             (const unsigned char*)img, o1, o2, lse, T, C1, C2);
  });
  return rc != FMI_OK ? rc : fmi_launch_status();
}
