// Fused self-attention forward on bf16 operands for the PICNet decoder's Auto_Attn at inference (base_function.py:420-439):
//      O = softmax_j(q_i . q_j) V   (queries = keys, no scaling),   optionally   o = gamma * O + residual.
// q [N,T,D], v and o [N,T,C] are bf16; scores, running maximum, row sum and the output accumulators are fp32; P is rounded to bf16 only
// as the B operand of O^T += V^T P^T (the row sum adds the unrounded fp32 values).  The fp32 forward and the backward live in
// attention.hip; the mapping here is that of its bf16-pipe ("x6") forward with ONE bf16 MFMA where that one issues six, and nothing to cut:
//  * NW waves x 32 queries, one query per lane column (S^T = K Q^T, the Q fragment in registers for the whole kernel), so the
//    exponentiated tile is already the B operand of the second product and never touches LDS;
//  * a stage is 64 keys: K rows [D bf16] at pitch 2 D + 16 bytes (A fragment = one ds_read_b128), V rows [C bf16] at pitch 2 C + 64 bytes
//    (A fragment = two ds_read_b64_tr_b16); global rows are already in that order, so a tile goes global -> registers -> LDS as 16-byte
//    chunks, double buffered, the loads of tile t + 1 in flight during the 2 (D / 16 + 2 NCT) MFMAs of tile t; one barrier per 64 keys;
//  * online softmax with a LAZY reference maximum, as in the fp32 kernels: one wave-uniform test per 64 keys, and a rescale only when a
//    tile's maximum exceeds the reference by more than ATT_THR (fp32 and bf16 have the range: p <= e^20); when it fires, the
//    accumulators AND the row sum -- everything still expressed at the old reference -- are scaled by exp(old - new) exactly once;
//  * the epilogue's gamma * O + residual is evaluated in fp32 before the one rounding of o.
// No atomics, no score matrix in memory, no fp32 detour.
#include "bf16x8.h"
#include "x6.h"

#define ATT_THR 20.0f


// dynamic LDS of attn_fwd_bf16_kernel: two stages of 64 K rows and 64 V rows at their padded pitches
template <int D, int NCT>
constexpr int attn_fwd_bf16_lds = 2 * 64 * ((2 * D + 16) + (2 * NCT * 32 + 64));

// GUIDED (ExampleGuidedAttention, example_guided_att.py:21-41): the V tile is [ref | src], each CT / 2 channels wide -- a 16-byte chunk of
// a row comes from v (= ref) for the first CT / 2 channels and from v2 (= src) for the rest -- so ONE softmax serves both value maps,
// and the epilogue blends the first half with ref by the soft mask m [N,T]: o[:CT/2] = (1 - m) (A ref) + m ref, o[CT/2:] = A src.
// CF > 0 (GUIDED only; the pSp shapes, psp_encoders.py:128-132): the value maps are CF channels wide and grid index z is a SLICE of
// CT / 2 = 128 of them -- the V tile is [ref slice | src slice], read at row pitch CF from channel 128 z, and written to
// o[..., 128 z : 128 z + 128] and o[..., CF + 128 z : CF + 128 z + 128] of the [N,T,2 CF] output.  Every slice recomputes the scores from
// the shared q (2 T^2 D against 4 T^2 128 of value work), so the accumulators stay at NCT tiles whatever CF is.  CF == 0 is the
// unsliced kernel, whose code the slicing does not touch.
template <int D, int NCT, int NW, bool GUIDED = false, int CF = 0>
__global__ void __launch_bounds__(NW * 64, 1) attn_fwd_bf16_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ v,
                                                                   uint16_t* __restrict__ o, float* __restrict__ lse,
                                                                   const float* __restrict__ gamma, const uint16_t* __restrict__ res, int T,
                                                                   const uint16_t* __restrict__ v2, const float* __restrict__ mask) {
  constexpr int CT = NCT * 32, KEYS = 64;
  constexpr int KP = 2 * D + 16, VP = 2 * CT + 64;          // row pitches (bytes)
  constexpr int KBYTES = KEYS * KP, STAGE = KBYTES + KEYS * VP;
  constexpr int NTH = NW * 64;
  constexpr int KCH = KEYS * D / 8, VCH = KEYS * CT / 8;    // 16-byte chunks of a K / V tile
  constexpr int NKL = (KCH + NTH - 1) / NTH, NVL = VCH / NTH;
  static_assert(VCH % NTH == 0, "whole 16-byte passes over the V tile");
  static_assert(D % 16 == 0, "whole bf16 k-steps");
  static_assert(1 * STAGE + STAGE == attn_fwd_bf16_lds<D, NCT>, "the host passes the bytes this carve ends at");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b16[];  // [2][STAGE]
  typedef __attribute__((address_space(3))) unsigned char* lds_ptr;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr)smem_b16;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y;
  const int q0 = blockIdx.x * (NW * 32) + wid * 32;
  const uint16_t* qb = q + (int64_t)n * T * D;
  constexpr int CV = GUIDED ? CT / 2 : CT;                  // channels of one value map (of its slice with CF)
  constexpr int CP = CF ? CF : CV;                          // row pitch of a value map (elements)
  static_assert(CF == 0 || (GUIDED && CF % CV == 0), "slices are whole halves of the guided V tile");
  const int coff = CF ? (int)blockIdx.z * CV : 0;           // first channel of this workgroup's slice
  const uint16_t* vb = v + (int64_t)n * T * CP + coff;
  const uint16_t* vb2 = GUIDED ? v2 + (int64_t)n * T * CP + coff : nullptr;

  // this lane's query fragment: B[k = d][col = query], d = 16 kk + 8 lh + j
  bf16x8_t qp[D / 16];
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk)
    qp[kk] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(q0 + l31) * D + 16 * kk + 8 * lh));

  f32x16 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float mref = -INFINITY, lsum = 0.f;

  u32x4_t rk[NKL], rv[NVL];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NKL; ++i) {
      const int f = tid + NTH * i;
      const int key = f / (D / 8), ch = f % (D / 8);
      rk[i] = (f < KCH) ? *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(k0 + key) * D + 8 * ch) : u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + NTH * i;
      const int key = f / (CT / 8), ch = f % (CT / 8);
      if constexpr (GUIDED)
        rv[i] = *reinterpret_cast<const u32x4_t*>((ch < CV / 8 ? vb + 8 * ch : vb2 + 8 * (ch - CV / 8)) + (int64_t)(k0 + key) * CP);
      else
        rv[i] = *reinterpret_cast<const u32x4_t*>(vb + (int64_t)(k0 + key) * CT + 8 * ch);
    }
  };
  auto lstore = [&](int st) {
    unsigned char* base = smem_b16 + st * STAGE;
#pragma unroll
    for (int i = 0; i < NKL; ++i) {
      const int f = tid + NTH * i;
      if (f < KCH) *reinterpret_cast<u32x4_t*>(base + (f / (D / 8)) * KP + (f % (D / 8)) * 16) = rk[i];
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + NTH * i;
      *reinterpret_cast<u32x4_t*>(base + KBYTES + (f / (CT / 8)) * VP + (f % (CT / 8)) * 16) = rv[i];
    }
  };
  // transposed V fragment reads: lane 4 q + p of a 16-lane group addresses key row q, channels 4 p .. 4 p + 3 of the group's 16
  const int i16 = lane & 15;
  const uint32_t vlane = (uint32_t)((4 * lh + (i16 >> 2)) * VP + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2);
  const uint32_t klane = (uint32_t)(l31 * KP + 16 * lh);

  gload(0);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < T; k0 += KEYS) {
    gload(k0 + KEYS < T ? k0 + KEYS : k0);  // unconditional prefetch (the last iteration re-reads its own tile)
    const uint32_t kimg = lds0 + (uint32_t)(buf * STAGE) + klane;
    const uint32_t vimg = lds0 + (uint32_t)(buf * STAGE + KBYTES) + vlane;
    // S^T[key][query] for 2 x 32 keys x this wave's 32 queries; register r of half lh is key 32 u + (r & 3) + 8 (r >> 2) + 4 lh
    f32x16 st[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[u][r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk) {
        typedef __attribute__((address_space(3))) bf16x8_t* lp8;
        const bf16x8_t kp = *(lp8)(uintptr_t)(kimg + (uint32_t)(u * 32 * KP + kk * 32));
        st[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kp, qp[kk], st[u], 0, 0, 0);
      }
    }
    float tmax = fmaxf(st[0][0], st[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, fmaxf(st[0][r], st[1][r]));
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
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[u][r] = __expf(st[u][r] - mref);
        psum += st[u][r];
      }
    psum += __shfl_xor(psum, 32, 64);
    lsum += psum;
    // O^T[c][query] += V^T[c][key] P^T[key][query]: element j of k-step s is key 32 u + 16 s + 8 (j >> 2) + 4 lh + (j & 3), the order
    // the score registers already have
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4_t pw;
#pragma unroll
        for (int e = 0; e < 4; ++e) pw[e] = cvt_pk_bf16(st[u][8 * s + 2 * e], st[u][8 * s + 2 * e + 1]);
        const bf16x8_t pp = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
          typedef short s16x4_t __attribute__((ext_vector_type(4)));
          typedef __attribute__((address_space(3))) s16x4_t* lp4;
          const uint32_t ad = vimg + (uint32_t)((32 * u + 16 * s) * VP + 64 * c);
          union {
            s16x4_t h[2];
            bf16x8_t v;
          } vf;
          vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)ad);
          vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp4)(uintptr_t)(ad + 8 * VP));
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.v, pp, acc[c], 0, 0, 0);
        }
      }
    }
    lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: register r of tile c is channel c*32 + (r&3) + 8*(r>>2) + 4*lh of query q0 + l31
  const float inv = 1.f / lsum;
  const float gm = gamma ? gamma[0] : 0.f;
  const int64_t row = (int64_t)n * T + q0 + l31;
  const float mk = GUIDED ? mask[row] : 0.f;
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t off = CF ? row * (2 * CF) + (c < NCT / 2 ? 0 : CF - CV) + coff + c * 32 + 8 * g + 4 * lh : row * CT + c * 32 + 8 * g + 4 * lh;
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = acc[c][4 * g + e] * inv;
      if constexpr (GUIDED) {
        if (c < NCT / 2) {  // (1 - m) (A ref) + m ref in fp32 before the one rounding; m = 1 returns ref bit for bit
          const uint2 r = *reinterpret_cast<const uint2*>(v + row * CP + coff + c * 32 + 8 * g + 4 * lh);
          const float om = 1.f - mk;
          f[0] = fmaf(om, f[0], mk * bf_lo(r.x));
          f[1] = fmaf(om, f[1], mk * bf_hi(r.x));
          f[2] = fmaf(om, f[2], mk * bf_lo(r.y));
          f[3] = fmaf(om, f[3], mk * bf_hi(r.y));
        }
      } else if (gamma) {
        const uint2 r = *reinterpret_cast<const uint2*>(res + off);
        f[0] = fmaf(gm, f[0], bf_lo(r.x));
        f[1] = fmaf(gm, f[1], bf_hi(r.x));
        f[2] = fmaf(gm, f[2], bf_lo(r.y));
        f[3] = fmaf(gm, f[3], bf_hi(r.y));
      }
      *reinterpret_cast<uint2*>(o + off) = make_uint2(cvt_pk_bf16(f[0], f[1]), cvt_pk_bf16(f[2], f[3]));
    }
  }
  if (lh == 0 && lse) lse[row] = mref + logf(lsum);
}

// The bf16 forward's shape dispatch: eight waves (256 queries per workgroup) where whole workgroups still fill the chip, else four.
extern "C" int fmi_attention_fwd_bf16_waves(int N, int T) { return (T % 256 == 0 && (int64_t)(T / 256) * N >= 256) ? 8 : 4; }

extern "C" int fmi_attention_fwd_bf16(const uint16_t* q, const uint16_t* v, uint16_t* o, float* lse, const float* gamma,
                                      const uint16_t* residual, int N, int T, int D, int C, int waves, void* stream) {
  if (!q || !v || !o || N <= 0 || T <= 0 || D <= 0 || C <= 0 || (gamma == nullptr) != (residual == nullptr)) return FMI_ERR_BAD_ARG;
  if (T % 128 != 0 || !((D == 64 && C == 256) || (D == 32 && C == 128)) || N > 65535) return FMI_ERR_UNSUPPORTED;
  if (waves != 0 && waves != 4 && !(waves == 8 && T % 256 == 0)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)v | (uintptr_t)o | (uintptr_t)residual) & 15) != 0 || (((uintptr_t)lse | (uintptr_t)gamma) & 3) != 0)
    return FMI_ERR_BAD_ARG;
  const int nw = waves ? waves : fmi_attention_fwd_bf16_waves(N, T);
  const dim3 grid(T / (nw * 32), N), block(nw * 64);
  hipStream_t st = (hipStream_t)stream;
#define ATTB16_LAUNCH(DD, NN, WW) \
  fmi_launch_lds<attn_fwd_bf16_kernel<DD, NN, WW>>(grid, block, attn_fwd_bf16_lds<DD, NN>, st, q, v, o, lse, gamma, residual, T, (const uint16_t*)nullptr, \
                                                   (const float*)nullptr)
  const int rc = D == 64 ? (nw == 8 ? ATTB16_LAUNCH(64, 8, 8) : ATTB16_LAUNCH(64, 8, 4)) : (nw == 8 ? ATTB16_LAUNCH(32, 4, 8) : ATTB16_LAUNCH(32, 4, 4));
#undef ATTB16_LAUNCH
  return rc != FMI_OK ? rc : fmi_launch_status();
}

// The guided attention and its blend in one launch (example_guided_att.py:21-41): q [N,T,D], src / ref [N,T,C], out [N,T,2C] bf16, mask fp32
// [N,T].  The dispatch is the plain forward's: eight waves where whole workgroups still fill the chip, else four.
extern "C" int fmi_guided_attention_fwd_bf16_waves(int N, int T) { return fmi_attention_fwd_bf16_waves(N, T); }

extern "C" int fmi_guided_attention_fwd_bf16(const uint16_t* q, const uint16_t* src, const uint16_t* ref, const float* mask, uint16_t* out, int N,
                                             int T, int D, int C, int waves, void* stream) {
  if (!q || !src || !ref || !mask || !out || N <= 0 || T <= 0 || D <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (T % 128 != 0 || !(D == 32 && C == 128) || N > 65535) return FMI_ERR_UNSUPPORTED;
  if (waves != 0 && waves != 4 && !(waves == 8 && T % 256 == 0)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)src | (uintptr_t)ref | (uintptr_t)out) & 15) != 0 || ((uintptr_t)mask & 3) != 0) return FMI_ERR_BAD_ARG;
  const int nw = waves ? waves : fmi_guided_attention_fwd_bf16_waves(N, T);
  const dim3 grid(T / (nw * 32), N), block(nw * 64);
  hipStream_t st = (hipStream_t)stream;
#define ATTG16_LAUNCH(WW)                                                                                                                        \
  fmi_launch_lds<attn_fwd_bf16_kernel<32, 8, WW, true>>(grid, block, attn_fwd_bf16_lds<32, 8>, st, q, ref, out, (float*)nullptr, (const float*)nullptr, \
                                                        (const uint16_t*)nullptr, T, src, mask)
  const int rc = nw == 8 ? ATTG16_LAUNCH(8) : ATTG16_LAUNCH(4);
#undef ATTG16_LAUNCH
  return rc != FMI_OK ? rc : fmi_launch_status();
}

// The same at the pSp encoder's shapes (psp_encoders.py:128-132): (D, C) = (64, 256) is attention2, (128, 512) attention1.  One workgroup
// per (query tile, sample, slice of 128 channels): C / 128 slices in grid z, each recomputing the scores from the shared q.  Arguments,
// checks and the wave dispatch are fmi_guided_attention_fwd_bf16's, whose own accepted shape stays (32, 128).
extern "C" int fmi_guided_attention_sliced_fwd_bf16(const uint16_t* q, const uint16_t* src, const uint16_t* ref, const float* mask, uint16_t* out,
                                                    int N, int T, int D, int C, int waves, void* stream) {
  if (!q || !src || !ref || !mask || !out || N <= 0 || T <= 0 || D <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (T % 128 != 0 || !((D == 64 && C == 256) || (D == 128 && C == 512)) || N > 65535) return FMI_ERR_UNSUPPORTED;
  if (waves != 0 && waves != 4 && !(waves == 8 && T % 256 == 0)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)src | (uintptr_t)ref | (uintptr_t)out) & 15) != 0 || ((uintptr_t)mask & 3) != 0) return FMI_ERR_BAD_ARG;
  const int nw = waves ? waves : fmi_guided_attention_fwd_bf16_waves(N, T);
  const dim3 grid(T / (nw * 32), N, C / 128), block(nw * 64);
  hipStream_t st = (hipStream_t)stream;
#define ATTGS_LAUNCH(DD, CC, WW)                                                                                                                  \
  fmi_launch_lds<attn_fwd_bf16_kernel<DD, 8, WW, true, CC>>(grid, block, attn_fwd_bf16_lds<DD, 8>, st, q, ref, out, (float*)nullptr, (const float*)nullptr, \
                                                            (const uint16_t*)nullptr, T, src, mask)
  const int rc = C == 256 ? (nw == 8 ? ATTGS_LAUNCH(64, 256, 8) : ATTGS_LAUNCH(64, 256, 4)) : (nw == 8 ? ATTGS_LAUNCH(128, 512, 8) : ATTGS_LAUNCH(128, 512, 4));
#undef ATTGS_LAUNCH
  return rc != FMI_OK ? rc : fmi_launch_status();
}
