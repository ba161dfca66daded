// Backward of the bf16 self-attention of attention_bf16.hip (training; Auto_Attn with attn_dtype = bf16):
//      O = softmax_j(q_i . q_j) V   (queries = keys, no scaling),   lse_i = log sum_j exp(q_i . q_j)   as fmi_attention_fwd_bf16 stored them.
// With S_ij = q_i . q_j - lse_i,  P = exp(S),  dP_ij = go_i . v_j - delta_i,  delta_i = sum_c go_ic o_ic,  dS = P o dP:
//      gv_j = sum_i P_ij go_i          gq_j = sum_i dS_ij q_i  (key side)  +  sum_i dS_ji q_i  (query side).
// Rounding points: q16, v16, go16 = bf16(go), and P and dS as MFMA operands are rounded to bf16 ONCE each (round to nearest even);
// scores, exp, dP - delta, delta itself (from the UNROUNDED go) and every accumulator are fp32.
//
// No float atomics and no hand-off between workgroups: every output element has exactly one writing workgroup per launch, so the result
// does not depend on scheduling and fmi_set_deterministic has nothing to switch.  Three launches:
//   attn_bwd_prep_bf16_kernel   one pass over go (fp32) and o (bf16): go16 and delta; C / 8 lanes own a row, fixed shuffle order.
//   attn_bwd_bf16_key_kernel    KEY-stationary: a wave owns 32 keys -- their K and V fragments in registers for the whole kernel, their
//                               gv^T [C x 32] and key-side gq^T [D x 32] in accumulators -- and the workgroup (4 waves, 128 keys) sweeps
//                               all queries, 64 per stage.  Writes gv and the key-side half of gq with plain stores.
//   attn_bwd_bf16_query_kernel  QUERY-stationary, the forward's mapping: a wave owns 32 queries (Q and go fragments in registers, -lse and
//                               -delta one scalar per lane) and sweeps all keys, 64 per stage.  Adds the query-side half to what the
//                               key launch stored: a stream-ordered read-modify-write by the one owner of the row.
// Both keep the stationary index on the MFMA lane column, so that S and dP (chains that START at -lse and -delta) leave their MFMAs in
// exactly the register order the next product's B operand has -- P and dS never touch LDS (the forward's trick, both ways round).
// The streamed index lives in LDS: one image per tile, read by rows (ds_read_b128: A of the S / dP products) AND transposed
// (ds_read_b64_tr_b16: A of the gv^T / gq^T products).  Global -> registers -> LDS as 16-byte chunks, double buffered, one barrier a stage.
// S and dP are computed in both sweeps: (D + C + C + D) + (D + C + D) = 1024 MACs per (query, key) pair at (64, 256) against 704 in one
// pass -- the price of not summing gq across workgroups.
#include "bf16x8.h"
#include "x6.h"

typedef __attribute__((address_space(3))) unsigned char* bwd_lds_ptr;
typedef __attribute__((address_space(3))) bf16x8_t* bwd_lp8;
typedef short bwd_s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bwd_s16x4_t* bwd_lp4;

// A fragment read by rows: lane (l31, lh) of the caller has put row l31, byte 16 lh into `ad`
__device__ __forceinline__ bf16x8_t bwd_row_frag(uint32_t ad) { return *(bwd_lp8)(uintptr_t)ad; }
// A fragment read transposed from 16 rows x 32 columns at `ad` (which carries the caller's lane term, see bwd_tr_lane): row = column
// l31 of the image, k-slot j of half lh = image row 8 (j >> 2) + 4 lh + (j & 3) -- the order the S^T / dP^T accumulator registers have
__device__ __forceinline__ bf16x8_t bwd_tr_frag(uint32_t ad, int pitch) {
  union {
    bwd_s16x4_t h[2];
    bf16x8_t v;
  } f;
  f.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bwd_lp4)(uintptr_t)ad);
  f.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bwd_lp4)(uintptr_t)(ad + 8 * pitch));
  return f.v;
}
// lane 4 q + p of a 16-lane group addresses image row q (+ 4 lh), elements 4 p .. 4 p + 3 of the group's 16 columns
__device__ __forceinline__ uint32_t bwd_tr_lane(int lane, int pitch) {
  const int i16 = lane & 15, lh = lane >> 5;
  return (uint32_t)((4 * lh + (i16 >> 2)) * pitch + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2);
}
// registers 8 s .. 8 s + 7 of an accumulator tile as the B operand of k-step s, rounded to bf16 (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x8_t bwd_pack(const f32x16& a, int s) {
  u32x4_t w;
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = cvt_pk_bf16(a[8 * s + 2 * e], a[8 * s + 2 * e + 1]);
  return __builtin_bit_cast(bf16x8_t, w);
}

// ---- go16 = bf16(go), delta = rowsum(go o float(o)) ----
template <int C>
__global__ void __launch_bounds__(256) attn_bwd_prep_bf16_kernel(const float* __restrict__ go, const uint16_t* __restrict__ o,
                                                                 uint16_t* __restrict__ go16, float* __restrict__ delta, int64_t rows) {
  constexpr int LPR = C / 8;  // lanes per row, 8 channels each
  const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // whole rows: the LPR lanes of a row leave together
  const int ch = threadIdx.x % LPR;
  float g[8], of[8];
  bf_load8f(go + row * C + 8 * ch, g);
  bf_unpack8(*reinterpret_cast<const uint4*>(o + row * C + 8 * ch), of);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s = fmaf(g[e], of[e], s);
  *reinterpret_cast<uint4*>(go16 + row * C + 8 * ch) = bf_pack8_hw(g);
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (ch == 0) delta[row] = s;
}

// dynamic LDS of the two sweeps: two stages of 64 streamed rows.  Pitches: an image that is read by rows only takes 16 bytes of padding,
// one that is (also) read transposed takes the forward's V padding of 64 on wide rows
template <int D, int NCT>
constexpr int attn_bwd_bf16_key_lds = 2 * (64 * ((2 * D + 16) + (2 * NCT * 32 + 64)) + 2 * 64 * 4);
template <int D, int NCT>
constexpr int attn_bwd_bf16_query_lds = 2 * 64 * ((2 * D + 16) + (2 * NCT * 32 + 16));

// ---- key-stationary sweep: gv and the key-side half of gq ----
template <int D, int NCT>
__global__ void __launch_bounds__(256, 1) attn_bwd_bf16_key_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ v,
                                                                   const uint16_t* __restrict__ go, const float* __restrict__ lse,
                                                                   const float* __restrict__ delta, float* __restrict__ gq,
                                                                   float* __restrict__ gv, int T) {
  constexpr int CT = NCT * 32, ROWS = 64, NTH = 256;
  constexpr int QP = 2 * D + 16, GP = 2 * CT + 64;          // row pitches (bytes) of the streamed Q and go images
  constexpr int QBYTES = ROWS * QP, GBYTES = ROWS * GP, STAGE = QBYTES + GBYTES + 2 * ROWS * 4;  // ... + (-lse) and (-delta) of the rows
  constexpr int QCH = ROWS * D / 8, GCH = ROWS * CT / 8;    // 16-byte chunks of a tile
  constexpr int NQL = (QCH + NTH - 1) / NTH, NGL = GCH / NTH;
  static_assert(GCH % NTH == 0 && (QCH % NTH == 0 || QCH < NTH), "whole 16-byte passes over the tiles");
  static_assert(D % 32 == 0, "whole accumulator tiles of the key-side gq");
  static_assert(2 * STAGE == attn_bwd_bf16_key_lds<D, NCT>, "the host passes the bytes this carve ends at");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_bwd[];  // [2][STAGE]
  const uint32_t lds0 = (uint32_t)(uintptr_t)(bwd_lds_ptr)smem_bwd;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y;
  const int k0 = blockIdx.x * 128 + wid * 32;               // this wave's keys
  const uint16_t* qb = q + (int64_t)n * T * D;
  const uint16_t* gb = go + (int64_t)n * T * CT;
  const float* lb = lse + (int64_t)n * T;
  const float* db = delta + (int64_t)n * T;

  // this lane's key: B[k = d][col = key] of S = Q K^T and B[k = c][col = key] of dP = go V^T, element 16 kk + 8 lh + j
  bf16x8_t kf[D / 16], vf[CT / 16];
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk)
    kf[kk] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(k0 + l31) * D + 16 * kk + 8 * lh));
#pragma unroll
  for (int kk = 0; kk < CT / 16; ++kk)
    vf[kk] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(v + ((int64_t)n * T + k0 + l31) * CT + 16 * kk + 8 * lh));

  f32x16 accv[NCT], accq[D / 32];  // gv^T [c][key] and key-side gq^T [d][key]
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) accv[c][r] = 0.f;
#pragma unroll
  for (int c = 0; c < D / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) accq[c][r] = 0.f;

  u32x4_t rq[NQL], rg[NGL];
  float rs = 0.f;
  auto gload = [&](int i0) {
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + NTH * i;
      rq[i] = (f < QCH) ? *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(i0 + f / (D / 8)) * D + 8 * (f % (D / 8))) : u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < NGL; ++i) {
      const int f = tid + NTH * i;
      rg[i] = *reinterpret_cast<const u32x4_t*>(gb + (int64_t)(i0 + f / (CT / 8)) * CT + 8 * (f % (CT / 8)));
    }
    if (tid < 2 * ROWS) rs = -(tid < ROWS ? lb[i0 + tid] : db[i0 + tid - ROWS]);  // the S and dP chains start at these
  };
  auto lstore = [&](int st) {
    unsigned char* base = smem_bwd + st * STAGE;
#pragma unroll
    for (int i = 0; i < NQL; ++i) {
      const int f = tid + NTH * i;
      if (f < QCH) *reinterpret_cast<u32x4_t*>(base + (f / (D / 8)) * QP + (f % (D / 8)) * 16) = rq[i];
    }
#pragma unroll
    for (int i = 0; i < NGL; ++i) {
      const int f = tid + NTH * i;
      *reinterpret_cast<u32x4_t*>(base + QBYTES + (f / (CT / 8)) * GP + (f % (CT / 8)) * 16) = rg[i];
    }
    if (tid < 2 * ROWS) *reinterpret_cast<float*>(base + QBYTES + GBYTES + 4 * tid) = rs;
  };
  const uint32_t qrow = (uint32_t)(l31 * QP + 16 * lh), grow = (uint32_t)(l31 * GP + 16 * lh);
  const uint32_t qtr = bwd_tr_lane(lane, QP), gtr = bwd_tr_lane(lane, GP);

  gload(0);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int i0 = 0; i0 < T; i0 += ROWS) {
    gload(i0 + ROWS < T ? i0 + ROWS : i0);  // unconditional prefetch (the last iteration re-reads its own tile)
    const uint32_t qimg = lds0 + (uint32_t)(buf * STAGE), gimg = qimg + QBYTES;
    const float* rowc = reinterpret_cast<const float*>(smem_bwd + buf * STAGE + QBYTES + GBYTES);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // S[query][key] and dP[query][key] for 32 queries x this wave's 32 keys; register r of half lh is query 32 u + (r & 3) + 8 (r >> 2) + 4 lh
      f32x16 s, dp;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(rowc + 32 * u + 8 * g + 4 * lh);
        const float4 b = *reinterpret_cast<const float4*>(rowc + ROWS + 32 * u + 8 * g + 4 * lh);
        s[4 * g] = a.x, s[4 * g + 1] = a.y, s[4 * g + 2] = a.z, s[4 * g + 3] = a.w;
        dp[4 * g] = b.x, dp[4 * g + 1] = b.y, dp[4 * g + 2] = b.z, dp[4 * g + 3] = b.w;
      }
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_row_frag(qimg + qrow + (uint32_t)(u * 32 * QP + kk * 32)), kf[kk], s, 0, 0, 0);
#pragma unroll
      for (int kk = 0; kk < CT / 16; ++kk)
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_row_frag(gimg + grow + (uint32_t)(u * 32 * GP + kk * 32)), vf[kk], dp, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __expf(s[r]);   // P
        dp[r] *= s[r];         // dS
      }
      // gv^T[c][key] += go^T[c][query] P[query][key],  gq^T[d][key] += Q^T[d][query] dS[query][key]: k-slot j of k-step s2 is query
      // 32 u + 16 s2 + 8 (j >> 2) + 4 lh + (j & 3), the order the registers already have
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t pp = bwd_pack(s, s2), dd = bwd_pack(dp, s2);
#pragma unroll
        for (int c = 0; c < NCT; ++c)
          accv[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_tr_frag(gimg + gtr + (uint32_t)((32 * u + 16 * s2) * GP + 64 * c), GP), pp, accv[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < D / 32; ++c)
          accq[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_tr_frag(qimg + qtr + (uint32_t)((32 * u + 16 * s2) * QP + 64 * c), QP), dd, accq[c], 0, 0, 0);
      }
    }
    lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // register r of tile c is channel 32 c + (r & 3) + 8 (r >> 2) + 4 lh of key k0 + l31: four consecutive channels per store
  const int64_t row = (int64_t)n * T + k0 + l31;
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(gv + row * CT + 32 * c + 8 * g + 4 * lh) = make_float4(accv[c][4 * g], accv[c][4 * g + 1], accv[c][4 * g + 2], accv[c][4 * g + 3]);
#pragma unroll
  for (int c = 0; c < D / 32; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(gq + row * D + 32 * c + 8 * g + 4 * lh) = make_float4(accq[c][4 * g], accq[c][4 * g + 1], accq[c][4 * g + 2], accq[c][4 * g + 3]);
}

// ---- query-stationary sweep: gq += the query-side half ----
template <int D, int NCT>
__global__ void __launch_bounds__(256, 1) attn_bwd_bf16_query_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ v,
                                                                     const uint16_t* __restrict__ go, const float* __restrict__ lse,
                                                                     const float* __restrict__ delta, float* __restrict__ gq, int T) {
  constexpr int CT = NCT * 32, KEYS = 64, NTH = 256;
  constexpr int KP = 2 * D + 16, VP = 2 * CT + 16;          // K: rows and transposed; V: rows only
  constexpr int KBYTES = KEYS * KP, STAGE = KBYTES + KEYS * VP;
  constexpr int KCH = KEYS * D / 8, VCH = KEYS * CT / 8;
  constexpr int NKL = (KCH + NTH - 1) / NTH, NVL = VCH / NTH;
  static_assert(VCH % NTH == 0 && (KCH % NTH == 0 || KCH < NTH), "whole 16-byte passes over the tiles");
  static_assert(D % 32 == 0, "whole accumulator tiles of the query-side gq");
  static_assert(2 * STAGE == attn_bwd_bf16_query_lds<D, NCT>, "the host passes the bytes this carve ends at");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_bwd[];  // [2][STAGE]
  const uint32_t lds0 = (uint32_t)(uintptr_t)(bwd_lds_ptr)smem_bwd;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int n = blockIdx.y;
  const int q0 = blockIdx.x * 128 + wid * 32;               // this wave's queries
  const uint16_t* qb = q + (int64_t)n * T * D;
  const uint16_t* vb = v + (int64_t)n * T * CT;
  const int64_t row = (int64_t)n * T + q0 + l31;

  // this lane's query: B[k = d][col = query] of S^T = K Q^T and B[k = c][col = query] of dP^T = V go^T
  bf16x8_t qf[D / 16], gf[CT / 16];
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk)
    qf[kk] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(q0 + l31) * D + 16 * kk + 8 * lh));
#pragma unroll
  for (int kk = 0; kk < CT / 16; ++kk)
    gf[kk] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(go + row * CT + 16 * kk + 8 * lh));
  const float nl = -lse[row], nd = -delta[row];

  f32x16 acc[D / 32];  // query-side gq^T [d][query]
#pragma unroll
  for (int c = 0; c < D / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  u32x4_t rk[NKL], rv[NVL];
  auto gload = [&](int j0) {
#pragma unroll
    for (int i = 0; i < NKL; ++i) {
      const int f = tid + NTH * i;
      rk[i] = (f < KCH) ? *reinterpret_cast<const u32x4_t*>(qb + (int64_t)(j0 + f / (D / 8)) * D + 8 * (f % (D / 8))) : u32x4_t{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) {
      const int f = tid + NTH * i;
      rv[i] = *reinterpret_cast<const u32x4_t*>(vb + (int64_t)(j0 + f / (CT / 8)) * CT + 8 * (f % (CT / 8)));
    }
  };
  auto lstore = [&](int st) {
    unsigned char* base = smem_bwd + st * STAGE;
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
  const uint32_t krow = (uint32_t)(l31 * KP + 16 * lh), vrow = (uint32_t)(l31 * VP + 16 * lh);
  const uint32_t ktr = bwd_tr_lane(lane, KP);

  gload(0);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int j0 = 0; j0 < T; j0 += KEYS) {
    gload(j0 + KEYS < T ? j0 + KEYS : j0);  // unconditional prefetch (the last iteration re-reads its own tile)
    const uint32_t kimg = lds0 + (uint32_t)(buf * STAGE), vimg = kimg + KBYTES;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // S^T[key][query] and dP^T[key][query] for 32 keys x this wave's 32 queries; register r of half lh is key 32 u + (r & 3) + 8 (r >> 2) + 4 lh
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = nl, dp[r] = nd;
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_row_frag(kimg + krow + (uint32_t)(u * 32 * KP + kk * 32)), qf[kk], s, 0, 0, 0);
#pragma unroll
      for (int kk = 0; kk < CT / 16; ++kk)
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_row_frag(vimg + vrow + (uint32_t)(u * 32 * VP + kk * 32)), gf[kk], dp, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] *= __expf(s[r]);  // dS^T
      // gq^T[d][query] += K^T[d][key] dS^T[key][query]
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t dd = bwd_pack(dp, s2);
#pragma unroll
        for (int c = 0; c < D / 32; ++c)
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwd_tr_frag(kimg + ktr + (uint32_t)((32 * u + 16 * s2) * KP + 64 * c), KP), dd, acc[c], 0, 0, 0);
      }
    }
    lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // this wave is the only writer of its rows in this launch, and the key launch before it on the stream was the only one in that
#pragma unroll
  for (int c = 0; c < D / 32; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4* p = reinterpret_cast<float4*>(gq + row * D + 32 * c + 8 * g + 4 * lh);
      const float4 h = *p;
      *p = make_float4(h.x + acc[c][4 * g], h.y + acc[c][4 * g + 1], h.z + acc[c][4 * g + 2], h.w + acc[c][4 * g + 3]);
    }
}

static inline bool attn_bwd_bf16_shape(int N, int T, int D, int C) {
  return T % 128 == 0 && ((D == 64 && C == 256) || (D == 32 && C == 128)) && N <= 65535;
}

extern "C" int fmi_attention_bwd_prep_bf16(const float* go, const uint16_t* o, uint16_t* go16, float* delta, int N, int T, int D, int C,
                                           void* stream) {
  if (!go || !o || !go16 || !delta || N <= 0 || T <= 0 || D <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (!attn_bwd_bf16_shape(N, T, D, C)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)go | (uintptr_t)o | (uintptr_t)go16 | (uintptr_t)delta) & 15) != 0) return FMI_ERR_BAD_ARG;
  const int64_t rows = (int64_t)N * T;
  if (rows / (C == 256 ? 8 : 16) > 0x7fffffffLL) return FMI_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (C == 256)
    hipLaunchKernelGGL(attn_bwd_prep_bf16_kernel<256>, dim3((unsigned)(rows / 8)), dim3(256), 0, st, go, o, go16, delta, rows);
  else
    hipLaunchKernelGGL(attn_bwd_prep_bf16_kernel<128>, dim3((unsigned)(rows / 16)), dim3(256), 0, st, go, o, go16, delta, rows);
  return fmi_launch_status();
}

extern "C" int fmi_attention_bwd_bf16(const uint16_t* q, const uint16_t* v, const uint16_t* go16, const float* lse, const float* delta,
                                      float* gq, float* gv, int N, int T, int D, int C, void* stream) {
  if (!q || !v || !go16 || !lse || !delta || !gq || !gv || N <= 0 || T <= 0 || D <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (!attn_bwd_bf16_shape(N, T, D, C)) return FMI_ERR_UNSUPPORTED;
  if ((((uintptr_t)q | (uintptr_t)v | (uintptr_t)go16 | (uintptr_t)lse | (uintptr_t)delta | (uintptr_t)gq | (uintptr_t)gv) & 15) != 0)
    return FMI_ERR_BAD_ARG;
  const dim3 grid(T / 128, N), block(256);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (D == 64) {
    rc = fmi_launch_lds<attn_bwd_bf16_key_kernel<64, 8>>(grid, block, attn_bwd_bf16_key_lds<64, 8>, st, q, v, go16, lse, delta, gq, gv, T);
    if (rc == FMI_OK) rc = fmi_launch_lds<attn_bwd_bf16_query_kernel<64, 8>>(grid, block, attn_bwd_bf16_query_lds<64, 8>, st, q, v, go16, lse, delta, gq, T);
  } else {
    rc = fmi_launch_lds<attn_bwd_bf16_key_kernel<32, 4>>(grid, block, attn_bwd_bf16_key_lds<32, 4>, st, q, v, go16, lse, delta, gq, gv, T);
    if (rc == FMI_OK) rc = fmi_launch_lds<attn_bwd_bf16_query_kernel<32, 4>>(grid, block, attn_bwd_bf16_query_lds<32, 4>, st, q, v, go16, lse, delta, gq, T);
  }
  return rc != FMI_OK ? rc : fmi_launch_status();
}
