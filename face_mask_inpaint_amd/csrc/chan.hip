// Per-channel bandwidth kernels on NHWC activations, fp32 and bf16: the element-wise operations and their reductions between the
// convolutions and norms of the IR-SE50 body of the pSp encoder (modules/psp/encoders/helpers.py:56-119) and the modulation products of
// the StyleGAN2 decoder (stylegan2/model.py:244-252).
//   scale_channels      x * s[n][c]               SE gate, modulation / demodulation;  adjoints: _gs (sum_p g x), _bwd (gx and gs in one pass)
//   scale_channels_add  x * s[n][c] + res         SE gate + residual add of a bottleneck_IR_SE block in one pass
//   prelu               x > 0 ? x : a[c] x        and its backward (gx, ga)
//   add_bcast           g + gpool[n][c] / P       the SE input's two gradients meet in one pass
//   subsample           x[n][oy s][ox s]          MaxPool2d(1, stride) and its scatter
//   global_avgpool      mean_p x[n][p][c]         AdaptiveAvgPool2d(1) of the SE module (bf16; the fp32 one is pool.hip's)
//   add                 a + b                     residual add of a plain IR block (bf16)
// Element type T = float or uint16_t (bf16 as raw bits); parameters, gates and every reduction result stay fp32.  The forward kernels are
// written once on Chunk<T> (bf16x8.h): one thread moves 16 bytes = 4 floats or 8 bf16, computes in fp32 and stores with bf_round (the
// inputs are this library's own activations: finite).  The reductions keep one kernel per type: their summation orders differ, and
// the order is part of the result; so does subsample, for its speed.
#include "bf16x8.h"
#include "sum_parts.h"

template <typename T>
using vec_t = typename Chunk<T>::vec;

// ---- scale_channels: y[n][p][c] = x[n][p][c] * s[n][c] -----------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) scale_channels_kernel(const vec_t<T>* __restrict__ x, const float* __restrict__ s, vec_t<T>* __restrict__ y,
                                                             int64_t PCV, int CV, int64_t total) {
  constexpr int N = Chunk<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const int64_t n = i / PCV;
    float f[N], sc[N];
    Chunk<T>::widen(x[i], f);
    Chunk<T>::loadf(s + (n * CV + cv) * N, sc);
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] *= sc[e];
    y[i] = Chunk<T>::narrow(f);
  }
}
// one element per thread: a channel count that has no whole chunks, or (fp32) a pointer off a 16-byte boundary.  Not a hot path
template <typename T>
__global__ void __launch_bounds__(256) scale_channels_scalar_kernel(const T* __restrict__ x, const float* __restrict__ s, T* __restrict__ y, int64_t PC,
                                                                    int C, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t n = i / PC;
    bf_st(y, i, bf_ld(x, i) * s[n * C + c]);
  }
}
template <typename T>
static int scale_channels_impl(const T* x, const float* s, T* y, int N, int64_t P, int C, bool chunked, void* stream) {
  if (chunked) {
    const int CV = C / Chunk<T>::N;
    const int64_t total = (int64_t)N * P * CV;
    hipLaunchKernelGGL(scale_channels_kernel<T>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const vec_t<T>*)x, s,
                       (vec_t<T>*)y, P * CV, CV, total);
  } else {
    const int64_t total = (int64_t)N * P * C;
    hipLaunchKernelGGL(scale_channels_scalar_kernel<T>, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, s, y, P * C, C, total);
  }
  return fmi_launch_status();
}
// fp32: anything that is not whole aligned chunks goes to the scalar kernel
extern "C" int fmi_scale_channels_f32(const float* x, const float* s, float* y, int N, int64_t P, int C, void* stream) {
  if (!x || !s || !y || N <= 0 || P <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  return scale_channels_impl<float>(x, s, y, N, P, C, C % 4 == 0 && fmi_al16(x) && fmi_al16(y) && fmi_al16(s), stream);
}
// bf16: the scalar kernel only for C % 8 != 0 (so that the op is defined for every channel count its fp32 twin takes); a misaligned pointer is refused
extern "C" int fmi_scale_channels_bf16(const uint16_t* x, const float* s, uint16_t* y, int N, int64_t P, int C, void* stream) {
  if (!x || !s || !y || N <= 0 || P <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 == 0 && (!fmi_al16(x) || !fmi_al16(y) || !fmi_al16(s))) return FMI_ERR_UNSUPPORTED;
  return scale_channels_impl<uint16_t>(x, s, y, N, P, C, C % 8 == 0, stream);
}

// ---- scale_channels_add: y = x * s[n][c] + res (helpers.py:64-72,116-118) -------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) scale_channels_add_kernel(const vec_t<T>* __restrict__ x, const float* __restrict__ s,
                                                                 const vec_t<T>* __restrict__ res, vec_t<T>* __restrict__ y, int64_t PCV, int CV,
                                                                 int64_t total) {
  constexpr int N = Chunk<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const int64_t n = i / PCV;
    float f[N], sc[N], r[N];
    Chunk<T>::widen(x[i], f);
    Chunk<T>::widen(res[i], r);
    Chunk<T>::loadf(s + (n * CV + cv) * N, sc);
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] = f[e] * sc[e] + r[e];
    y[i] = Chunk<T>::narrow(f);
  }
}
template <typename T>
static int scale_channels_add_impl(const T* x, const float* s, const T* res, T* y, int N, int64_t P, int C, void* stream) {
  if (!x || !s || !res || !y || N <= 0 || P <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % Chunk<T>::N != 0 || !fmi_al16(x) || !fmi_al16(y) || !fmi_al16(s) || !fmi_al16(res)) return FMI_ERR_UNSUPPORTED;
  const int CV = C / Chunk<T>::N;
  const int64_t total = (int64_t)N * P * CV;
  hipLaunchKernelGGL(scale_channels_add_kernel<T>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const vec_t<T>*)x, s,
                     (const vec_t<T>*)res, (vec_t<T>*)y, P * CV, CV, total);
  return fmi_launch_status();
}
extern "C" int fmi_scale_channels_add_f32(const float* x, const float* s, const float* res, float* y, int N, int64_t P, int C, void* stream) {
  return scale_channels_add_impl<float>(x, s, res, y, N, P, C, stream);
}
extern "C" int fmi_scale_channels_add_bf16(const uint16_t* x, const float* s, const uint16_t* res, uint16_t* y, int N, int64_t P, int C, void* stream) {
  return scale_channels_add_impl<uint16_t>(x, s, res, y, N, P, C, stream);
}

// ---- the adjoints of scale_channels ----------------------------------------------------------------------------------------
// gs[n][c] = sum_p g[n][p][c] * x[n][p][c].  With a partials workspace (ws_floats >= N*C) every row block stores its sums as one row
// and a second launch adds the rows (gs WRITTEN); without one the blocks add onto the caller-zeroed gs with fp32 atomics, which
// serialise per address (52 us per launch on the SE gates of the pSp encoder).
__global__ void __launch_bounds__(256) scale_channels_gs_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                float* __restrict__ gs, int64_t P, int C, int64_t rows_per_block,
                                                                int to_parts) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > P) r1 = P;
  const float* gb = g + (int64_t)n * P * C;
  const float* xb = x + (int64_t)n * P * C;
  float* dst = to_parts ? gs + ((int64_t)n * gridDim.x + blockIdx.x) * C : gs + (int64_t)n * C;
  for (int cg = 0; cg < C; cg += 64) {
    const int c = cg + tx;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
      int64_t r = r0 + ty;
      for (; r + 4 < r1; r += 8) {  // two independent pairs of loads in flight
        const float a0 = gb[r * C + c], b0 = xb[r * C + c], a1 = gb[(r + 4) * C + c], b1 = xb[(r + 4) * C + c];
        s0 = fmaf(a0, b0, s0), s1 = fmaf(a1, b1, s1);
      }
      for (; r < r1; r += 4) s0 = fmaf(gb[r * C + c], xb[r * C + c], s0);
    }
    part[ty][tx] = s0 + s1;
    __syncthreads();
    if (ty == 0 && c < C) {
      const float t = part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx];
      if (to_parts) dst[c] = t;
      else atomicAdd(dst + c, t);
    }
    __syncthreads();
  }
}
// out[n][c] = sum_{b < nparts} ws[(n * nparts + b) * C + c]
__global__ void __launch_bounds__(256) scale_channels_gs_finish_kernel(const float* __restrict__ ws, float* __restrict__ out, int nparts, int C,
                                                                       int total) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int n = t / C, c = t - n * C;
  const float* p = ws + (int64_t)n * nparts * C + c;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int q = 0;
  for (; q + 3 < nparts; q += 4) a0 += p[(int64_t)q * C], a1 += p[(int64_t)(q + 1) * C], a2 += p[(int64_t)(q + 2) * C], a3 += p[(int64_t)(q + 3) * C];
  for (; q < nparts; ++q) a0 += p[(int64_t)q * C];
  out[t] = (a0 + a1) + (a2 + a3);
}
extern "C" int fmi_scale_channels_gs_f32(const float* g, const float* x, float* gs, float* ws, int64_t ws_floats, int N, int64_t P, int C,
                                         void* stream) {
  if (!g || !x || !gs || N <= 0 || P <= 0 || C <= 0 || N > 65535) return FMI_ERR_BAD_ARG;
  const bool parts = ws && ws_floats >= (int64_t)N * C;
  int64_t blocks = ceil_div64(P, 128);
  int64_t cap = parts ? ws_floats / ((int64_t)N * C) : 1024;
  const int64_t want = ceil_div64(2048, N);
  if (parts && cap > want) cap = want;
  if (blocks > cap) blocks = cap;
  if (fmi_det() && !parts) blocks = 1;  // reproducible mode without a partials workspace: one block per sample
  const int64_t rpb = ceil_div64(P, blocks);
  blocks = ceil_div64(P, rpb);
  hipLaunchKernelGGL(scale_channels_gs_kernel, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, g, x, parts ? ws : gs, P, C, rpb,
                     parts ? 1 : 0);
  if (parts)
    hipLaunchKernelGGL(scale_channels_gs_finish_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, gs, (int)blocks, C,
                       N * C);
  return fmi_launch_status();
}

// Both gradients of y = x * s[n][c] in ONE pass over g and x: gx = g * s (written) and gs[n][c] = sum_p g * x (row-block partials in ws,
// then the adding launch above) -- the SE gate of every IR-SE block, the modulation / demodulation products of the fp32 decoder.  Two
// launches read g twice, and the gs kernel used 4-byte loads (2.3 TB/s).  A thread keeps one 4-channel group; C % 4 == 0, C / 4 <= 256.
__global__ void __launch_bounds__(256) scale_channels_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ x,
                                                                 const float* __restrict__ s, float4* __restrict__ gx, float* __restrict__ ws,
                                                                 int64_t P, int C4, int64_t rows_per_block) {
  __shared__ float part[256][4];
  const int RL = 256 / C4, cg = threadIdx.x % C4, rl = threadIdx.x / C4;
  const int n = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > P) r1 = P;
  const float4* gb = g + (int64_t)n * P * C4;
  const float4* xb = x + (int64_t)n * P * C4;
  float4* ob = gx + (int64_t)n * P * C4;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (rl < RL) {
    const float4 sv = *reinterpret_cast<const float4*>(s + ((int64_t)n * C4 + cg) * 4);
    auto one = [&](int64_t r, const float4 gv, const float4 xv) {
      a[0] = fmaf(gv.x, xv.x, a[0]), a[1] = fmaf(gv.y, xv.y, a[1]), a[2] = fmaf(gv.z, xv.z, a[2]), a[3] = fmaf(gv.w, xv.w, a[3]);
      ob[r * C4 + cg] = make_float4(gv.x * sv.x, gv.y * sv.y, gv.z * sv.z, gv.w * sv.w);
    };
    int64_t r = r0 + rl;
    for (; r + RL < r1; r += 2 * RL) {  // two independent pairs of 16-byte loads in flight
      const float4 g0 = gb[r * C4 + cg], x0 = xb[r * C4 + cg], g1 = gb[(r + RL) * C4 + cg], x1 = xb[(r + RL) * C4 + cg];
      one(r, g0, x0);
      one(r + RL, g1, x1);
    }
    for (; r < r1; r += RL) one(r, gb[r * C4 + cg], xb[r * C4 + cg]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[threadIdx.x][e] = a[e];
  __syncthreads();
  if ((int)threadIdx.x < C4) {
    float t[4] = {part[threadIdx.x][0], part[threadIdx.x][1], part[threadIdx.x][2], part[threadIdx.x][3]};
    for (int l = 1; l < RL; ++l)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += part[l * C4 + cg][e];
    *reinterpret_cast<float4*>(ws + ((int64_t)n * gridDim.x + blockIdx.x) * C4 * 4 + cg * 4) = make_float4(t[0], t[1], t[2], t[3]);
  }
}
/* gx = g * s[n][c] and gs[n][c] = sum_p g * x in one pass (the adjoint of fmi_scale_channels_f32 / the product part of
 * fmi_scale_channels_add_f32).  ws: >= N * C floats of scratch (more = more row blocks). */
extern "C" int fmi_scale_channels_bwd_f32(const float* g, const float* x, const float* s, float* gx, float* gs, float* ws, int64_t ws_floats, int N,
                                          int64_t P, int C, void* stream) {
  if (!g || !x || !s || !gx || !gs || !ws || N <= 0 || P <= 0 || C <= 0 || N > 65535 || ws_floats < (int64_t)N * C) return FMI_ERR_BAD_ARG;
  if (C % 4 != 0 || C / 4 > 256 || (((uintptr_t)g | (uintptr_t)x | (uintptr_t)s | (uintptr_t)gx | (uintptr_t)ws) & 15)) return FMI_ERR_UNSUPPORTED;
  int64_t blocks = ceil_div64(P, 64);
  int64_t cap = ws_floats / ((int64_t)N * C);
  const int64_t want = ceil_div64(4096, N);
  if (cap > want) cap = want;
  if (blocks > cap) blocks = cap;
  const int64_t rpb = ceil_div64(P, blocks);
  blocks = ceil_div64(P, rpb);
  hipLaunchKernelGGL(scale_channels_bwd_kernel, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (const float4*)x, s,
                     (float4*)gx, ws, P, C / 4, rpb);
  hipLaunchKernelGGL(scale_channels_gs_finish_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, gs, (int)blocks, C, N * C);
  return fmi_launch_status();
}
// gs[n][c] = sum_p g[n][p][c] * x[n][p][c]   (written, not accumulated; ws: partials workspace of >= N*C floats)
__global__ void __launch_bounds__(256) scale_channels_gs_bf16_kernel(const uint4* __restrict__ g, const uint4* __restrict__ x,
                                                                     float* __restrict__ ws, int64_t P, int C8, int64_t rows_per_block) {
  __shared__ float part[256][8];
  const int RL = 256 / C8, cg = threadIdx.x % C8, rl = threadIdx.x / C8;
  const int n = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > P) r1 = P;
  const uint4* gb = g + (int64_t)n * P * C8;
  const uint4* xb = x + (int64_t)n * P * C8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int64_t r = r0 + rl;
  for (; r + RL < r1; r += 2 * RL) {  // two independent pairs of 16-byte loads in flight
    float a[8], b[8], a2[8], b2[8];
    const uint4 ga = gb[r * C8 + cg], xa = xb[r * C8 + cg], gc = gb[(r + RL) * C8 + cg], xc = xb[(r + RL) * C8 + cg];
    bf_unpack8(ga, a), bf_unpack8(xa, b), bf_unpack8(gc, a2), bf_unpack8(xc, b2);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(a2[e], b2[e], fmaf(a[e], b[e], acc[e]));
  }
  for (; r < r1; r += RL) {
    float a[8], b[8];
    bf_unpack8(gb[r * C8 + cg], a);
    bf_unpack8(xb[r * C8 + cg], b);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(a[e], b[e], acc[e]);
  }
  chunk_reduce_store(acc, ws + ((int64_t)n * gridDim.x + blockIdx.x) * C8 * 8, C8, part);
}
// C % 8 != 0: one workgroup per (64-channel stripe, sample), four row lanes combined in a fixed order; gs WRITTEN, no workspace.  A long
// walk per thread (P / 4 rows): for the odd widths of small side networks, not for a body layer
__global__ void __launch_bounds__(256) scale_channels_gs_bf16_scalar_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ x,
                                                                            float* __restrict__ gs, int64_t P, int C) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx, n = blockIdx.y;
  float acc = 0.f;
  if (c < C)
    for (int64_t r = ty; r < P; r += 4) {
      const int64_t o = ((int64_t)n * P + r) * C + c;
      acc = fmaf(bf_lo(g[o]), bf_lo(x[o]), acc);
    }
  part[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c < C) gs[(int64_t)n * C + c] = (part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]);
}
extern "C" int fmi_scale_channels_gs_bf16(const uint16_t* g, const uint16_t* x, float* gs, float* ws, int64_t ws_floats, int N, int64_t P,
                                          int C, void* stream) {
  if (!g || !x || !gs || N <= 0 || P <= 0 || C <= 0 || N > 65535) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0) {  // no eight-channel chunks: the scalar form, which takes no workspace (ws may be NULL)
    hipLaunchKernelGGL(scale_channels_gs_bf16_scalar_kernel, dim3((unsigned)((C + 63) / 64), N), dim3(256), 0, (hipStream_t)stream, g, x, gs, P, C);
    return fmi_launch_status();
  }
  if (!ws || ws_floats < (int64_t)N * C) return FMI_ERR_BAD_ARG;
  if (!c8_ok(C) || !fmi_al16(g) || !fmi_al16(x) || !fmi_al16(ws)) return FMI_ERR_UNSUPPORTED;
  int64_t blocks = parts_for(P, N, C, ws_floats);
  const int64_t rpb = ceil_div64(P, blocks);
  blocks = ceil_div64(P, rpb);
  hipLaunchKernelGGL(scale_channels_gs_bf16_kernel, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, (const uint4*)g,
                     (const uint4*)x, ws, P, C / 8, rpb);
  launch_sum_parts(ws, gs, (int)blocks, C, N, (hipStream_t)stream);
  return fmi_launch_status();
}

// ---- PReLU(C): y = x > 0 ? x : a[c] x -----------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) prelu_kernel(const vec_t<T>* __restrict__ x, const float* __restrict__ a, vec_t<T>* __restrict__ y, int64_t total,
                                                    int CV) {
  constexpr int N = Chunk<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float f[N], s[N];
    Chunk<T>::widen(x[i], f);
    Chunk<T>::loadf(a + (i % CV) * N, s);
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] = f[e] > 0.f ? f[e] : s[e] * f[e];
    y[i] = Chunk<T>::narrow(f);
  }
}
template <typename T>
static int prelu_impl(const T* x, const float* a, T* y, int64_t rows, int C, void* stream) {
  const int64_t total = rows * (C / Chunk<T>::N);
  hipLaunchKernelGGL(prelu_kernel<T>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const vec_t<T>*)x, a, (vec_t<T>*)y,
                     total, C / Chunk<T>::N);
  return fmi_launch_status();
}
// fp32 only: C % 4 != 0 or a pointer off a 16-byte boundary
__global__ void __launch_bounds__(256) prelu_scalar_kernel(const float* __restrict__ x, const float* __restrict__ a, float* __restrict__ y,
                                                           int64_t total, int C) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    y[i] = v > 0.f ? v : a[i % C] * v;
  }
}
extern "C" int fmi_prelu_f32(const float* x, const float* a, float* y, int64_t rows, int C, void* stream) {
  if (!x || !a || !y || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 4 == 0 && fmi_al16(x) && fmi_al16(y) && fmi_al16(a)) return prelu_impl<float>(x, a, y, rows, C, stream);
  const int64_t total = rows * C;
  hipLaunchKernelGGL(prelu_scalar_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, a, y, total, C);
  return fmi_launch_status();
}
extern "C" int fmi_prelu_bf16(const uint16_t* x, const float* a, uint16_t* y, int64_t rows, int C, void* stream) {
  if (!x || !a || !y || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(x) || !fmi_al16(y) || !fmi_al16(a)) return FMI_ERR_UNSUPPORTED;
  return prelu_impl<uint16_t>(x, a, y, rows, C, stream);
}
// gx = g * (x > 0 ? 1 : a[c]);  ga[c] += sum_rows g * x * (x <= 0)   (caller zeroes ga)
__global__ void __launch_bounds__(256) prelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                        const float* __restrict__ a, float* __restrict__ gx, float* __restrict__ ga,
                                                        int64_t rows, int C, int64_t rows_per_block) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int cg = 0; cg < C; cg += 64) {
    const int c = cg + tx;
    float s = 0.f;
    if (c < C) {
      const float ac = a[c];
      for (int64_t r = r0 + ty; r < r1; r += 4) {
        const float xv = x[r * C + c], gv = g[r * C + c];
        gx[r * C + c] = xv > 0.f ? gv : ac * gv;
        if (xv <= 0.f) s += gv * xv;
      }
    }
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < C) atomicAdd(ga + c, part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx]);
    __syncthreads();
  }
}
// 16-byte form (C/4 a power of two <= 256): 256 threads = (256 / C4) rows x C4 four-channel chunks per pass, two row passes in flight;
// the scalar kernel walked 64-channel stripes one after the other with a workgroup barrier each (47 us floor per launch)
__global__ void __launch_bounds__(256) prelu_bwd_vec_kernel(const float4* __restrict__ g, const float4* __restrict__ x,
                                                            const float4* __restrict__ a, float4* __restrict__ gx, float* __restrict__ ga,
                                                            int64_t rows, int C4, int64_t rows_per_block, int to_parts) {
  __shared__ float4 part[256];
  const int cg = threadIdx.x % C4, rl = threadIdx.x / C4, RL = 256 / C4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  const float4 ac = a[cg];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  auto one = [&](int64_t r, const float4 xv, const float4 gv) {
    float4 o;
    o.x = xv.x > 0.f ? gv.x : ac.x * gv.x, o.y = xv.y > 0.f ? gv.y : ac.y * gv.y;
    o.z = xv.z > 0.f ? gv.z : ac.z * gv.z, o.w = xv.w > 0.f ? gv.w : ac.w * gv.w;
    gx[r * C4 + cg] = o;
    if (xv.x <= 0.f) s.x += gv.x * xv.x;
    if (xv.y <= 0.f) s.y += gv.y * xv.y;
    if (xv.z <= 0.f) s.z += gv.z * xv.z;
    if (xv.w <= 0.f) s.w += gv.w * xv.w;
  };
  int64_t r = r0 + rl;
  for (; r + RL < r1; r += 2 * RL) {
    const float4 x0 = x[r * C4 + cg], g0 = g[r * C4 + cg], x1 = x[(r + RL) * C4 + cg], g1 = g[(r + RL) * C4 + cg];
    one(r, x0, g0);
    one(r + RL, x1, g1);
  }
  for (; r < r1; r += RL) one(r, x[r * C4 + cg], g[r * C4 + cg]);
  part[threadIdx.x] = s;
  __syncthreads();
  if ((int)threadIdx.x < C4) {
    float4 t = part[threadIdx.x];
    for (int l = 1; l < RL; ++l) {
      const float4 v = part[l * C4 + threadIdx.x];
      t.x += v.x, t.y += v.y, t.z += v.z, t.w += v.w;
    }
    if (to_parts) {  // ga = partials workspace: row blockIdx.x
      reinterpret_cast<float4*>(ga)[(int64_t)blockIdx.x * C4 + threadIdx.x] = t;
    } else {
      atomicAdd(ga + 4 * threadIdx.x + 0, t.x);
      atomicAdd(ga + 4 * threadIdx.x + 1, t.y);
      atomicAdd(ga + 4 * threadIdx.x + 2, t.z);
      atomicAdd(ga + 4 * threadIdx.x + 3, t.w);
    }
  }
}
extern "C" int fmi_prelu_bwd_f32(const float* g, const float* x, const float* a, float* gx, float* ga, float* ws, int64_t ws_floats,
                                 int64_t rows, int C, void* stream) {
  if (!g || !x || !a || !gx || !ga || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  const int C4 = C / 4;
  if (C % 4 == 0 && C4 <= 256 && (C4 & (C4 - 1)) == 0 && ((((uintptr_t)g) | ((uintptr_t)x) | ((uintptr_t)gx) | ((uintptr_t)a)) & 15) == 0) {
    const bool parts = ws && ws_floats >= C && (((uintptr_t)ws) & 15) == 0;
    int64_t blocks = ceil_div64(rows, 64);
    const int64_t cap = parts ? (ws_floats / C < 1024 ? ws_floats / C : 1024) : 256;  // atomics on C addresses serialise: few blocks
    if (blocks > cap) blocks = cap;
    if (fmi_det() && !parts) blocks = 1;  // reproducible mode without a partials workspace
    const int64_t rpb = ceil_div64(rows, blocks);
    blocks = ceil_div64(rows, rpb);
    hipLaunchKernelGGL(prelu_bwd_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (const float4*)x,
                       (const float4*)a, (float4*)gx, parts ? ws : ga, rows, C4, rpb, parts ? 1 : 0);
    if (parts) launch_sum_parts<float>(ws, ga, (int)blocks, C, 1, (hipStream_t)stream);
    return fmi_launch_status();
  }
  int64_t blocks = ceil_div64(rows, 128);
  if (blocks > 2048) blocks = 2048;
  if (fmi_det()) blocks = 1;  // reproducible mode
  const int64_t rpb = ceil_div64(rows, blocks);
  blocks = ceil_div64(rows, rpb);
  hipLaunchKernelGGL(prelu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, x, a, gx, ga, rows, C, rpb);
  return fmi_launch_status();
}
// gx = g (x > 0 ? 1 : a[c]);  ga[c] = sum_rows g x (x <= 0): every block stores its sums as one row of the partials workspace,
// a second launch adds the rows (ga WRITTEN)
__global__ void __launch_bounds__(256) prelu_bwd_bf16_kernel(const uint4* __restrict__ g, const uint4* __restrict__ x, const float* __restrict__ a,
                                                             uint4* __restrict__ gx, float* __restrict__ parts, int64_t rows, int C8,
                                                             int64_t rows_per_block) {
  __shared__ float part[256 * 8];
  const int cg = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  float ac[8], s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (rl < RL) {
    bf_load8f(a + cg * 8, ac);
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      float xv[8], gv[8], o[8];
      bf_unpack8(x[r * C8 + cg], xv);
      bf_unpack8(g[r * C8 + cg], gv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        o[e] = xv[e] > 0.f ? gv[e] : ac[e] * gv[e];
        if (xv[e] <= 0.f) s[e] += gv[e] * xv[e];
      }
      gx[r * C8 + cg] = bf_pack8(o);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[threadIdx.x * 8 + e] = s[e];
  __syncthreads();
  if ((int)threadIdx.x < C8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
      for (int l = 0; l < RL; ++l) t += part[(l * C8 + threadIdx.x) * 8 + e];
      parts[((int64_t)blockIdx.x * C8 + threadIdx.x) * 8 + e] = t;
    }
  }
}
__global__ void __launch_bounds__(256) sum_rows_f32_kernel(const float* __restrict__ ws, float* __restrict__ out, int nparts, int width, float scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= width) return;
  float t = 0.f;
  for (int q = 0; q < nparts; ++q) t += ws[(int64_t)q * width + i];
  out[i] = t * scale;
}
extern "C" int fmi_prelu_bwd_bf16(const uint16_t* g, const uint16_t* x, const float* a, uint16_t* gx, float* ga, float* ws, int64_t ws_floats,
                                  int64_t rows, int C, void* stream) {
  if (!g || !x || !a || !gx || !ga || !ws || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  const int C8 = C / 8;
  if (C % 8 != 0 || C8 > 256 || (C8 & (C8 - 1)) != 0 || !fmi_al16(g) || !fmi_al16(x) || !fmi_al16(gx) || !fmi_al16(a) || ws_floats < C) return FMI_ERR_UNSUPPORTED;
  int64_t blocks = ceil_div64(rows, 64);
  const int64_t cap = ws_floats / C < 512 ? ws_floats / C : 512;
  if (blocks > cap) blocks = cap;
  const int64_t rpb = ceil_div64(rows, blocks);
  blocks = ceil_div64(rows, rpb);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(prelu_bwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)g, (const uint4*)x, a, (uint4*)gx, ws, rows, C8, rpb);
  hipLaunchKernelGGL(sum_rows_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)ws, ga, (int)blocks, C, 1.f);
  return fmi_launch_status();
}

// ---- add_bcast: gx = g + gpool[n][c] / P.  The SE input's two gradients -- through the gated product (g) and through the global
// average pool (gpool) -- meet in one pass instead of a pool-backward pass plus an accumulation pass of the autograd engine ----
template <typename T>
__global__ void __launch_bounds__(256) add_bcast_kernel(const vec_t<T>* __restrict__ g, const float* __restrict__ gpool, vec_t<T>* __restrict__ gx,
                                                        int64_t PCV, int CV, int64_t total, float inv) {
  constexpr int N = Chunk<T>::N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const int64_t n = i / PCV;
    float f[N], p[N];
    Chunk<T>::widen(g[i], f);
    Chunk<T>::loadf(gpool + (n * CV + cv) * N, p);
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] += p[e] * inv;
    gx[i] = Chunk<T>::narrow(f);
  }
}
template <typename T>
static int add_bcast_impl(const T* g, const float* gpool, T* gx, int N, int64_t P, int C, void* stream) {
  if (!g || !gpool || !gx || N <= 0 || P <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % Chunk<T>::N != 0 || !fmi_al16(g) || !fmi_al16(gx) || !fmi_al16(gpool)) return FMI_ERR_UNSUPPORTED;
  const int CV = C / Chunk<T>::N;
  const int64_t total = (int64_t)N * P * CV;
  hipLaunchKernelGGL(add_bcast_kernel<T>, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const vec_t<T>*)g, gpool,
                     (vec_t<T>*)gx, P * CV, CV, total, 1.f / (float)P);
  return fmi_launch_status();
}
extern "C" int fmi_add_bcast_f32(const float* g, const float* gpool, float* gx, int N, int64_t P, int C, void* stream) {
  return add_bcast_impl<float>(g, gpool, gx, N, P, C, stream);
}
extern "C" int fmi_add_bcast_bf16(const uint16_t* g, const float* gpool, uint16_t* gx, int N, int64_t P, int C, void* stream) {
  return add_bcast_impl<uint16_t>(g, gpool, gx, N, P, C, stream);
}

// ---- subsample: y[n][oy][ox] = x[n][oy s][ox s] (MaxPool2d(kernel 1, stride s)); backward scatters into zeros.  Bytes only, no arithmetic.
// One kernel per type: a shared one (templated on the unit it moves) cost the fp32 scatter 2 % at 16 x 128 x 128 x 64 (profiles/chan_refactor.txt) ----
__global__ void __launch_bounds__(256) subsample_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C,
                                                        int OH, int OW, int s, int64_t total, int backward) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    int64_t r = i / C;
    if (!backward) {  // i indexes y
      const int ox = (int)(r % OW);
      r /= OW;
      const int oy = (int)(r % OH);
      const int64_t n = r / OH;
      y[i] = x[((n * H + (int64_t)oy * s) * W + (int64_t)ox * s) * C + c];
    } else {          // i indexes gx (= y argument), x argument = gy
      const int xx = (int)(r % W);
      r /= W;
      const int yy = (int)(r % H);
      const int64_t n = r / H;
      const bool hit = (yy % s == 0) && (xx % s == 0) && (yy / s < OH) && (xx / s < OW);
      y[i] = hit ? x[((n * OH + yy / s) * OW + xx / s) * C + c] : 0.f;
    }
  }
}
extern "C" int fmi_subsample_f32(const float* x, float* y, int N, int H, int W, int C, int stride, int backward, void* stream) {
  if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || stride <= 0) return FMI_ERR_BAD_ARG;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const int64_t total = backward ? (int64_t)N * H * W * C : (int64_t)N * OH * OW * C;
  hipLaunchKernelGGL(subsample_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, OH, OW, stride,
                     total, backward);
  return fmi_launch_status();
}
__global__ void __launch_bounds__(256) subsample_bf16_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int H, int W, int C8, int OH, int OW,
                                                             int s, int64_t total, int backward) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C8);
    int64_t r = i / C8;
    if (!backward) {  // i indexes y
      const int ox = (int)(r % OW);
      r /= OW;
      const int oy = (int)(r % OH);
      const int n = (int)(r / OH);
      y[i] = x[(((int64_t)n * H + oy * s) * W + ox * s) * C8 + c];
    } else {  // i indexes gx (= y here, of extent H x W); x is the small gradient
      const int xx = (int)(r % W);
      r /= W;
      const int yy = (int)(r % H);
      const int n = (int)(r / H);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (yy % s == 0 && xx % s == 0 && yy / s < OH && xx / s < OW) v = x[(((int64_t)n * OH + yy / s) * OW + xx / s) * C8 + c];
      y[i] = v;
    }
  }
}
extern "C" int fmi_subsample_bf16(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int stride, int backward, void* stream) {
  if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || stride <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(x) || !fmi_al16(y)) return FMI_ERR_UNSUPPORTED;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const int64_t total = (int64_t)N * (backward ? (int64_t)H * W : (int64_t)OH * OW) * (C / 8);
  hipLaunchKernelGGL(subsample_bf16_kernel, dim3(fmi_bw_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)y, H, W, C / 8,
                     OH, OW, stride, total, backward);
  return fmi_launch_status();
}

// y = a + b (bf16), the residual add of a plain IR block
__global__ void __launch_bounds__(256) add_bf16_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, uint4* __restrict__ y, int64_t total8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += (int64_t)gridDim.x * 256) {
    float f[8], r[8];
    bf_unpack8(a[i], f);
    bf_unpack8(b[i], r);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += r[e];
    y[i] = bf_pack8(f);
  }
}
// a length that is no multiple of 8: one element per thread (not a hot path: the IR-SE body's tensors are multiples of 64 channels)
__global__ void __launch_bounds__(256) add_bf16_scalar_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                              int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = (bf16_t)bf_pack2(bf_lo(a[i]) + bf_lo(b[i]), 0.f);
}
extern "C" int fmi_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, int64_t n, void* stream) {
  if (!a || !b || !y || n <= 0) return FMI_ERR_BAD_ARG;
  if (n % 8 != 0) {
    hipLaunchKernelGGL(add_bf16_scalar_kernel, dim3(fmi_bw_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, n);
    return fmi_launch_status();
  }
  if (!fmi_al16(a) || !fmi_al16(b) || !fmi_al16(y)) return FMI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(add_bf16_kernel, dim3(fmi_bw_grid(n / 8, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const uint4*)a, (const uint4*)b, (uint4*)y, n / 8);
  return fmi_launch_status();
}

// ---- AdaptiveAvgPool2d(1) of the SE module: pooled[n][c] = mean_p x[n][p][c] (fp32 out), partial rows + one adding launch ----
__global__ void __launch_bounds__(256) gap_bf16_kernel(const uint4* __restrict__ x, float* __restrict__ parts, int64_t P, int C8, int64_t rows_per_block) {
  __shared__ float part[256 * 8];
  const int cg = threadIdx.x % C8, rl = threadIdx.x / C8, RL = 256 / C8;
  const int n = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > P) r1 = P;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (rl < RL)
    for (int64_t r = r0 + rl; r < r1; r += RL) {
      float f[8];
      bf_unpack8(x[((int64_t)n * P + r) * C8 + cg], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += f[e];
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[threadIdx.x * 8 + e] = s[e];
  __syncthreads();
  if ((int)threadIdx.x < C8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
      for (int l = 0; l < RL; ++l) t += part[(l * C8 + threadIdx.x) * 8 + e];
      parts[(((int64_t)n * gridDim.x + blockIdx.x) * C8 + threadIdx.x) * 8 + e] = t;
    }
  }
}
__global__ void __launch_bounds__(256) gap_finish_kernel(const float* __restrict__ parts, float* __restrict__ out, int nparts, int C, float inv) {
  const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (c >= C) return;
  float t = 0.f;
  for (int q = 0; q < nparts; ++q) t += parts[((int64_t)n * nparts + q) * C + c];
  out[(int64_t)n * C + c] = t * inv;
}
extern "C" int fmi_global_avgpool_bf16(const uint16_t* x, float* pooled, float* ws, int64_t ws_floats, int N, int64_t P, int C, void* stream) {
  if (!x || !pooled || !ws || N <= 0 || P <= 0 || C <= 0 || N > 65535) return FMI_ERR_BAD_ARG;
  const int C8 = C / 8;
  if (C % 8 != 0 || C8 > 256 || (C8 & (C8 - 1)) != 0 || !fmi_al16(x) || ws_floats < (int64_t)N * C) return FMI_ERR_UNSUPPORTED;
  int64_t blocks = ceil_div64(P, 64);
  const int64_t cap = ws_floats / ((int64_t)N * C) < 64 ? ws_floats / ((int64_t)N * C) : 64;
  if (blocks > cap) blocks = cap;
  const int64_t rpb = ceil_div64(P, blocks);
  blocks = ceil_div64(P, rpb);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gap_bf16_kernel, dim3((unsigned)blocks, N), dim3(256), 0, st, (const uint4*)x, ws, P, C8, rpb);
  hipLaunchKernelGGL(gap_finish_kernel, dim3((C + 255) / 256, N), dim3(256), 0, st, (const float*)ws, pooled, (int)blocks, C, 1.f / (float)P);
  return fmi_launch_status();
}
