// The mask-detector trainer's loss and validation metric on NHWC logits [P][C] (train_mask_detector.py:24-58,127-134 with
// modules/loss.py:148-186): CrossEntropyLoss + dice_loss(softmax, one_hot) forward and backward, the argmax Dice score of `evaluate`,
// and per-plane (sum a b, sum a, sum b) for the general dice_* helpers.  Bandwidth kernels: 16-byte loads, four pixels per thread and
// iteration, fp64 accumulation, reduced to one partial row per workgroup and finished by a second launch in a fixed order (the scheme
// and its helpers: head.h): no atomics, nothing to zero, bit-reproducible in either mode.
// The target is the dataset's int64 map (kind 0) or an fp32 map (kind 1); `> 0` (train_mask_detector.py:127) is applied here, so the
// class of a pixel is 0 or 1 whatever C is, as one_hot((mask > 0).long(), C) has it.
#include <math.h>
#include "common.h"
#include "head.h"

namespace {

__device__ __forceinline__ int cls_at(const void* t, int kind, int64_t p) {
  return kind == 0 ? (reinterpret_cast<const int64_t*>(t)[p] > 0 ? 1 : 0) : (reinterpret_cast<const float*>(t)[p] > 0.f ? 1 : 0);
}
// classes of pixels 4 g .. 4 g + 3: two 16-byte loads of int64, or one of fp32
__device__ __forceinline__ void cls_group(const void* t, int kind, int64_t g, int* cls) {
  if (kind == 0) {
    const longlong2* q = reinterpret_cast<const longlong2*>(t) + 2 * g;
    const longlong2 a = q[0], b = q[1];
    cls[0] = a.x > 0, cls[1] = a.y > 0, cls[2] = b.x > 0, cls[3] = b.y > 0;
  } else {
    const float4 a = reinterpret_cast<const float4*>(t)[g];
    cls[0] = a.x > 0.f, cls[1] = a.y > 0.f, cls[2] = a.z > 0.f, cls[3] = a.w > 0.f;
  }
}
// logits of pixels 4 g .. 4 g + 3: C 16-byte loads; v[j * C + c]
template <int C>
__device__ __forceinline__ void logit_group(const float* x, int64_t g, float* v) {
  const float4* q = reinterpret_cast<const float4*>(x) + g * C;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const float4 t = q[j];
    v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
  }
}
// stable softmax of one pixel with the accurate expf / logf: p[c] and the log-sum-exp
template <int C>
__device__ __forceinline__ float softmax_px(const float* x, float* p) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = expf(x[c] - m);
    s += p[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = p[c] / s;
  return m + logf(s);
}
template <int C>
__device__ __forceinline__ int argmax_px(const float* x) {
  int bi = 0;
#pragma unroll
  for (int c = 1; c < C; ++c)
    if (x[c] > x[bi] || (x[c] != x[c] && x[bi] == x[bi])) bi = c;  // the first maximum wins, NaN counts as the maximum (torch.argmax)
  return bi;
}

// dice_coeff (modules/loss.py:156-162) from the three sums; the `sets_sum == 0 -> 2 * inter` branch without a host read
__device__ __forceinline__ double dice_of(double inter, double sets_sum, double eps) {
  if (sets_sum == 0.0) sets_sum = 2.0 * inter;
  return (2.0 * inter + eps) / (sets_sum + eps);
}

// ---- loss forward: per workgroup one row (sum -log p_t, then per class: sum p_c t_c, sum p_c, sum t_c)
template <int C>
__device__ __forceinline__ void loss_px(const float* x, int cls, double& nll, double* I, double* S, unsigned* T) {
  float p[C];
  const float lse = softmax_px<C>(x, p);
  float xt = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) xt = cls == c ? x[c] : xt;
  nll += (double)(lse - xt);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    S[c] += (double)p[c];
    if (cls == c) {
      I[c] += (double)p[c];
      T[c] += 1u;
    }
  }
}
template <int C>
__global__ void __launch_bounds__(256) seg_loss_fwd_kernel(const float* __restrict__ x, const void* __restrict__ t, int kind, int64_t P,
                                                           double* __restrict__ part) {
  double nll = 0.0, I[C], S[C];
  unsigned T[C];  // a thread sees fewer than 2^32 pixels
#pragma unroll
  for (int c = 0; c < C; ++c) I[c] = 0.0, S[c] = 0.0, T[c] = 0u;
  const int64_t G = P >> 2;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
    float v[4 * C];
    int cls[4];
    logit_group<C>(x, g, v);
    cls_group(t, kind, g, cls);
#pragma unroll
    for (int j = 0; j < 4; ++j) loss_px<C>(v + j * C, cls[j], nll, I, S, T);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(P & 3)) {  // the last P % 4 pixels
    const int64_t p = (G << 2) + threadIdx.x;
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[p * C + c];
    loss_px<C>(v, cls_at(t, kind, p), nll, I, S, T);
  }
  double acc[1 + 3 * C];
  acc[0] = nll;
#pragma unroll
  for (int c = 0; c < C; ++c) acc[1 + c] = I[c], acc[1 + C + c] = S[c], acc[1 + 2 * C + c] = (double)T[c];
  block_rows_out<1 + 3 * C>(acc, part, blockIdx.x);
}
// one workgroup: sums[0] = sum -log p_t, sums[1 + c] = I_c, sums[1 + C + c] = sum p_c, sums[1 + 2 C + c] = sum t_c;
// out3 = (ce, dice, ce + dice)
__global__ void __launch_bounds__(256) seg_loss_finish_kernel(const double* __restrict__ part, int64_t rows, int C, int64_t P, double eps,
                                                              float* __restrict__ out3, double* __restrict__ sums) {
  __shared__ double red[4];
  __shared__ double tot[1 + 3 * 8];
  const int nv = 1 + 3 * C;
  for (int k = 0; k < nv; ++k) {
    const double s = column_sum(part, rows, nv, k, red);
    if (threadIdx.x == 0) tot[k] = s;
  }
  __syncthreads();
  if (threadIdx.x < nv) sums[threadIdx.x] = tot[threadIdx.x];
  if (threadIdx.x == 0) {
    const double ce = tot[0] / (double)P;
    double d = 0.0;
    for (int c = 0; c < C; ++c) d += dice_of(tot[1 + c], tot[1 + C + c] + tot[1 + 2 * C + c], eps);
    const double dice = 1.0 - d / (double)C;
    out3[0] = (float)ce, out3[1] = (float)dice, out3[2] = (float)(ce + dice);
  }
}

// ---- loss backward: dlogits[p][k] = g p_k (h_k - sum_j p_j h_j) + g (p_k - t_k) / P with
// h_c = -(1 / C) (2 t_c (U_c + eps) - (2 I_c + eps)) / (U_c + eps)^2 = ha_c t_c + hb_c, U_c = sum p_c + sum t_c
template <int C>
__device__ __forceinline__ void bwd_px(const float* x, int cls, const float* ha, const float* hb, float g, float g_over_p, float* d) {
  float p[C], h[C];
  softmax_px<C>(x, p);
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    h[c] = cls == c ? ha[c] + hb[c] : hb[c];
    dot += p[c] * h[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) d[c] = g * (p[c] * (h[c] - dot)) + g_over_p * (p[c] - (cls == c ? 1.f : 0.f));
}
template <int C>
__global__ void __launch_bounds__(256) seg_loss_bwd_kernel(const float* __restrict__ x, const void* __restrict__ t, int kind, int64_t P, double eps,
                                                           const double* __restrict__ sums, const float* __restrict__ gout, float* __restrict__ dx) {
  float ha[C], hb[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double inter = sums[1 + c], u = sums[1 + C + c] + sums[1 + 2 * C + c];
    // U_c == 0 is dice_coeff's other branch, (2 I + eps) / (2 I + eps): constant, no gradient
    ha[c] = u == 0.0 ? 0.f : (float)(-2.0 / ((double)C * (u + eps)));
    hb[c] = u == 0.0 ? 0.f : (float)((2.0 * inter + eps) / ((double)C * (u + eps) * (u + eps)));
  }
  const float g = gout[0], gp = (float)((double)g / (double)P);
  const int64_t G = P >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < G; i += (int64_t)gridDim.x * 256) {
    float v[4 * C], d[4 * C];
    int cls[4];
    logit_group<C>(x, i, v);
    cls_group(t, kind, i, cls);
#pragma unroll
    for (int j = 0; j < 4; ++j) bwd_px<C>(v + j * C, cls[j], ha, hb, g, gp, d + j * C);
    float4* q = reinterpret_cast<float4*>(dx) + i * C;
#pragma unroll
    for (int j = 0; j < C; ++j) q[j] = make_float4(d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(P & 3)) {
    const int64_t p = (G << 2) + threadIdx.x;
    float v[C], d[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = x[p * C + c];
    bwd_px<C>(v, cls_at(t, kind, p), ha, hb, g, gp, d);
#pragma unroll
    for (int c = 0; c < C; ++c) dx[p * C + c] = d[c];
  }
}

// ---- Dice score of `evaluate` (train_mask_detector.py:47-49): per (sample, class 1 .. C-1) the counts I, sum pred, sum true of the
// one-hot argmax against the one-hot target.  grid (gx, N); VEC needs H * W % 4 == 0 (every sample then starts on a 16-byte boundary).
template <int C, bool VEC>
__global__ void __launch_bounds__(256) seg_score_kernel(const float* __restrict__ x, const void* __restrict__ t, int kind, int64_t HW,
                                                        double* __restrict__ part) {
  constexpr int NV = 3 * (C - 1);
  unsigned cnt[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) cnt[k] = 0u;
  const int64_t n = blockIdx.y, base = n * HW;
  auto count = [&](int pred, int cls) {
#pragma unroll
    for (int c = 1; c < C; ++c) {
      cnt[3 * (c - 1)] += (pred == c && cls == c) ? 1u : 0u;
      cnt[3 * (c - 1) + 1] += pred == c ? 1u : 0u;
      cnt[3 * (c - 1) + 2] += cls == c ? 1u : 0u;
    }
  };
  if (VEC) {
    const int64_t G = HW >> 2, g0 = base >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
      float v[4 * C];
      int cls[4];
      logit_group<C>(x, g0 + g, v);
      cls_group(t, kind, g0 + g, cls);
#pragma unroll
      for (int j = 0; j < 4; ++j) count(argmax_px<C>(v + j * C), cls[j]);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
      float v[C];
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = x[(base + i) * C + c];
      count(argmax_px<C>(v), cls_at(t, kind, base + i));
    }
  }
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = (double)cnt[k];
  block_rows_out<NV>(acc, part, n * gridDim.x + blockIdx.x);
}
// one workgroup: thread i takes samples i, i + 256, ...; per sample the mean over classes of dice_coeff; then the mean over samples
__global__ void __launch_bounds__(256) seg_score_finish_kernel(const double* __restrict__ part, int gx, int N, int C, double eps,
                                                               float* __restrict__ out) {
  __shared__ double red[4];
  const int nv = 3 * (C - 1);
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    double d = 0.0;
    for (int c = 0; c < C - 1; ++c) {
      double a[3] = {0.0, 0.0, 0.0};
      for (int r = 0; r < gx; ++r)
        for (int k = 0; k < 3; ++k) a[k] += part[((int64_t)n * gx + r) * nv + 3 * c + k];
      d += dice_of(a[0], a[1] + a[2], eps);
    }
    s += d / (double)(C - 1);
  }
  s = block_sum_256_d(s, red);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)N);
}

// ---- (sum a b, sum a, sum b) per plane of two fp32 tensors [planes][n]; grid (gx, planes)
template <bool VEC>
__global__ void __launch_bounds__(256) plane_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                         double* __restrict__ part) {
  const float* pa = a + (int64_t)blockIdx.y * n;
  const float* pb = b + (int64_t)blockIdx.y * n;
  double acc[3] = {0.0, 0.0, 0.0};
  if (VEC) {
    const int64_t G = n >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G; g += (int64_t)gridDim.x * 256) {
      const float4 u = reinterpret_cast<const float4*>(pa)[g], w = reinterpret_cast<const float4*>(pb)[g];
      acc[0] += (double)u.x * (double)w.x + (double)u.y * (double)w.y + (double)u.z * (double)w.z + (double)u.w * (double)w.w;
      acc[1] += ((double)u.x + (double)u.y) + ((double)u.z + (double)u.w);
      acc[2] += ((double)w.x + (double)w.y) + ((double)w.z + (double)w.w);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      const double u = (double)pa[i], w = (double)pb[i];
      acc[0] += u * w, acc[1] += u, acc[2] += w;
    }
  }
  block_rows_out<3>(acc, part, (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

}  // namespace

#define SEG_DISPATCH_C(CALL) \
  switch (C) {               \
    case 2: CALL(2); break;  \
    case 3: CALL(3); break;  \
    case 4: CALL(4); break;  \
    case 5: CALL(5); break;  \
    case 6: CALL(6); break;  \
    case 7: CALL(7); break;  \
    default: CALL(8); break; \
  }

extern "C" int fmi_seg_ce_dice_fwd_f32(const float* logits, const void* target, int target_kind, int64_t P, int C, double eps, float* out3,
                                       double* sums, double* ws_part, int64_t ws_doubles, void* stream) {
  if (!logits || !target || !out3 || !sums || !ws_part || P <= 0 || C < 2 || C > 8 || (target_kind != 0 && target_kind != 1)) return FMI_ERR_BAD_ARG;
  if (!fmi_al16(logits) || !fmi_al16(target)) return FMI_ERR_BAD_ARG;
  const int rows = rows_for(P >> 2, ROWS_SEG_LOSS);
  if (ws_doubles < (int64_t)rows * (1 + 3 * C)) return FMI_ERR_BAD_ARG;
#define CALL(CC) hipLaunchKernelGGL(seg_loss_fwd_kernel<CC>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, target, target_kind, P, ws_part)
  SEG_DISPATCH_C(CALL)
#undef CALL
  hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws_part, (int64_t)rows, C, P, eps, out3, sums);
  return fmi_launch_status();
}

extern "C" int fmi_seg_ce_dice_bwd_f32(const float* logits, const void* target, int target_kind, int64_t P, int C, double eps, const double* sums,
                                       const float* gout, float* dlogits, void* stream) {
  if (!logits || !target || !sums || !gout || !dlogits || P <= 0 || C < 2 || C > 8 || (target_kind != 0 && target_kind != 1)) return FMI_ERR_BAD_ARG;
  if (!fmi_al16(logits) || !fmi_al16(target) || !fmi_al16(dlogits)) return FMI_ERR_BAD_ARG;
  const int grid = fmi_bw_grid(P >> 2, 256);
#define CALL(CC) \
  hipLaunchKernelGGL(seg_loss_bwd_kernel<CC>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, target, target_kind, P, eps, sums, gout, dlogits)
  SEG_DISPATCH_C(CALL)
#undef CALL
  return fmi_launch_status();
}

extern "C" int fmi_seg_dice_score_f32(const float* logits, const void* target, int target_kind, int N, int64_t HW, int C, double eps, float* out,
                                      double* ws_part, int64_t ws_doubles, void* stream) {
  if (!logits || !target || !out || !ws_part || N <= 0 || N > 65535 || HW <= 0 || C < 2 || C > 8 || (target_kind != 0 && target_kind != 1))
    return FMI_ERR_BAD_ARG;
  if (!fmi_al16(logits) || !fmi_al16(target)) return FMI_ERR_BAD_ARG;
  const bool vec = (HW & 3) == 0;
  const int gx = rows_for(vec ? HW >> 2 : HW, ROWS_PER_PLANE);
  if (ws_doubles < (int64_t)N * gx * 3 * (C - 1)) return FMI_ERR_BAD_ARG;
  const dim3 grid(gx, N), block(256);
#define CALL(CC)                                                                                                                        \
  if (vec)                                                                                                                              \
    hipLaunchKernelGGL((seg_score_kernel<CC, true>), grid, block, 0, (hipStream_t)stream, logits, target, target_kind, HW, ws_part);   \
  else                                                                                                                                  \
    hipLaunchKernelGGL((seg_score_kernel<CC, false>), grid, block, 0, (hipStream_t)stream, logits, target, target_kind, HW, ws_part)
  SEG_DISPATCH_C(CALL)
#undef CALL
  hipLaunchKernelGGL(seg_score_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws_part, gx, N, C, eps, out);
  return fmi_launch_status();
}

extern "C" int fmi_plane_sums_f32(const float* a, const float* b, int planes, int64_t n, double* out3, double* ws_part, int64_t ws_doubles,
                                  void* stream) {
  if (!a || !b || !out3 || !ws_part || planes <= 0 || planes > 65535 || n <= 0) return FMI_ERR_BAD_ARG;
  const bool vec = (n & 3) == 0 && fmi_al16(a) && fmi_al16(b);
  const int gx = rows_for(vec ? n >> 2 : n, planes == 1 ? ROWS_ONE_PLANE : ROWS_PER_PLANE);
  if (ws_doubles < (int64_t)planes * gx * 3) return FMI_ERR_BAD_ARG;
  if (vec)
    hipLaunchKernelGGL(plane_sums_kernel<true>, dim3(gx, planes), dim3(256), 0, (hipStream_t)stream, a, b, n, ws_part);
  else
    hipLaunchKernelGGL(plane_sums_kernel<false>, dim3(gx, planes), dim3(256), 0, (hipStream_t)stream, a, b, n, ws_part);
  hipLaunchKernelGGL(plane_rows_finish_kernel<double>, dim3((planes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws_part, gx, planes, 3, 1.0, out3);
  return fmi_launch_status();
}
