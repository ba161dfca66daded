// Inference form of the IR-SE bottleneck blocks of the pSp encoder (modules/psp/encoders/helpers.py:56-119 in eval mode) on bf16 NHWC
// activations: what lies between the convolutions of a block, fused.  The convolutions carry PReLU and the folded BatchNorms in their
// output stage (conv_bf16.hip, EpChanB) and leave the SE squeeze as partial column sums; here are
//   * the SE gate in one launch (finish of the partial sums, fc1, ReLU, fc2, sigmoid),
//   * the block tail (gate, residual add, the NEXT block's first BatchNorm, the fp32 pyramid tap) in one pass,
//   * the hand-over from the fp32 stem.
// Parameters and arithmetic are fp32, every bf16 value is rounded once, nothing is accumulated through atomics.  One thread of the
// element-wise kernels moves 8 channels (16-byte loads and stores).
#include "bf16x8.h"

// ---- SE gate: one workgroup of 512 threads per sample --------------------------------------------------------------------------
// part (rows_per_part > 0): [block of rows_per_part anchor rows][2][C] -- slot 0 = the block's rows of the sample its first row lies in,
// slot 1 = its rows of the next sample (P >= rows_per_part: a block touches at most two samples).  Sample n owns blocks
// n P / rpp .. ((n + 1) P - 1) / rpp; the G = 512 / C thread groups walk them interleaved and are added in group order: a fixed order.
__global__ void __launch_bounds__(512) se_gate_kernel(const float* __restrict__ part, int rpp, int64_t P, float inv, const float* __restrict__ fc1,
                                                      const float* __restrict__ fc2, float* __restrict__ gates, int C, int hid) {
  __shared__ float grp_sum[512];
  __shared__ float pooled[512];
  __shared__ float hidden[32];
  const int tid = threadIdx.x, n = blockIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = 512 / C, g = tid / C, c = tid - g * C;
  float t = 0.f;
  if (g < G) {
    if (rpp == 0) {
      if (g == 0) t = part[(int64_t)n * C + c];
    } else {
      const int64_t b0 = (int64_t)n * P / rpp, b1 = ((int64_t)(n + 1) * P - 1) / rpp;
      for (int64_t b = b0 + g; b <= b1; b += G) {
        const int64_t first = b * rpp / P;  // the sample of the block's first row: n or n - 1
        t += part[(b * 2 + (n - first)) * C + c];
      }
    }
  }
  grp_sum[tid] = t;
  __syncthreads();
  if (tid < C) {
    float s = 0.f;
    for (int q = 0; q < G; ++q) s += grp_sum[q * C + tid];
    pooled[tid] = s * inv;
  }
  __syncthreads();
  // fc1 + ReLU: wave w takes hidden units w, w + 8, ...; a lane walks channels lane, lane + 64, ...
  for (int j0 = 0; j0 < hid; j0 += 8) {
    const int j = j0 + w;
    float s = 0.f;
    if (j < hid)
      for (int k = lane; k < C; k += 64) s += fc1[(int64_t)j * C + k] * pooled[k];
    s = wave_sum(s);
    if (j < hid && lane == 0) hidden[j] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  if (tid < C) {
    float s = 0.f;
    for (int j = 0; j < hid; ++j) s += fc2[(int64_t)tid * hid + j] * hidden[j];
    gates[(int64_t)n * C + tid] = 1.f / (1.f + expf(-s));
  }
}
extern "C" int fmi_se_gate_f32(const float* part, int rows_per_part, int64_t P, float inv_count, const float* fc1, const float* fc2, float* gates,
                               int N, int C, void* stream) {
  if (!part || !fc1 || !fc2 || !gates || N <= 0 || C <= 0 || P <= 0 || rows_per_part < 0) return FMI_ERR_BAD_ARG;
  if (C % 16 != 0 || C > 512 || (rows_per_part > 0 && P < rows_per_part)) return FMI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)N), dim3(512), 0, (hipStream_t)stream, part, rows_per_part, P, inv_count, fc1, fc2, gates, C,
                     C / 16);
  return fmi_launch_status();
}

// ---- block tail ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) irse_tail_kernel(const uint4* __restrict__ r, const float* __restrict__ gate, const uint4* __restrict__ sc,
                                                        const float* __restrict__ nscale, const float* __restrict__ nshift, uint4* __restrict__ y,
                                                        uint4* __restrict__ z, float* __restrict__ tap, int OH, int OW, int C8, int SH, int SW, int ss,
                                                        int64_t total) {
  const int64_t PO = (int64_t)OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    const int64_t pix = i / C8, n = pix / PO;
    int64_t si = i;
    if (ss != 1) {
      const int64_t rem = pix - n * PO;
      const int oy = (int)(rem / OW), ox = (int)(rem - (int64_t)oy * OW);
      si = ((n * SH + (int64_t)oy * ss) * SW + (int64_t)ox * ss) * C8 + c8;
    }
    float f[8], s[8];
    bf_unpack8(r[i], f);
    bf_unpack8(sc[si], s);
    if (gate) {
      float g[8];
      bf_load8f(gate + (n * C8 + c8) * 8, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = f[e] * g[e] + s[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += s[e];
    }
    y[i] = bf_pack8(f);
    if (tap) {
      float4* t = reinterpret_cast<float4*>(tap + i * 8);
      t[0] = make_float4(f[0], f[1], f[2], f[3]);
      t[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
    if (z) {
      float a[8], b[8];
      bf_load8f(nscale + c8 * 8, a);
      bf_load8f(nshift + c8 * 8, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = f[e] * a[e] + b[e];
      z[i] = bf_pack8(f);
    }
  }
}
extern "C" int fmi_irse_tail_bf16(const uint16_t* r, const float* gate, const uint16_t* sc, const float* next_scale, const float* next_shift,
                                  uint16_t* y, uint16_t* z, float* tap, int N, int OH, int OW, int C, int SH, int SW, int sc_stride, void* stream) {
  if (!r || !sc || !y || N <= 0 || OH <= 0 || OW <= 0 || C <= 0 || SH <= 0 || SW <= 0 || (z && (!next_scale || !next_shift))) return FMI_ERR_BAD_ARG;
  if (sc_stride != 1 && sc_stride != 2) return FMI_ERR_UNSUPPORTED;
  if (OH != (SH - 1) / sc_stride + 1 || OW != (SW - 1) / sc_stride + 1) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(r) || !fmi_al16(gate) || !fmi_al16(sc) || !fmi_al16(next_scale) || !fmi_al16(next_shift) || !fmi_al16(y) || !fmi_al16(z) ||
      !fmi_al16(tap))
    return FMI_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)N * OH * OW * (C / 8);
  hipLaunchKernelGGL(irse_tail_kernel, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, (const uint4*)r, gate, (const uint4*)sc,
                     next_scale, next_shift, (uint4*)y, (uint4*)z, tap, OH, OW, C / 8, SH, SW, sc_stride, total);
  return fmi_launch_status();
}

// ---- stem hand-over ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) irse_stem_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                        uint4* __restrict__ y, uint4* __restrict__ z, int C8, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    float f[8], a[8], b[8];
    bf_load8f(x + i * 8, f);
    bf_load8f(scale + c8 * 8, a);
    bf_load8f(shift + c8 * 8, b);
    y[i] = bf_pack8(f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * a[e] + b[e];
    z[i] = bf_pack8(f);
  }
}
extern "C" int fmi_irse_stem_bf16(const float* x, const float* scale, const float* shift, uint16_t* y, uint16_t* z, int64_t rows, int C, void* stream) {
  if (!x || !scale || !shift || !y || !z || rows <= 0 || C <= 0) return FMI_ERR_BAD_ARG;
  if (C % 8 != 0 || !fmi_al16(x) || !fmi_al16(scale) || !fmi_al16(shift) || !fmi_al16(y) || !fmi_al16(z)) return FMI_ERR_UNSUPPORTED;
  const int64_t total = rows * (C / 8);
  hipLaunchKernelGGL(irse_stem_kernel, dim3(fmi_bw_grid(total, 256 * 2)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, (uint4*)y, (uint4*)z,
                     C / 8, total);
  return fmi_launch_status();
}
