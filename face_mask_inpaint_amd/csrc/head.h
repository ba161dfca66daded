// What the one-pass loss heads share (segloss.hip, psploss.hip, ganhead.hip; loss.hip's ssim_valid takes the finishing launch and
// rows_for): the partial-row reduction and the RGB pixel I/O.  Include after common.h.
//
// The reduction scheme: every thread accumulates in fp64; a workgroup reduces wave shuffle -> LDS and writes ONE row of NV partial sums
// (block_rows_out); a finishing launch adds the rows in a fixed order (column_sum / rows_finish_kernel for one total over all rows,
// plane_rows_finish_kernel for one total per plane).  No atomics, nothing to zero, bit-reproducible in either mode.  The order of every
// addition here is part of the result: do not reassociate.
//
// Several files of one library include this header: everything is forceinline, static inline, a template or in the anonymous namespace.
// It holds no fp32 arithmetic, so a file's `#pragma clang fp contract` setting (ganhead.hip's, ahead of its includes) changes nothing here.
#pragma once
#ifndef FMI_HOST_EMU  // needs common.h's device branch (wave_sum_d, block_sum_256_d)

namespace {

// ---- row reductions ----
// Caps of the partial rows a sum kernel writes (= its workgroups).  functional.py sizes the workspaces by the same numbers
// (_ROWS_PER_PLANE, _ROWS_ONE_PLANE, _ROWS_SEG_LOSS there): change both sides together, or the entries return FMI_ERR_BAD_ARG.
constexpr int ROWS_PER_PLANE = 64;   // per sample or plane: seg_dice_score, plane_sums (planes > 1), psp / gan head forward, ssim_valid
constexpr int ROWS_ONE_PLANE = 256;  // plane_sums over a single plane
constexpr int ROWS_SEG_LOSS = 1024;  // seg_ce_dice forward, over the whole batch

// v[0 .. NV) of every thread -> part[row][0 .. NV): wave shuffle, LDS, the four waves added as (w0 + w1) + (w2 + w3).
// Contract: reached by all 256 threads of the workgroup in uniform control flow, and at most once per kernel and NV -- the LDS array
// has no leading barrier, so a second call could overwrite it while the first is still being read.
template <int NV>
__device__ __forceinline__ void block_rows_out(double* v, double* __restrict__ part, int64_t row) {
  __shared__ double red[4][NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum_d(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < NV) part[row * NV + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// sum of column k of part[rows][nv]: thread t adds rows t, t + 256, ... in order, then the block in a fixed order
__device__ __forceinline__ double column_sum(const double* __restrict__ part, int64_t rows, int nv, int k, double* lds4) {
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < rows; r += 256) s += part[r * nv + k];
  return block_sum_256_d(s, lds4);
}
// one workgroup: the nv column totals of part[rows][nv] to sums[k] and / or, divided by count, to means[k] (either may be NULL)
__global__ void __launch_bounds__(256) rows_finish_kernel(const double* __restrict__ part, int64_t rows, int nv, double count, double* __restrict__ sums,
                                                          float* __restrict__ means) {
  __shared__ double red[4];
  for (int k = 0; k < nv; ++k) {
    const double s = column_sum(part, rows, nv, k, red);
    if (threadIdx.x == 0) {
      if (sums) sums[k] = s;
      if (means) means[k] = (float)(s / count);
    }
  }
}
// part[planes][gx][nv]: one thread per (plane, k) adds rows 0 .. gx - 1 in order; out[plane * nv + k] = (T)(sum * scale)
template <class T>
__global__ void plane_rows_finish_kernel(const double* __restrict__ part, int gx, int planes, int nv, double scale, T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * nv) return;
  const int plane = i / nv, k = i - plane * nv;
  double s = 0.0;
  for (int r = 0; r < gx; ++r) s += part[((int64_t)plane * gx + r) * nv + k];
  out[i] = (T)(s * scale);
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
// workgroups (= partial rows) for work_items at 256 per workgroup, within [1, cap]
inline int rows_for(int64_t work_items, int cap) {
  int64_t g = ceil_div64(work_items, 256);
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---- RGB pixel I/O: PX = 4 neighbouring pixels (16-byte accesses; the caller has checked size and alignment) or PX = 1 ----
// PX pixels of one plane starting at element e
template <int PX>
__device__ __forceinline__ void load_px(const float* __restrict__ x, int64_t e, float* v) {
  if (PX == 4) {
    const float4 t = *reinterpret_cast<const float4*>(x + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = x[e];
  }
}
// 3 PX interleaved values to / from element e of an NHWC image
template <int PX>
__device__ __forceinline__ void store_hwc(float* __restrict__ x, int64_t e, const float* v) {
  if (PX == 4) {
    float4* q = reinterpret_cast<float4*>(x + e);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) x[e + k] = v[k];
  }
}
template <int PX>
__device__ __forceinline__ void load_hwc(const float* __restrict__ x, int64_t e, float* v) {
  if (PX == 4) {
    const float4* q = reinterpret_cast<const float4*>(x + e);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = q[k];
      v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x[e + k];
  }
}
// RGB of pixel p of sample n: from three planes, or from an interleaved [N][H][W][3] image (hwc)
__device__ __forceinline__ void load_rgb(const float* __restrict__ x, bool hwc, int64_t n, int64_t hw, int64_t p, float* v) {
  if (hwc) {
    const float* q = x + (n * hw + p) * 3;
    v[0] = q[0], v[1] = q[1], v[2] = q[2];
  } else {
    const float* q = x + n * 3 * hw + p;
    v[0] = q[0], v[1] = q[hw], v[2] = q[2 * hw];
  }
}
// PX pixels x RGB from pixel p of sample n into a[c][j]: four pixels are three 16-byte loads in either layout
template <int PX>
__device__ __forceinline__ void load_rgb_run(const float* __restrict__ x, bool hwc, int64_t n, int64_t hw, int64_t p, float (*a)[PX]) {
  if (PX == 1) {
    float t[3];
    load_rgb(x, hwc, n, hw, p, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c][0] = t[c];
  } else if (hwc) {
    float t[3 * PX];
    load_hwc<PX>(x, (n * hw + p) * 3, t);
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c][j] = t[j * 3 + c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) load_px<PX>(x, (n * 3 + c) * hw + p, a[c]);
  }
}
// d[c][j] to pixels p .. p + PX - 1 of sample n, in the image's own layout
template <int PX>
__device__ __forceinline__ void store_rgb_run(float* __restrict__ x, bool hwc, int64_t n, int64_t hw, int64_t p, float (*d)[PX]) {
  if (hwc) {
    float o[3 * PX];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[j * 3 + c] = d[c][j];
    store_hwc<PX>(x, (n * hw + p) * 3, o);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (PX == 4)
        *reinterpret_cast<float4*>(x + (n * 3 + c) * hw + p) = make_float4(d[c][0], d[c][1], d[c][2], d[c][3]);
      else
        x[(n * 3 + c) * hw + p] = d[c][0];
    }
  }
}

}  // namespace
#endif  // !FMI_HOST_EMU
