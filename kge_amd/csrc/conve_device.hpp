// conve_device.hpp -- the canonical arithmetic of ConvE's evaluation network (kge/model/conve.py:75-93), defined ONCE:
// both kernels of conve.hip compute through these functions, so a query row is a pure function of its two table rows
// and the network.  Compiled with -ffp-contract=off: one rounding per written operation, fused
// multiply-adds only where __builtin_fmaf stands.
//
// With e = ent[s][1:], r = rel[p][1:] read as two h x w images stacked to 2h x w (the subject on top), channel c < 32:
//   convolution   v = b_c (or +0 without a bias);  for ky = 0 .. fs-1, for kx = 0 .. fs-1 (ascending):
//                 v = fma(img[y + ky - pad][x + kx - pad], w_c[ky][kx], v).  A tap that falls into the zero padding
//                 enters no fma (cv_conv).
//   batch norm    (v - mean) * rsq,  rsq = 1 / sqrt(var + eps): one add, one correctly rounded square root, one
//                 correctly rounded division -- the same function for both norms (cv_rsq, cv_bn).
//   ReLU          v > 0 ? v : +0 (a NaN stays a NaN, -0 becomes +0) (cv_relu).
//   projection    feature k' = c * Ho * Wo + y * Wo + x.  Output j is the sum of 32 channel partials.  Partial c runs
//                 over the channel's positions k = y * Wo + x in groups of eight: group g holds k = 8 g .. 8 g + 7 and is
//                 taken in four steps t = 0 .. 3; step t adds position 8 g + t and then position 8 g + 4 + t, each as
//                 P = fma(feature, proj_w[j][c * Ho * Wo + k], P), from +0, groups ascending -- the chain
//                 v_mfma_f32_32x32x2_f32 executes.  Positions k >= Ho * Wo of the last group are zeros on both sides.
//                 Then x_j = ((((P_0 + P_1) + P_2) + ...) + P_31) + proj_b[j], plain additions in ascending c
//                 (cv_finish).
//   output        q[0] = 1.0f, q[1 + j] = relu(bn2(x_j)).
#pragma once
#include "common.hpp"

namespace kge {

constexpr int CV_CHANNELS = 32;       // conve.py:53-60: out_channels = 32; also the split of the feature axis
constexpr int CV_TM = 32;             // query rows per workgroup: the M of one 32x32x2 MFMA
constexpr int CV_THREADS = 256;
constexpr int CV_MAX_LDF = 1024;      // floats per row of the feature slice in LDS: 32 rows = 128 KiB
constexpr int CV_LDS_ASK = 48 * 1024; // more dynamic LDS than a launch gets without asking

// floats per LDS row of one channel's slice: Ho * Wo rounded up to whole groups of eight, + 1 (an odd pitch: the 32
// rows of an MFMA operand read fall into 32 different banks)
__host__ __device__ inline int cv_ldf(int hw) { return ((hw + 7) & ~7) + 1; }

__device__ __forceinline__ float cv_rsq(float var, float eps) { return __fdiv_rn(1.0f, __fsqrt_rn(var + eps)); }
__device__ __forceinline__ float cv_bn(float v, float mean, float rsq) { return (v - mean) * rsq; }
__device__ __forceinline__ float cv_relu(float v) { return v <= 0.0f ? 0.0f : v; }

// one output of the convolution.  es / rs: the subject's and the relation's image (h x w floats, row-major: the row
// behind its bias column); wc: the channel's FS x FS taps.
template <int FS>
__device__ __forceinline__ float cv_conv(const float* __restrict__ es, const float* __restrict__ rs, int h, int w,
                                         int pad, int y, int x, const float (&wc)[FS * FS], float bias) {
  float v = bias;
#pragma unroll
  for (int ky = 0; ky < FS; ++ky) {
    const int yy = y + ky - pad;
    if (yy < 0 || yy >= 2 * h) continue;
    const float* src = yy < h ? es + yy * w : rs + (yy - h) * w;
#pragma unroll
    for (int kx = 0; kx < FS; ++kx) {
      const int xx = x + kx - pad;
      if (xx >= 0 && xx < w) v = __builtin_fmaf(src[xx], wc[ky * FS + kx], v);
    }
  }
  return v;
}

// the 32 channel partials of one output, `stride` floats apart, to the value in front of batch-norm 2
__device__ __forceinline__ float cv_finish(const float* __restrict__ part, long long stride, float proj_b) {
  float x = part[0];
  for (int c = 1; c < CV_CHANNELS; ++c) x = x + part[c * stride];
  return x + proj_b;
}

}  // namespace kge
