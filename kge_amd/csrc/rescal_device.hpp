// rescal_device.hpp -- the canonical arithmetic of RESCAL (kge/model/rescal.py:14-52), defined ONCE: every RESCAL
// kernel of rescal.hip builds its query vector through these functions, so a query is a pure function of its entity row
// and its mixing matrix.  Compiled with -ffp-contract=off: one rounding per written operation,
// fused multiply-adds only where __builtin_fmaf stands.
//
// A relation row is M, row-major d x d (rescal.py:25).  score(s, p, o) = s^T M o in two stages:
//   sp_ (and spo, neg slot 2)   q_b = sum_a s_a M[a][b]      rs_matvec_t:  q = M^T s, the sum runs DOWN a column
//   _po (and neg slot 0)        q_a = sum_b M[a][b] o_b      rs_matvec:    q = M o,   the sum runs ALONG a row
// Both sums are REDUCE8 over the summation index k (a, resp. b):  the indices are cut into groups of four (k / 4); group
// c goes to partial sum c mod 8; a partial sum takes its terms in ascending k as p = fma(x_k, M_k, p), starting from
// +0; the eight partial sums are then added as the xor butterfly of an 8-lane group does it (offsets 4, 2, 1):
//   ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)).
// Indices k >= d do not exist: they enter no sum.  The second stage -- q against the other row -- is not defined here:
// it is the float32 chain of the ComplEx / DistMult kernels (rules 3 and 4) over (q, row).
//
// Both functions are called by all 256 threads of a workgroup; the vector x and the result live in LDS.  The backward
// uses the same two functions for its mat-vec (g_s = M g_q is rs_matvec, g_o = M^T g_q is rs_matvec_t).
#pragma once
#include "common.hpp"

namespace kge {

constexpr int RS_MAX_DIM = KGE_RESCAL_MAX_DIM;  // 256: one coordinate per thread of a workgroup, 8 KiB of partial sums
constexpr int RS_THREADS = 256;
constexpr int RS_LDV = RS_MAX_DIM + 4;  // a vector in LDS (the element path pads the last group of four)

__device__ __forceinline__ float rs_combine8(float p0, float p1, float p2, float p3, float p4, float p5, float p6,
                                             float p7) {
  return ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7));
}
// the same sum over the 8 lanes of a group (all eight active)
__device__ __forceinline__ float rs_butterfly8(float P) {
  P = P + __shfl_xor(P, 4, 64);
  P = P + __shfl_xor(P, 2, 64);
  P = P + __shfl_xor(P, 1, 64);
  return P;
}

// four coordinates k0 .. k0 + 3 of a row; the element path reads one float at a time and gives 0 behind the row's end
template <bool VEC>
__device__ __forceinline__ f32x4 rs_ld4(const float* row, int k0, int d) {
  if (VEC) return ld4<float>(row + k0);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (k0 + i < d) ? row[k0 + i] : 0.0f;
  return r;
}

// out_b = sum_a x_a M[a][b], b < d.  A thread owns one partial sum of four neighbouring columns: consecutive threads
// take consecutive groups of four columns, so a wave reads whole contiguous pieces of rows of M (16 bytes per lane on
// the vector path).  `part`: 8 * RS_LDV floats of LDS.  Ends with a barrier: `out` is complete for every thread.
template <bool VEC>
__device__ __forceinline__ void rs_matvec_t(const float* __restrict__ M, const float* x, int d, float* part, float* out) {
  const int nc4 = (d + 3) >> 2;
  for (int w = threadIdx.x; w < 8 * nc4; w += RS_THREADS) {
    const int k = w / nc4, c0 = (w - k * nc4) * 4;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int a0 = 4 * k; a0 < d; a0 += 32) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = a0 + i;
        if (a < d) {
          const f32x4 m4 = rs_ld4<VEC>(M + (long long)a * d, c0, d);
          const float xa = x[a];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xa, m4[j], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[k * RS_LDV + c0 + j] = acc[j];
  }
  __syncthreads();
  for (int b = threadIdx.x; b < d; b += RS_THREADS)
    out[b] = rs_combine8(part[b], part[RS_LDV + b], part[2 * RS_LDV + b], part[3 * RS_LDV + b], part[4 * RS_LDV + b],
                         part[5 * RS_LDV + b], part[6 * RS_LDV + b], part[7 * RS_LDV + b]);
  __syncthreads();
}

// out_a = sum_b M[a][b] x_b, a < d.  An 8-lane group per row of M, lane lg takes the groups of four lg, lg + 8, ...:
// the group reads 128 contiguous bytes of the row per step, the sum is reduced across the lanes.  Ends with a barrier.
template <bool VEC>
__device__ __forceinline__ void rs_matvec(const float* __restrict__ M, const float* x, int d, float* out) {
  const int lg = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int rows = (d + 31) & ~31;  // (whole waves stay in the loop: the shuffles see all lanes)
  for (int a = g; a < rows; a += RS_THREADS / 8) {
    float P = 0.0f;
    if (a < d) {
      const float* row = M + (long long)a * d;
      for (int k0 = lg * 4; k0 < d; k0 += 32) {
        const f32x4 m4 = rs_ld4<VEC>(row, k0, d);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (VEC || k0 + i < d) P = __builtin_fmaf(m4[i], x[k0 + i], P);
      }
    }
    P = rs_butterfly8(P);
    if (a < d && lg == 0) out[a] = P;
  }
  __syncthreads();
}

// ---- the second stage, row-wise (kge_score_spo / kge_score_neg): the summation of score_spo.hip's DistMult kernel over
// (q, x) -- spo_device.hpp apply_chunk with the fixed side q * 1.0f = q: a lane owns the chunk of eight coordinates
// [8 lg, 8 lg + 8) as one fma chain from +0, the G lanes of a group (G = group_size(d)) are added by the xor butterfly
// G / 2, ..., 1.  `q` in LDS, `x` a row in memory.  All lanes of a group call.
template <bool VEC>
__device__ __forceinline__ float rs_row_dot(const float* q, const float* __restrict__ x, int d, int lg, int G) {
  float P = 0.0f;
  const int c0 = lg * 8;
  if (c0 < d) {
    const f32x4 x0 = rs_ld4<VEC>(x, c0, d), x1 = rs_ld4<VEC>(x, c0 + 4, d);  // (vector path: d % 8 == 0)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (VEC || c0 + i < d) P = __builtin_fmaf(q[c0 + i], x0[i], P);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (VEC || c0 + 4 + i < d) P = __builtin_fmaf(q[c0 + 4 + i], x1[i], P);
  }
  for (int off = G >> 1; off >= 1; off >>= 1) P = P + __shfl_xor(P, off, 64);
  return P;
}

}  // namespace kge
