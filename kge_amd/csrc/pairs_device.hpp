// pairs_device.hpp -- the 64 x 64 tile of the exact f32 pair kernels (score_pairs.hip: pairs_kernel; ce_dist.hip: the
// fused 1vsAll loss of TransE / RotatE): tile geometry, the guarded row load and the distance scorers' 4 x 4 micro-tile.
// One definition for both files, so that a score folded into a loss has the bits of the score kge_score_sp stores.
#pragma once
#include "common.hpp"

namespace kge {

constexpr int PT_BM = 64, PT_BN = 64, PT_KC = 16, PT_LD = 68;

template <typename T, bool VEC>
__device__ __forceinline__ f32x4 load4(const T* row, int c, int limit) {
  if (VEC) return ld4<T>(row + c);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (c + i < limit) ? ld1<T>(row + c + i) : 0.0f;
  return r;
}

// One coordinate pair (first-half elements q0 / t0v, second-half elements q1 / t1v) of a 4 x 4 micro-tile of TransE /
// RotatE distances, added to the running norms in the canonical order (oracle/kge_oracle.c: pair_score).
template <int SCORER, int NORM>
__device__ __forceinline__ void dist_micro_tile(const f32x4& q0, const f32x4& q1, const f32x4& t0v, const f32x4& t1v,
                                                float (&acc)[4][4], float lp) {
  if constexpr (SCORER != KGE_TRANSE) {
    // RotatE: |q - t| of 16 complex coordinates.  The correctly rounded square root in its short form
    // (common.hpp: sqrt_rn_core, checked exhaustively) wherever all 16 squares lie in its range -- ONE check
    // of their minimum and maximum per micro-tile instead of a branch per root; zeros, denormal-sized or huge
    // squares, inf and NaN (the maximum of a set with a NaN may hide it: NaN in, NaN out either way) send the
    // micro-tile through the IEEE sequence.
    float x[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dre = q0[i] - t0v[j], dim_ = q1[i] - t1v[j];
        x[i][j] = __builtin_fmaf(dim_, dim_, dre * dre);
      }
    float mn = x[0][0], mx = x[0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mn = __builtin_fminf(mn, x[i][j]);
        mx = __builtin_fmaxf(mx, x[i][j]);
      }
    if (__builtin_expect(mn >= SQRT_FAST_LO && mx <= SQRT_FAST_HI, 1)) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = norm_acc<NORM>(acc[i][j], sqrt_rn_core(x[i][j]), lp);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = norm_acc<NORM>(acc[i][j], __builtin_sqrtf(x[i][j]), lp);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = norm_acc<NORM>(acc[i][j], __builtin_fabsf(q0[i] - t0v[j]), lp);
        acc[i][j] = norm_acc<NORM>(acc[i][j], __builtin_fabsf(q1[i] - t1v[j]), lp);
      }
  }
}

// the finished norm of a distance scorer -> its score
template <int NORM>
__device__ __forceinline__ float dist_score(float v, float lp) {
  if (NORM == NORM_L1) return -v;
  if (NORM == NORM_L2) return -__builtin_sqrtf(v);
  return -powf(v, 1.0f / lp);
}

}  // namespace kge
