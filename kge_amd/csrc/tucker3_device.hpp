// tucker3_device.hpp -- the canonical arithmetic of the Tucker3 relation projection (kge/model/embedder/
// tucker3_relation_embedder.py: M_p = (B[p] @ W^T).view(d, d)), defined once.
//
//   out[i][j] = sum_{k < d_r} B[idx_i][k] * W[j][k]
//
// ONE fused multiply-add chain per element, in ascending k, from +0:
//
//   acc = +0;  for k = 0 .. d_r - 1:  acc = fma(B[idx_i][k], W[j][k], acc)
//
// exactly d_r operations -- a ragged last K chunk stops at d_r, it is not padded with zero terms (fma(0, 0, -0) would
// turn a -0 into +0).  The element is a pure function of its B row and its W row: the chain does not know the tile, the
// lane, n, the index form or how the operands were loaded (16-byte or element loads fetch the same floats).
#pragma once
#include "common.hpp"

namespace kge {

constexpr int T3_BM = 64, T3_BN = 128, T3_KC = 32;   // output tile of a workgroup, K chunk
constexpr int T3_LDA = T3_BM + 4, T3_LDW = T3_BN + 4;  // LDS pitches of the transposed chunks [k][row] (16-byte rows)
constexpr int T3_THREADS = 256, T3_TR = 8, T3_TC = 4;  // a thread's register tile: 8 rows x 4 columns

__device__ __forceinline__ float t3_step(float acc, float b, float w) { return __builtin_fmaf(b, w, acc); }

// 4 consecutive floats from p, of which `valid` exist (the rest: 0, never used by the chain)
__device__ __forceinline__ f32x4 t3_load4(const float* p, long long valid, bool vec) {
  if (valid >= 4 && vec) return ld4<float>(p);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < valid) r[e] = p[e];
  return r;
}

}  // namespace kge
