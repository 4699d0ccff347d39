// bwd_device.hpp -- the per-coordinate-pair gradient arithmetic shared by the backward kernels (bwd.hip,
// score_neg_shared.hip, ce_dist.hip).
#pragma once
#include "common.hpp"

namespace kge {

// element k of a float32 row, 0 beyond its valid length
__device__ __forceinline__ float ldf(const float* row, int k, int limit) {
  return k < limit ? row[k] : 0.0f;
}

// weight of one distance component e (TransE) given the pair's distance
template <int NORM>
__device__ __forceinline__ float transe_w(float e, float dist, float p) {
  if (NORM == NORM_L1) return (e > 0.f) ? 1.f : ((e < 0.f) ? -1.f : 0.f);
  if (NORM == NORM_L2) return dist > 0.f ? e / dist : 0.f;
  if (dist <= 0.f || e == 0.f) return 0.f;
  float ae = __builtin_fabsf(e);
  return (e > 0.f ? 1.f : -1.f) * powf(ae, p - 1.f) / powf(dist, p - 1.f);
}

// weights (wre, wim) of one complex distance component (RotatE)
template <int NORM>
__device__ __forceinline__ void rotate_w(float dre, float dim_, float dist, float p, float& wre,
                                         float& wim) {
  float ab = sqrt_rn_fast(__builtin_fmaf(dim_, dim_, dre * dre));  // (correctly rounded: common.hpp)
  float f;
  if (NORM == NORM_L1) f = ab > 0.f ? 1.f / ab : 0.f;
  else if (NORM == NORM_L2) f = dist > 0.f ? 1.f / dist : 0.f;
  else f = (dist > 0.f && ab > 0.f) ? powf(ab, p - 2.f) / powf(dist, p - 1.f) : 0.f;
  wre = dre * f;
  wim = dim_ * f;
}

// ---- score_spo backward ---------------------------------------------------------------------
// gradients of g * score(s, p, o) w.r.t. one coordinate pair (first-half element 0, second-half
// element 1) of the s, p and o rows
// (ROTPRE: RotatE with r0 = cos, r1 = sin of the phase, precomputed per relation -- rot_table_kernel)
template <int SCORER, int NORM, bool ROTPRE = false>
__device__ __forceinline__ void spo_pair_grads(float s0, float s1, float r0, float r1, float o0, float o1,
                                               bool has1, float g, float dist, float lp, float& ds0,
                                               float& ds1, float& dp0, float& dp1, float& do0, float& do1) {
  dp1 = 0.f;
  if (SCORER == KGE_DISTMULT) {
    ds0 = g * (r0 * o0); ds1 = g * (r1 * o1);
    dp0 = g * (s0 * o0); dp1 = g * (s1 * o1);
    do0 = g * (s0 * r0); do1 = g * (s1 * r1);
  } else if (SCORER == KGE_COMPLEX) {
    ds0 = g * (o0 * r0 + o1 * r1); ds1 = g * (o1 * r0 - o0 * r1);
    dp0 = g * (o0 * s0 + o1 * s1); dp1 = g * (o1 * s0 - o0 * s1);
    do0 = g * (s0 * r0 - s1 * r1); do1 = g * (s1 * r0 + s0 * r1);
  } else if (SCORER == KGE_TRANSE) {
    const float e0 = ((s0 + r0) - o0) + 1e-6f, e1 = ((s1 + r1) - o1) + 1e-6f;
    const float w0 = -g * transe_w<NORM>(e0, dist, lp);
    const float w1 = has1 ? -g * transe_w<NORM>(e1, dist, lp) : 0.f;
    ds0 = w0; ds1 = w1; dp0 = w0; dp1 = w1; do0 = -w0; do1 = -w1;
  } else {
    float sn, cs;
    if constexpr (ROTPRE) {
      cs = r0;
      sn = r1;
    } else {
      sincos_canon(r0, sn, cs);
    }
    const float q0 = s0 * cs - s1 * sn, q1 = s0 * sn + s1 * cs;
    float wre, wim;
    rotate_w<NORM>(q0 - o0, q1 - o1, dist, lp, wre, wim);
    const float dq0 = -g * wre, dq1 = -g * wim;
    ds0 = dq0 * cs + dq1 * sn; ds1 = dq1 * cs - dq0 * sn;
    dp0 = dq1 * q0 - dq0 * q1;
    do0 = -dq0; do1 = -dq1;
  }
}

}  // namespace kge
