// transh_device.hpp -- the canonical arithmetic of TransH (kge/model/transh.py:39-78), defined ONCE: every TransH
// kernel of transh.hip scores a pair through these functions, so a pair's score is a pure function of its three rows
// and l_norm.  Compiled with -ffp-contract=off: one rounding per written operation, fused
// multiply-adds only where __builtin_fmaf stands.
//
// A relation row is [d_r | w_r] (torch.chunk(p_emb, 2, dim=1)).  With eps = 1e-6 (F.pairwise_distance) and
// w^ = w / max(||w||_2, 1e-12) (F.normalize):
//   nw2     = sum_k w_k w_k                          REDUCE8, fma chain
//   den     = max(sqrt_rn(nw2), 1e-12)
//   w^_k    = w_k / den                              IEEE division
//   a(e)    = sum_k w^_k e_k                         REDUCE8, fma chain
//   fixed_k = fma(-a(q), w^_k, q_k) + d_k            sp_ / spo / neg (q = s);   ... - d_k for _po (q = o)
//   v_k     = fma(a(t), w^_k, fixed_k - t_k) + eps   t = the row on the other side (o; for _po: s)
//   acc     = sum_k |v_k|  (L1, plain adds)  or  sum_k v_k v_k  (L2, fma chain)      REDUCE8
//   score   = -acc (L1),  -sqrt_rn(acc) (L2)
// REDUCE8: the coordinates are cut into groups of four (k / 4); group c goes to partial sum c mod 8; a partial sum
// takes its coordinates in ascending k, starting from +0; the eight partial sums are then added as the xor butterfly
// of an 8-lane group does it (offsets 4, 2, 1):  ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)).
// Coordinates k >= d do not exist: they enter no sum (a zero-padded coordinate of the two fma-chain dot products adds
// fma(0, 0, acc) = acc exactly, which the tiled kernel uses; the norm's sum is guarded).
#pragma once
#include "common.hpp"

namespace kge {

constexpr float TH_EPS = 1e-6f;        // F.pairwise_distance's eps, added to every component of the difference
constexpr float TH_NORM_EPS = 1e-12f;  // F.normalize's eps

__device__ __forceinline__ float th_combine8(const float* p) {
  return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]));
}
// the same sum over the 8 lanes of a group (all eight active)
__device__ __forceinline__ float th_butterfly8(float P) {
  P = P + __shfl_xor(P, 4, 64);
  P = P + __shfl_xor(P, 2, 64);
  P = P + __shfl_xor(P, 1, 64);
  return P;
}
__device__ __forceinline__ float th_den(float nw2) { return __builtin_fmaxf(sqrt_rn(nw2), TH_NORM_EPS); }
__device__ __forceinline__ float th_what(float w, float den) { return __fdiv_rn(w, den); }
// DSIGN = +1: (e - a w^) + d_r   (sp_, spo, neg);   -1: (e - a w^) - d_r   (_po)
template <int DSIGN>
__device__ __forceinline__ float th_fixed(float e, float wh, float a, float dr) {
  const float pe = __builtin_fmaf(-a, wh, e);
  return DSIGN > 0 ? pe + dr : pe - dr;
}
__device__ __forceinline__ float th_v(float fixed, float t, float c, float wh) {
  return __builtin_fmaf(c, wh, fixed - t) + TH_EPS;
}
template <int NORM>
__device__ __forceinline__ float th_acc(float acc, float v) {
  return NORM == NORM_L1 ? acc + __builtin_fabsf(v) : __builtin_fmaf(v, v, acc);
}
template <int NORM>
__device__ __forceinline__ float th_score(float acc) {
  return NORM == NORM_L1 ? -acc : -sqrt_rn(acc);
}

// four coordinates k0 .. k0 + 3 of a row; the element path reads one float at a time and gives 0 behind the row's end
template <bool VEC>
__device__ __forceinline__ f32x4 th_ld4(const float* row, int k0, int d) {
  if (VEC) return ld4<float>(row + k0);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (k0 + i < d) ? row[k0 + i] : 0.0f;
  return r;
}

// ---- the row-wise form: an 8-lane group per row, lane lg takes the groups of four c = lg, lg + 8, ... ----
template <bool VEC>
__device__ __forceinline__ float th_group_nw2(const float* w, int d, int lg) {
  float P = 0.0f;
  for (int k0 = lg * 4; k0 < d; k0 += 32) {
    const f32x4 x = th_ld4<VEC>(w, k0, d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (VEC || k0 + i < d) P = __builtin_fmaf(x[i], x[i], P);
  }
  return th_butterfly8(P);
}
template <bool VEC>
__device__ __forceinline__ float th_group_dot(const float* w, float den, const float* e, int d, int lg) {
  float P = 0.0f;
  for (int k0 = lg * 4; k0 < d; k0 += 32) {
    const f32x4 x = th_ld4<VEC>(w, k0, d), y = th_ld4<VEC>(e, k0, d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (VEC || k0 + i < d) P = __builtin_fmaf(th_what(x[i], den), y[i], P);
  }
  return th_butterfly8(P);
}
// the triple form: score(q, r, t) with a_q = a(q), c_t = a(t) already reduced
template <int NORM, bool VEC>
__device__ __forceinline__ float th_group_score(const float* q, const float* dr, const float* w, const float* t, float den,
                                                float a_q, float c_t, int d, int lg) {
  float P = 0.0f;
  for (int k0 = lg * 4; k0 < d; k0 += 32) {
    const f32x4 xq = th_ld4<VEC>(q, k0, d), xd = th_ld4<VEC>(dr, k0, d), xw = th_ld4<VEC>(w, k0, d),
                xt = th_ld4<VEC>(t, k0, d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (VEC || k0 + i < d) {
        const float wh = th_what(xw[i], den);
        P = th_acc<NORM>(P, th_v(th_fixed<1>(xq[i], wh, a_q, xd[i]), xt[i], c_t, wh));
      }
  }
  return th_score<NORM>(th_butterfly8(P));
}

}  // namespace kge
