// spo_device.hpp -- device pieces of the row-wise scoring kernels (score_spo.hip, score_neg_shared.hip, score_so.hip): one
// lane's chunk of 8 coordinates, the fixed side of a triple, the per-chunk arithmetic and the group butterfly.  One
// definition, so that every kernel built from them produces the same bits.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "philox.hpp"

namespace kge {

// per-lane chunk of 8 coordinates of one row (first half and, for complex scorers,
// second half)
template <typename T, bool VEC>
__device__ __forceinline__ f32x8 load_chunk(const T* row, int c0, int limit) {
  if (VEC) return ld8<T>(row + c0);
  f32x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (c0 + i < limit) ? ld1<T>(row + c0 + i) : 0.0f;
  return r;
}

template <int SCORER>
struct IsComplex {
  static constexpr bool value = (SCORER == KGE_COMPLEX || SCORER == KGE_ROTATE);
};

// Per-lane state that does not depend on the corrupted slot ("fixed side").
struct Fixed {
  f32x8 f0, f1, f2, f3;
};

// slot == 2 (object varies; also plain score_spo): fixed side = query vector q(s, r).
// slot == 0 (subject varies): fixed side = relation (or its cos/sin) and the object.
// e0/e1: halves of the fixed ENTITY row, r0/r1: relation row halves (RotatE: r0 = phases).
template <int SCORER>
__device__ __forceinline__ Fixed prep_chunk(int slot, const f32x8& e0, const f32x8& e1,
                                            const f32x8& r0, const f32x8& r1) {
  Fixed F;
  F.f0 = r0; F.f1 = r1; F.f2 = e0; F.f3 = e1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (slot != 0) {
      if (SCORER == KGE_DISTMULT) {
        F.f0.v[i] = e0.v[i] * r0.v[i];
      } else if (SCORER == KGE_COMPLEX) {
        F.f0.v[i] = e0.v[i] * r0.v[i] - e1.v[i] * r1.v[i];
        F.f1.v[i] = e1.v[i] * r0.v[i] + e0.v[i] * r1.v[i];
      } else if (SCORER == KGE_TRANSE) {
        F.f0.v[i] = e0.v[i] + r0.v[i];
      } else {
        float sn, cs;
        sincos_canon(r0.v[i], sn, cs);
        F.f0.v[i] = e0.v[i] * cs - e1.v[i] * sn;
        F.f1.v[i] = e0.v[i] * sn + e1.v[i] * cs;
      }
    } else if (SCORER == KGE_ROTATE) {
      float sn, cs;
      sincos_canon(r0.v[i], sn, cs);
      F.f0.v[i] = cs;
      F.f1.v[i] = sn;
    }
  }
  return F;
}

// score_so.hip: the query q(s, r) of one chunk as prep_chunk<SCORER>(2, ...) forms it, for a relation row that was
// staged once and is shared by many (s, o) pairs.  RotatE: r0 / r1 are cos / sin of the row's phases (sincos_canon
// evaluated where the row was staged, not per pair) and enter the expressions of prep_chunk above unchanged; the other
// scorers: prep_chunk itself.  Same operations in the same order (-ffp-contract=off): the same bits.
template <int SCORER>
__device__ __forceinline__ Fixed prep_chunk_staged(const f32x8& e0, const f32x8& e1, const f32x8& r0,
                                                   const f32x8& r1) {
  if constexpr (SCORER != KGE_ROTATE) {
    return prep_chunk<SCORER>(2, e0, e1, r0, r1);
  } else {
    Fixed F;
    F.f0 = r0; F.f1 = r1; F.f2 = e0; F.f3 = e1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float cs = r0.v[i], sn = r1.v[i];
      F.f0.v[i] = e0.v[i] * cs - e1.v[i] * sn;
      F.f1.v[i] = e0.v[i] * sn + e1.v[i] * cs;
    }
    return F;
  }
}

// accumulate one chunk (x0/x1 = halves of the varying entity row) into the lane partial P
template <int SCORER, int NORM>
__device__ __forceinline__ float apply_chunk(int slot, float P, const Fixed& F,
                                             const f32x8& x0, const f32x8& x1, int cnt,
                                             float lp) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < cnt) {
      if (SCORER == KGE_DISTMULT) {
        if (slot != 0) P = __builtin_fmaf(F.f0.v[i], x0.v[i], P);
        else P = __builtin_fmaf(x0.v[i] * F.f0.v[i], F.f2.v[i], P);
      } else if (SCORER == KGE_COMPLEX) {
        float qre, qim, ore, oim;
        if (slot != 0) {
          qre = F.f0.v[i]; qim = F.f1.v[i]; ore = x0.v[i]; oim = x1.v[i];
        } else {
          qre = x0.v[i] * F.f0.v[i] - x1.v[i] * F.f1.v[i];
          qim = x1.v[i] * F.f0.v[i] + x0.v[i] * F.f1.v[i];
          ore = F.f2.v[i]; oim = F.f3.v[i];
        }
        P = __builtin_fmaf(qre, ore, P);
        P = __builtin_fmaf(qim, oim, P);
      } else if (SCORER == KGE_TRANSE) {
        float df;  // F.pairwise_distance adds eps=1e-6 to every component (transe.py:18)
        if (slot != 0) df = (F.f0.v[i] - x0.v[i]) + 1e-6f;
        else df = ((x0.v[i] + F.f0.v[i]) - F.f2.v[i]) + 1e-6f;
        P = norm_acc<NORM>(P, __builtin_fabsf(df), lp);
      } else {  // ROTATE
        float qre, qim, ore, oim;
        if (slot != 0) {
          qre = F.f0.v[i]; qim = F.f1.v[i]; ore = x0.v[i]; oim = x1.v[i];
        } else {
          qre = x0.v[i] * F.f0.v[i] - x1.v[i] * F.f1.v[i];
          qim = x0.v[i] * F.f1.v[i] + x1.v[i] * F.f0.v[i];
          ore = F.f2.v[i]; oim = F.f3.v[i];
        }
        float dre = qre - ore, dim_ = qim - oim;
        float ab = sqrt_rn_fast(__builtin_fmaf(dim_, dim_, dre * dre));  // (correctly rounded: common.hpp)
        P = norm_acc<NORM>(P, ab, lp);
      }
    }
  }
  return P;
}

// one lane's chunk of the half of a row that starts at column `half` (0 or h), with the embedder dropout of that row
// occurrence applied where the chunk reaches the registers (DROP; philox.hpp): everything after the load is the
// arithmetic of the undropped kernel.  VEC implies half % 4 == 0 and c0 % 8 == 0 (vec_ok): two Philox blocks per chunk.
template <typename T, bool VEC, bool DROP>
__device__ __forceinline__ f32x8 load_chunk_d(const T* row, int half, int c0, int limit, const RowMask& m,
                                              const DropKey& k) {
  f32x8 r = load_chunk<T, VEC>(row + half, c0, limit);
  if constexpr (DROP) mask_chunk<VEC>(r, half + c0, m, k);
  return r;
}

// load the fixed side of chunk c0 for (entity row erow, relation row rrow)
template <int SCORER, typename T, bool VEC, bool DROP>
__device__ __forceinline__ Fixed load_fixed_d(int slot, const T* erow, const T* rrow, int c0, int D, int h,
                                              const RowMask& em, const RowMask& rm, const DropKey& k) {
  constexpr bool CPLX = (SCORER == KGE_COMPLEX || SCORER == KGE_ROTATE);
  f32x8 e0 = load_chunk_d<T, VEC, DROP>(erow, 0, c0, D, em, k);
  f32x8 r0 = load_chunk_d<T, VEC, DROP>(rrow, 0, c0, D, rm, k);
  f32x8 e1 = e0, r1 = r0;
  if (CPLX) e1 = load_chunk_d<T, VEC, DROP>(erow, h, c0, D, em, k);
  if (SCORER == KGE_COMPLEX) r1 = load_chunk_d<T, VEC, DROP>(rrow, h, c0, D, rm, k);
  return prep_chunk<SCORER>(slot, e0, e1, r0, r1);
}

template <int SCORER, typename T, bool VEC>
__device__ __forceinline__ Fixed load_fixed(int slot, const T* erow, const T* rrow, int c0,
                                            int D, int h) {
  return load_fixed_d<SCORER, T, VEC, false>(slot, erow, rrow, c0, D, h, RowMask{}, RowMask{}, DropKey{});
}

template <int SCORER, int NORM>
__device__ __forceinline__ float finalize(float acc, float lp) {
  if (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT) return acc;
  if (NORM == NORM_L1) return -acc;
  if (NORM == NORM_L2) return -__builtin_sqrtf(acc);
  return -powf(acc, 1.0f / lp);
}

template <int G>
__device__ __forceinline__ float group_butterfly(float P) {
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) P = P + __shfl_xor(P, off, 64);
  return P;
}

// ---- host-side helpers of the dispatch ------------------------------------------------------
static inline int group_size(int D) {
  int nchunks = (D + 7) / 8;
  int G = 8;  // groups narrower than 8 lanes are not instantiated (idle lanes add +0)
  while (G < nchunks && G < 64) G <<= 1;
  return G;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// can every 8-coordinate chunk be read with aligned vector loads?
static bool vec_ok(int scorer, int dtype, int d, int dr, const Operand& S, const Operand& R,
                   const Operand& O) {
  const int es = dtype == KGE_BF16 ? 2 : 4;
  const bool cplx = scorer == KGE_COMPLEX || scorer == KGE_ROTATE;
  const int D = cplx ? d / 2 : d;
  if (D % 8) return false;
  if (!aligned16(S.base) || !aligned16(R.base) || !aligned16(O.base)) return false;
  if ((S.ld * es) % 16 || (R.ld * es) % 16 || (O.ld * es) % 16) return false;
  if (cplx && ((long long)(d / 2) * es) % 16) return false;
  return true;
}

}  // namespace kge
