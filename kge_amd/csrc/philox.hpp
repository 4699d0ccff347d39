// philox.hpp -- the counter-based generator shared by the device sampler (neg_sample.hip) and the embedder dropout of
// the triple-wise kernels (score_spo.hip, bwd.hip, embed.hip), and the ONE definition of the dropout mask
// (include/kge_amd.h, "Embedder dropout").
//
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): no state, no library; a block is a pure function of
// (counter, key), so a backward kernel regenerates the forward's mask from (seed, call) alone.
#pragma once
#include "common.hpp"

namespace kge {

struct Philox4 {
  unsigned r0, r1, r2, r3;
};

__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

// ---- embedder dropout (lookup_embedder.py:96-105: torch.nn.Dropout on every gathered row) -----------------------------
// element c of a gathered row occurrence is DROPPED iff word (c % 4) of Philox4x32-10(counter, key) < thr, with
//   counter = (c / 4, occ, (uint32)call, role)      role: 0 = s row, 1 = p row, 2 = o row
//   key     = (seed low 32, (seed high 32) ^ KGE_DROPOUT_KEY_XOR)      (apart from the sampler's streams of the same seed)
//   thr     = (uint32)floor(p * 2^32)               (host, in double)
// kept: x * scale, scale = 1.0f / (1.0f - p) (host, float32); dropped: x * 0.0f.  thr == 0: the row passes untouched.
constexpr unsigned KGE_DROPOUT_KEY_XOR = 0x44524F50u;

struct DropKey {  // per call
  unsigned k0, k1, call;
  unsigned thr_ent, thr_rel;
  float sc_ent, sc_rel;
};

struct RowMask {  // per gathered row occurrence
  unsigned occ, role, thr;
  float scale;
};

__host__ __device__ __forceinline__ RowMask ent_mask(const DropKey& k, unsigned role, unsigned occ) {
  return RowMask{occ, role, k.thr_ent, k.sc_ent};
}
__host__ __device__ __forceinline__ RowMask rel_mask(const DropKey& k, unsigned occ) {
  return RowMask{occ, 1u, k.thr_rel, k.sc_rel};
}

// the mask factor of column `col` of the row: 0.0f or scale
__device__ __forceinline__ float drop_factor(int col, const RowMask& m, const DropKey& k) {
  if (m.thr == 0) return m.scale;  // (p == 0: scale == 1)
  const Philox4 r = philox4x32_10((unsigned)(col >> 2), m.occ, k.call, m.role, k.k0, k.k1);
  const int w = col & 3;
  const unsigned u = w == 0 ? r.r0 : (w == 1 ? r.r1 : (w == 2 ? r.r2 : r.r3));
  return u < m.thr ? 0.0f : m.scale;
}

// the mask on the 8 columns [col0, col0 + 8) held by one lane: two Philox blocks (ALIGNED: col0 % 4 == 0, the vector
// path), three where the chunk straddles block boundaries
template <bool ALIGNED>
__device__ __forceinline__ void mask_chunk(f32x8& x, int col0, const RowMask& m, const DropKey& k) {
  if (m.thr == 0) return;  // bit for bit
  constexpr int NQ = ALIGNED ? 2 : 3;
  unsigned w[4 * NQ];
  const unsigned q0 = (unsigned)(col0 >> 2);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const Philox4 r = philox4x32_10(q0 + q, m.occ, k.call, m.role, k.k0, k.k1);
    w[4 * q] = r.r0; w[4 * q + 1] = r.r1; w[4 * q + 2] = r.r2; w[4 * q + 3] = r.r3;
  }
  const int a = ALIGNED ? 0 : (col0 & 3);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    unsigned u = w[i];
    if (!ALIGNED) u = a == 0 ? w[i] : (a == 1 ? w[i + 1] : (a == 2 ? w[i + 2] : w[i + 3]));
    x.v[i] = x.v[i] * (u < m.thr ? 0.0f : m.scale);
  }
}

}  // namespace kge
