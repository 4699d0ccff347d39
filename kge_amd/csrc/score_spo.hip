// score_spo.hip -- row-wise triple scoring: KgeModel.score_spo (kge_model.py:663-680)
// and the negative-sampling "triple" path (sampler.py:291-306), gfx950.
//
// HBM-gather bound: per scored triple one corrupted-slot row (d*elt bytes) is
// algorithmically required.  A group of G lanes (G = power of two
// >= D/8, D = number of reduction coordinates) owns one triple; lane g of the group
// owns coordinates [8g, 8g+8) (+ 8*64*t when D > 512) and reads them with 16/32-byte
// vector loads, so a group reads whole contiguous row segments.  The row reduction is
// the canonical "64 strided partials + xor butterfly" of oracle/kge_oracle.c
// (spo_score): levels with offset >= G add an exact +0 and are skipped.
#include "spo_device.hpp"

namespace kge {

// ---- score_spo ----------------------------------------------------------------------
// DROP: the embedder dropout of the three gathered rows of triple `row` (occurrence `row`, roles 0 / 1 / 2), applied
// where a chunk is loaded (spo_device.hpp); DROP == false is the kernel as it was, `dk` unused.
template <int SCORER, typename T, int NORM, bool VEC, int G, bool DROP>
__device__ __forceinline__ void spo_body(const Operand& S, const Operand& R, const Operand& O, int d, int dr,
                                         long long n, float lp, float* __restrict__ out, const DropKey& dk) {
  constexpr bool CPLX = IsComplex<SCORER>::value;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int RPW = 64 / G;  // rows per wave
  const int lg = lane & (G - 1);
  const long long row = ((long long)blockIdx.x * 4 + wave) * RPW + (lane / G);
  const bool valid = row < n;
  const int h = d / 2;
  const int D = CPLX ? h : d;
  const int nchunks = (D + 7) / 8;
  float P = 0.0f;
  if (valid) {
    const T* srow = (const T*)S.base + index_at(S.idx, row) * S.ld;
    const T* rrow = (const T*)R.base + index_at(R.idx, row) * R.ld;
    const T* orow = (const T*)O.base + index_at(O.idx, row) * O.ld;
    for (int ci = lg; ci < nchunks; ci += 64) {  // G < 64 implies nchunks <= G: one trip
      const int c0 = ci * 8;
      const int cnt = (D - c0 < 8) ? (D - c0) : 8;
      const RowMask ms = ent_mask(dk, 0u, (unsigned)row), mp = rel_mask(dk, (unsigned)row),
                    mo = ent_mask(dk, 2u, (unsigned)row);
      Fixed F = load_fixed_d<SCORER, T, VEC, DROP>(2, srow, rrow, c0, D, h, ms, mp, dk);
      f32x8 x0 = load_chunk_d<T, VEC, DROP>(orow, 0, c0, D, mo, dk);
      f32x8 x1 = x0;
      if (CPLX) x1 = load_chunk_d<T, VEC, DROP>(orow, h, c0, D, mo, dk);
      P = apply_chunk<SCORER, NORM>(2, P, F, x0, x1, VEC ? 8 : cnt, lp);
    }
  }
  P = group_butterfly<G>(P);
  if (valid && lg == 0) out[row] = finalize<SCORER, NORM>(P, lp);
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256) void spo_kernel(Operand S, Operand R, Operand O, int d,
                                                  int dr, long long n, float lp,
                                                  float* __restrict__ out) {
  spo_body<SCORER, T, NORM, VEC, G, false>(S, R, O, d, dr, n, lp, out, DropKey{});
}

template <int SCORER, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256) void spo_drop_kernel(Operand S, Operand R, Operand O, int d, int dr, long long n,
                                                       float lp, float* __restrict__ out, DropKey dk) {
  spo_body<SCORER, float, NORM, VEC, G, true>(S, R, O, d, dr, n, lp, out, dk);
}

// ---- negative sampling, "triple" semantics ---------------------------------------------
// grid.y = positive row i; the block's groups stride over that row's K negatives.  The
// non-corrupted entity row and the relation row are loaded ONCE per group into registers
// (one chunk per lane; D <= 512) so only the corrupted-slot row streams from HBM.
// DROP: the two fixed rows of positive i carry the masks of occurrence i (roles 1 and 0 / 2), generated once per group
// where the fixed side is loaded; the corrupted row of (i, k) carries the mask of occurrence i K + k, role = slot.
template <int SCORER, typename T, int NORM, bool VEC, int G, bool DROP>
__device__ __forceinline__ void neg_body(const Operand& S, const Operand& R, const Operand& O, int d, int dr, int slot,
                                         const void* neg, int neg_itype, long long neg_ld, long long K, float lp,
                                         float* __restrict__ out, long long ldo, const DropKey& dk) {
  constexpr bool CPLX = IsComplex<SCORER>::value;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int GPW = 64 / G;
  constexpr int GPB = 4 * GPW;  // groups per block
  const int lg = lane & (G - 1);
  const int gid = wave * GPW + lane / G;
  const long long i = blockIdx.y;
  const int h = d / 2;
  const int D = CPLX ? h : d;
  const int nchunks = (D + 7) / 8;
  const T* ent = (const T*)S.base;  // S.base == O.base == entity table
  const T* fixrow = ent + index_at(slot == 0 ? O.idx : S.idx, i) * S.ld;
  const T* rrow = (const T*)R.base + index_at(R.idx, i) * R.ld;
  const Index nix = {neg, 1, neg_itype};

  // first chunk of the fixed side lives in registers for the whole negative loop
  Fixed F0;
  const int c00 = lg * 8;
  const int cnt0 = (D - c00 < 8) ? (D - c00) : 8;
  const RowMask mf = ent_mask(dk, slot == 0 ? 2u : 0u, (unsigned)i), mp = rel_mask(dk, (unsigned)i);
  if (lg < nchunks) F0 = load_fixed_d<SCORER, T, VEC, DROP>(slot, fixrow, rrow, c00, D, h, mf, mp, dk);

  // The slot is uniform over the launch: one specialised copy of the loop per side keeps the
  // side selection out of the per-coordinate arithmetic; on the vector path every chunk is full
  // (D % 8 == 0), so the per-coordinate tail test folds away as well.
  auto sweep = [&](auto slot_c) {
    constexpr int SLOT = decltype(slot_c)::value;
    const long long step = (long long)gridDim.x * GPB;
    const bool act = lg < nchunks;
    auto row_of = [&](long long kk) { return ent + index_at(nix, i * neg_ld + kk) * S.ld; };
    auto load_x = [&](const T* xr, f32x8& a, f32x8& b, const RowMask& mx) {
      a = load_chunk_d<T, VEC, DROP>(xr, 0, c00, D, mx, dk);
      b = a;
      if (CPLX) b = load_chunk_d<T, VEC, DROP>(xr, h, c00, D, mx, dk);
    };
    // No software pipeline: prefetching the next negative's index (RotatE 159 -> 167 us) or its
    // index and row (159 -> 270 us, TransE 138 -> 145 us) was slower on MI355X than leaving the
    // latency to the 4..8 resident waves per SIMD -- the extra live registers cost occupancy.
    for (long long k = (long long)blockIdx.x * GPB + gid; k < K; k += step) {
      const T* rc = row_of(k);
      const RowMask mx = ent_mask(dk, (unsigned)SLOT, (unsigned)(i * K + k));
      float P = 0.0f;
      if (act) {
        f32x8 x0, x1;
        load_x(rc, x0, x1, mx);
        P = apply_chunk<SCORER, NORM>(SLOT, P, F0, x0, x1, VEC ? 8 : cnt0, lp);
      }
      for (int ci = lg + 64; ci < nchunks; ci += 64) {  // only when D > 512
        const int c0 = ci * 8;
        const int cnt = (D - c0 < 8) ? (D - c0) : 8;
        Fixed F = load_fixed_d<SCORER, T, VEC, DROP>(SLOT, fixrow, rrow, c0, D, h, mf, mp, dk);
        f32x8 y0 = load_chunk_d<T, VEC, DROP>(rc, 0, c0, D, mx, dk);
        f32x8 y1 = y0;
        if (CPLX) y1 = load_chunk_d<T, VEC, DROP>(rc, h, c0, D, mx, dk);
        P = apply_chunk<SCORER, NORM>(SLOT, P, F, y0, y1, VEC ? 8 : cnt, lp);
      }
      P = group_butterfly<G>(P);
      if (lg == 0) out[i * ldo + k] = finalize<SCORER, NORM>(P, lp);
    }
  };
  if (slot == 0) sweep(std::integral_constant<int, 0>{});
  else sweep(std::integral_constant<int, 2>{});
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256, 4) void neg_kernel(Operand S, Operand R, Operand O, int d,
                                                  int dr, int slot, const void* neg,
                                                  int neg_itype, long long neg_ld,
                                                  long long K, float lp,
                                                  float* __restrict__ out, long long ldo) {
  neg_body<SCORER, T, NORM, VEC, G, false>(S, R, O, d, dr, slot, neg, neg_itype, neg_ld, K, lp, out, ldo, DropKey{});
}

template <int SCORER, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256, 4) void neg_drop_kernel(Operand S, Operand R, Operand O, int d, int dr, int slot,
                                                          const void* neg, int neg_itype, long long neg_ld, long long K,
                                                          float lp, float* __restrict__ out, long long ldo, DropKey dk) {
  neg_body<SCORER, float, NORM, VEC, G, true>(S, R, O, d, dr, slot, neg, neg_itype, neg_ld, K, lp, out, ldo, dk);
}


template <int SCORER, typename T, int NORM, bool VEC>
static int launch_spo_g(int G, const Operand& S, const Operand& R, const Operand& O, int d,
                        int dr, long long n, float lp, float* out, hipStream_t st, const DropKey* dk) {
#define KGE_SPO_CASE(GG)                                                                 \
  case GG: {                                                                             \
    long long rows_per_block = 4LL * (64 / GG);                                          \
    unsigned grid = (unsigned)((n + rows_per_block - 1) / rows_per_block);               \
    if constexpr (std::is_same<T, float>::value) {                                       \
      if (dk) {                                                                          \
        hipLaunchKernelGGL((spo_drop_kernel<SCORER, NORM, VEC, GG>), dim3(grid), dim3(256), 0, st, S, R, O, d, dr, n, \
                           lp, out, *dk);                                                \
        break;                                                                           \
      }                                                                                  \
    }                                                                                    \
    hipLaunchKernelGGL((spo_kernel<SCORER, T, NORM, VEC, GG>), dim3(grid), dim3(256), 0, \
                       st, S, R, O, d, dr, n, lp, out);                                  \
    break;                                                                               \
  }
  switch (G) {
    KGE_SPO_CASE(8)
    KGE_SPO_CASE(16)
    KGE_SPO_CASE(32)
    KGE_SPO_CASE(64)
    default:
      return KGE_ERR_UNSUPPORTED;
  }
#undef KGE_SPO_CASE
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, typename T, int NORM, bool VEC>
static int launch_neg_g(int G, const Operand& S, const Operand& R, const Operand& O, int d,
                        int dr, long long n, int slot, const void* neg, int neg_itype,
                        long long neg_ld, long long K, float lp, float* out, long long ldo,
                        hipStream_t st, const DropKey* dk) {
#define KGE_NEG_CASE(GG)                                                                   \
  case GG: {                                                                               \
    long long gpb = 4LL * (64 / GG);                                                       \
    /* negatives per group: 16 amortises the group's fixed side (two row loads, RotatE: */  \
    /* sin/cos), 4 when that would leave fewer than ~2048 workgroups */                    \
    long long per = 16;                                                                    \
    while (per > 4 && n * ((K + gpb * per - 1) / (gpb * per)) < 2048) per >>= 1;           \
    long long bx = (K + gpb * per - 1) / (gpb * per);                                      \
    if (bx < 1) bx = 1;                                                                    \
    if (bx > 64) bx = 64;                                                                  \
    if constexpr (std::is_same<T, float>::value) {                                         \
      if (dk) {                                                                            \
        hipLaunchKernelGGL((neg_drop_kernel<SCORER, NORM, VEC, GG>), dim3((unsigned)bx, (unsigned)n), dim3(256), 0, st, \
                           S, R, O, d, dr, slot, neg, neg_itype, neg_ld, K, lp, out, ldo, *dk); \
        break;                                                                             \
      }                                                                                    \
    }                                                                                      \
    hipLaunchKernelGGL((neg_kernel<SCORER, T, NORM, VEC, GG>), dim3((unsigned)bx, (unsigned)n), \
                       dim3(256), 0, st, S, R, O, d, dr, slot, neg, neg_itype, neg_ld, K,  \
                       lp, out, ldo);                                                      \
    break;                                                                                 \
  }
  switch (G) {
    KGE_NEG_CASE(8)
    KGE_NEG_CASE(16)
    KGE_NEG_CASE(32)
    KGE_NEG_CASE(64)
    default:
      return KGE_ERR_UNSUPPORTED;
  }
#undef KGE_NEG_CASE
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}


template <int SCORER, typename T>
static int dispatch_spo(bool neg_mode, int norm, bool vec, int G, const Operand& S,
                        const Operand& R, const Operand& O, int d, int dr, long long n,
                        int slot, const void* neg, int neg_itype, long long neg_ld,
                        long long K, float lp, float* out, long long ldo, hipStream_t st,
                        const DropKey* dk) {
#define KGE_GO(NORM, VEC)                                                                \
  return neg_mode ? launch_neg_g<SCORER, T, NORM, VEC>(G, S, R, O, d, dr, n, slot, neg,  \
                                                        neg_itype, neg_ld, K, lp, out,   \
                                                        ldo, st, dk)                     \
                  : launch_spo_g<SCORER, T, NORM, VEC>(G, S, R, O, d, dr, n, lp, out, st, dk)
  if constexpr (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT) {
    (void)norm;  // no norm: a single instantiation
    if (vec) { KGE_GO(NORM_L1, true); } else { KGE_GO(NORM_L1, false); }
  } else {
    if (norm == NORM_L1) {
      if (vec) { KGE_GO(NORM_L1, true); } else { KGE_GO(NORM_L1, false); }
    } else if (norm == NORM_L2) {
      if (vec) { KGE_GO(NORM_L2, true); } else { KGE_GO(NORM_L2, false); }
    } else {
      if (vec) { KGE_GO(NORM_LP, true); } else { KGE_GO(NORM_LP, false); }
    }
  }
#undef KGE_GO
}

static int run_spo_impl(int scorer, int dtype, bool neg_mode, const Operand& S, const Operand& R,
                        const Operand& O, int d, int dr, long long n, int slot, const void* neg,
                        int neg_itype, long long neg_ld, long long K, float lp, float* out,
                        long long ldo, hipStream_t st, const DropKey* dk) {
  if (n == 0 || (neg_mode && K == 0)) return KGE_OK;
  const bool cplx = scorer == KGE_COMPLEX || scorer == KGE_ROTATE;
  if (cplx && (d % 2)) return KGE_ERR_INVALID_ARG;
  const int D = cplx ? d / 2 : d;
  const int G = group_size(D);
  const bool vec = vec_ok(scorer, dtype, d, dr, S, R, O);
  const int norm = norm_mode(lp);
#define KGE_DT(SC)                                                                        \
  return dtype == KGE_BF16                                                                \
             ? dispatch_spo<SC, unsigned short>(neg_mode, norm, vec, G, S, R, O, d, dr, n, \
                                                slot, neg, neg_itype, neg_ld, K, lp, out,  \
                                                ldo, st, nullptr)                          \
             : dispatch_spo<SC, float>(neg_mode, norm, vec, G, S, R, O, d, dr, n, slot,    \
                                       neg, neg_itype, neg_ld, K, lp, out, ldo, st, dk)
  switch (scorer) {
    case KGE_COMPLEX: KGE_DT(KGE_COMPLEX);
    case KGE_DISTMULT: KGE_DT(KGE_DISTMULT);
    case KGE_TRANSE: KGE_DT(KGE_TRANSE);
    case KGE_ROTATE: KGE_DT(KGE_ROTATE);
  }
#undef KGE_DT
  return KGE_ERR_INVALID_ARG;
}

int run_spo(int scorer, int dtype, bool neg_mode, const Operand& S, const Operand& R,
            const Operand& O, int d, int dr, long long n, int slot, const void* neg,
            int neg_itype, long long neg_ld, long long K, float lp, float* out,
            long long ldo, hipStream_t st) {
  return run_spo_impl(scorer, dtype, neg_mode, S, R, O, d, dr, n, slot, neg, neg_itype, neg_ld, K, lp, out, ldo, st,
                      nullptr);
}

// kge_score_spo_dropout / kge_score_neg_dropout: float32 tables, the same dispatch, the kernels with DROP
int run_spo_drop(int scorer, bool neg_mode, const Operand& S, const Operand& R, const Operand& O, int d, int dr,
                 long long n, int slot, const void* neg, int neg_itype, long long neg_ld, long long K, float lp,
                 float* out, long long ldo, const DropKey& dk, hipStream_t st) {
  return run_spo_impl(scorer, KGE_F32, neg_mode, S, R, O, d, dr, n, slot, neg, neg_itype, neg_ld, K, lp, out, ldo, st,
                      &dk);
}

}  // namespace kge
