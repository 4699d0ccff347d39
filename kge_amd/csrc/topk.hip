// topk.hip -- filtered top-k link prediction, gfx950: the k best entities of (s, p, ?) / (?, p, o) without the [n, E]
// score matrix.  What it replaces in the reference: KgeModel.score_sp / score_po (kge_model.py:682-725), the masking of
// EntityRankingJob._filter_and_rank (eval_entity_ranking.py:233-313) and torch.topk over the masked scores.
//
//   topk_select_kernel  the 64 x 64 tile walk of pairs_kernel (score_pairs.hip) on the canonical chain: the
//                       same gather, query build, MFMA / micro-tile chain through pairs_device.hpp, so every score has
//                       the bits kge_score_sp / kge_score_po store.  A finished tile goes through the operand buffers
//                       (as pairs_kernel's counting epilogue does) and is consumed there: each of the workgroup's 64
//                       rows keeps a sorted list of its k best 64-bit keys in LDS.  The lists leave the workgroup once.
//   topk_merge_kernel   one wave per row merges the `groups` sorted lists into the best k and unpacks them.
//
// Key: high word = the order-preserving unsigned image of the canonical score (NaN -> -inf, -0.0 -> +0.0),
// low word = 0xFFFFFFFF - j (j = the column inside the scored slice).  A larger key is better; equal scores order by
// ascending entity id; every real column has a non-zero key (j <= 2^32 - 2) and 0 means "empty".  The keys of a row are
// pairwise distinct, so the best k of their union is one fixed set in one fixed order: the result does not depend on
// how the columns were cut into groups, on col_tiles or on which workgroup ran first.
#include "common.hpp"
#include "pairs_device.hpp"
#include "switches.hpp"

namespace kge {

struct TopkArgs {
  int nfilt;                     // <= 2
  const unsigned int* bits[2];   // the filter bits of RankArgs (common.hpp): bit (j & 31) of word [i * rs + (j >> 5) * us]
  long long bits_rs, bits_us;
  int col_tiles;                 // column tiles a workgroup walks
  int k;                         // <= KGE_TOPK_MAX
  unsigned long long* part;      // [n][groups][k] keys, groups = gridDim.x
};

__device__ __forceinline__ unsigned long long topk_key(float s, unsigned int j) {
  if (s != s) s = -__builtin_inff();  // count_one's NaN rule (common.hpp)
  if (s == 0.0f) s = 0.0f;            // -0.0 -> +0.0
  const unsigned int u = __float_as_uint(s);
  const unsigned int hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)hi << 32) | (unsigned long long)(0xFFFFFFFFu - j);
}

extern __shared__ __attribute__((aligned(16))) unsigned long long topk_lists[];  // [k][64]: position-major, row fastest

template <int SCORER, typename T, int NORM, bool VEC, bool MFMA>
__global__ __launch_bounds__(256) void topk_select_kernel(Operand A, Operand R, Operand TG, int dir, int d, int dr,
                                                          long long n, long long m, float lp, int round_q, TopkArgs ta) {
  constexpr bool DOT = (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT);
  __shared__ __attribute__((aligned(16))) float QT[2][2][PT_KC][PT_LD];  // operands; then the finished tile [64][PT_LD]
  static_assert(sizeof(QT) >= PT_BM * PT_LD * 4, "the score tile fits the operand buffers");
  auto& Qs = QT[0];
  auto& Ts = QT[1];
  unsigned long long* const L = topk_lists;

  const int tid = threadIdx.x;
  const int K = ta.k;
  const int CT = ta.col_tiles;
  const long long row0 = (long long)blockIdx.y * PT_BM;
  for (int x = tid; x < K * PT_BM; x += 256) L[x] = 0ull;  // (the first tile's barriers come before the first insertion)
  // the list of row tid / 4 is owned by the lane with tid % 4 == 0: entries held and admission threshold (the list's
  // smallest key once it is full, else 0: every real key is above it)
  int cnt = 0;
  unsigned long long thr = 0ull;

  for (int ct = 0; ct < CT; ++ct) {
    const long long col0 = ((long long)blockIdx.x * CT + ct) * PT_BN;
    if (col0 >= m) break;
    if (ct > 0) __syncthreads();  // the previous tile's consumers are done with the operand buffers
    const int hh = (d + 1) / 2;   // coordinate pairs
    const int lim1 = d - hh;      // valid second-half elements
    const int nchunk = (hh + PT_KC - 1) / PT_KC;

    // staging role: row sr, coordinates 4 * scq .. + 3 of the chunk
    const int sr = tid >> 2, scq = tid & 3;
    long long qrow = row0 + sr;
    if (qrow >= n) qrow = n - 1;  // clamp: rows beyond n are computed but never listed
    long long trow = col0 + sr;
    if (trow >= m) trow = m - 1;
    const T* arow = (const T*)A.base + index_at(A.idx, qrow) * A.ld;
    const T* rrow = (const T*)R.base + index_at(R.idx, qrow) * R.ld;
    const T* tgrow = (const T*)TG.base + index_at(TG.idx, trow) * TG.ld;
    const int rl0 = (SCORER == KGE_ROTATE) ? dr : hh;  // valid relation first-half elements
    const int rl1 = (SCORER == KGE_ROTATE) ? 0 : lim1;

    f32x4 a0, a1, r0, r1, t0, t1;
    auto gload = [&](int ch) {
      const int c = ch * PT_KC + scq * 4;
      // chunk tail beyond the row (VEC: hh % 4 == 0): zeros.  (Written as one guarded block with plain assignments:
      // an early return from the lambda left two of the vectors in a private-memory slot.)
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 la0 = zero4, la1 = zero4, lr0 = zero4, lr1 = zero4, lt0 = zero4, lt1 = zero4;
      if (!(VEC && c >= hh)) {
        la0 = load4<T, VEC>(arow, c, hh);
        la1 = load4<T, VEC>(arow + hh, c, lim1);
        lr0 = load4<T, VEC>(rrow, c, rl0);
        if (SCORER != KGE_ROTATE) lr1 = load4<T, VEC>(rrow + hh, c, rl1);
        else lr1 = lr0;
        lt0 = load4<T, VEC>(tgrow, c, hh);
        lt1 = load4<T, VEC>(tgrow + hh, c, lim1);
      }
      a0 = la0; a1 = la1; r0 = lr0; r1 = lr1; t0 = lt0; t1 = lt1;
    };
    auto sstore = [&]() {
      f32x4 q0, q1;
      build_q4<SCORER>(dir, a0, a1, r0, r1, q0, q1);
      if (round_q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          q0[i] = round_bf16(q0[i]);
          q1[i] = round_bf16(q1[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Qs[0][scq * 4 + i][sr] = q0[i];
        Qs[1][scq * 4 + i][sr] = q1[i];
        Ts[0][scq * 4 + i][sr] = t0[i];
        Ts[1][scq * 4 + i][sr] = t1[i];
      }
    };

    const int lane = tid & 63, wave = tid >> 6;
    f32x16 macc;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 16; ++i) macc[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

    const int tx = tid & 15, ty = tid >> 4;
    const int mrow = 32 * (wave >> 1) + (lane & 31), mcol = 32 * (wave & 1) + (lane & 31);
    const int mh = lane >> 5;

    gload(0);
    sstore();
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
      if (ch + 1 < nchunk) gload(ch + 1);
      if (DOT && MFMA) {
#pragma unroll
        for (int cc = 0; cc < PT_KC; ++cc) {
          float av = Qs[mh][cc][mrow];
          float bv = Ts[mh][cc][mcol];
          macc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, macc, 0, 0, 0);
        }
      } else {
#pragma unroll 4
        for (int cc = 0; cc < PT_KC; ++cc) {
          f32x4 q0 = *reinterpret_cast<const f32x4*>(&Qs[0][cc][ty * 4]);
          f32x4 q1 = *reinterpret_cast<const f32x4*>(&Qs[1][cc][ty * 4]);
          f32x4 t0v = *reinterpret_cast<const f32x4*>(&Ts[0][cc][tx * 4]);
          f32x4 t1v = *reinterpret_cast<const f32x4*>(&Ts[1][cc][tx * 4]);
          if constexpr (!DOT) {
            dist_micro_tile<SCORER, NORM>(q0, q1, t0v, t1v, acc, lp);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                acc[i][j] = __builtin_fmaf(q0[i], t0v[j], acc[i][j]);
                acc[i][j] = __builtin_fmaf(q1[i], t1v[j], acc[i][j]);
              }
          }
        }
      }
      __syncthreads();
      if (ch + 1 < nchunk) sstore();
      __syncthreads();
    }

    // the finished tile through the operand buffers (the loop ended with a barrier)
    float* const tile = &QT[0][0][0][0];  // [64][PT_LD]
    if (DOT && MFMA) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        tile[(32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * mh) * PT_LD + 32 * (wave & 1) + (lane & 31)] = macc[r];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[i][j];
          if constexpr (!DOT) v = dist_score<NORM>(v, lp);
          tile[(ty * 4 + i) * PT_LD + tx * 4 + j] = v;
        }
    }
    __syncthreads();

    // scan: the four lanes of a row take 16 columns each and mark the unfiltered ones above the row's threshold
    const int row = tid >> 2, seg = tid & 3;
    const long long orow = row0 + row;
    const long long c0 = col0 + seg * 16;  // first column of the segment, relative to the scored slice
    const unsigned long long thr_row = __shfl(thr, lane & ~3, 64);
    unsigned int pass = 0u;
    if (orow < n && c0 < m) {
      unsigned int filt = 0u;
#pragma unroll
      for (int f = 0; f < 2; ++f)
        if (f < ta.nfilt) {
          const unsigned int w = ta.bits[f][orow * ta.bits_rs + (c0 >> 5) * ta.bits_us];
          filt |= (w >> (unsigned int)(c0 & 31)) & 0xFFFFu;
        }
      const float* src = tile + row * PT_LD + seg * 16;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c0 + c < m && !((filt >> c) & 1u) && topk_key(src[c], (unsigned int)(c0 + c)) > thr_row) pass |= 1u << c;
    }
    unsigned long long cand = (unsigned long long)pass << (16 * seg);
    cand |= __shfl_xor(cand, 1, 64);
    cand |= __shfl_xor(cand, 2, 64);
    // insert: one lane per row, ascending column; the threshold rises as the list fills
    if (seg == 0) {
      while (cand) {
        const int c = __builtin_ctzll(cand);
        cand &= cand - 1;
        const unsigned long long key = topk_key(tile[row * PT_LD + c], (unsigned int)(col0 + c));
        if (key <= thr) continue;
        int p = cnt < K ? cnt : K - 1;  // the slot that opens (a full list drops its last entry)
        while (p > 0) {
          const unsigned long long prev = L[(p - 1) * PT_BM + row];
          if (prev > key) break;
          L[p * PT_BM + row] = prev;
          --p;
        }
        L[p * PT_BM + row] = key;
        if (cnt < K) ++cnt;
        thr = cnt == K ? L[(K - 1) * PT_BM + row] : 0ull;
      }
    }
  }  // column tiles

  __syncthreads();
  const long long groups = gridDim.x;
  for (int x = tid; x < K * PT_BM; x += 256) {
    const int row = x / K, p = x - row * K;
    const long long orow = row0 + row;
    if (orow < n) ta.part[(orow * groups + blockIdx.x) * K + p] = L[p * PT_BM + row];
  }
}

// One wave per row: lane l owns the lists l, l + 64, ... and keeps the largest of their heads; per output position the
// wave takes the largest of the lanes' keys, and the lane that held it moves that list's head on.
constexpr int TOPK_MAX_GROUPS = 512;

__global__ __launch_bounds__(256) void topk_merge_kernel(const unsigned long long* __restrict__ part, int groups, int k,
                                                         long long n, long long col_begin, float* __restrict__ out_val,
                                                         long long* __restrict__ out_idx, long long ld) {
  __shared__ int head[4][TOPK_MAX_GROUPS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= n) return;  // (whole waves; no workgroup barrier below)
  int* const hd = head[wave];
  const unsigned long long* const lists = part + i * (long long)groups * k;
  for (int g = lane; g < groups; g += 64) hd[g] = 0;
  unsigned long long best = 0ull;
  for (int g = lane; g < groups; g += 64) {
    const unsigned long long v = lists[(long long)g * k];
    best = v > best ? v : best;
  }
  for (int r = 0; r < k; ++r) {
    unsigned long long top = best;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = __shfl_xor(top, off, 64);
      top = o > top ? o : top;
    }
    if (lane == 0) {
      float v = -__builtin_inff();
      long long id = -1;
      if (top != 0ull) {
        const unsigned int hi = (unsigned int)(top >> 32);
        v = __uint_as_float((hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi);
        id = col_begin + (long long)(0xFFFFFFFFu - (unsigned int)top);
      }
      out_val[i * ld + r] = v;
      out_idx[i * ld + r] = id;
    }
    if (top != 0ull && best == top) {  // (keys are distinct: exactly one lane)
      best = 0ull;
      for (int g = lane; g < groups; g += 64) {
        int h = hd[g];
        unsigned long long v = h < k ? lists[(long long)g * k + h] : 0ull;
        if (v == top) {
          hd[g] = ++h;
          v = h < k ? lists[(long long)g * k + h] : 0ull;
        }
        best = v > best ? v : best;
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------
static inline bool topk_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// (the conditions of score_pairs.hip's vector loads)
static bool topk_vec_ok(int dtype, int d, int dr, int scorer, const Operand& A, const Operand& R, const Operand& TG) {
  if (d % 8) return false;
  if (scorer == KGE_ROTATE && dr != d / 2) return false;
  const int es = dtype == KGE_BF16 ? 2 : 4;
  const int al = dtype == KGE_BF16 ? 8 : 16;
  if (!topk_aligned16(A.base) || !topk_aligned16(R.base) || !topk_aligned16(TG.base)) return false;
  if ((A.ld * es) % al || (R.ld * es) % al || (TG.ld * es) % al) return false;
  return true;
}

// column tiles per workgroup and column groups of a launch: enough groups that the row blocks x groups fill the CUs
// twice over, at least four tiles per workgroup where there are that many (the lists fill during the first tiles: the
// more tiles follow, the less that costs), at most TOPK_MAX_GROUPS groups (topk_merge_kernel's head table).
// SW_TOPK_COL_TILES overrides the tiles per workgroup (tests).
long long topk_groups(long long n, long long m, int* col_tiles) {
  const long long tiles = (m + PT_BN - 1) / PT_BN, row_blocks = (n + PT_BM - 1) / PT_BM;
  if (tiles <= 0 || row_blocks <= 0) {
    if (col_tiles) *col_tiles = 1;
    return 0;
  }
  long long want = 512 / row_blocks;
  if (want < 1) want = 1;
  long long ctn = (tiles + want - 1) / want;
  if (ctn < 4) ctn = tiles < 4 ? tiles : 4;
  const long long forced = sw(SW_TOPK_COL_TILES);
  if (forced > 0) ctn = forced;
  const long long least = (tiles + TOPK_MAX_GROUPS - 1) / TOPK_MAX_GROUPS;
  if (ctn < least) ctn = least;
  if (ctn > (1LL << 30)) ctn = 1LL << 30;
  if (col_tiles) *col_tiles = (int)ctn;
  return (tiles + ctn - 1) / ctn;
}

template <int SCORER, typename T, int NORM, bool VEC, bool MFMA>
static int launch_topk(const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr, long long n,
                       long long m, float lp, int round_q, const TopkArgs& ta, long long groups, hipStream_t st) {
  auto kern = topk_select_kernel<SCORER, T, NORM, VEC, MFMA>;
  const size_t lds = (size_t)ta.k * PT_BM * sizeof(unsigned long long);
  if (lds > 32 * 1024) {  // (more dynamic LDS than a launch gets without asking)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            KGE_TOPK_MAX * PT_BM * (int)sizeof(unsigned long long)) != hipSuccess) {
      (void)hipGetLastError();
      return KGE_ERR_LAUNCH;
    }
  }
  const dim3 grid((unsigned)groups, (unsigned)((n + PT_BM - 1) / PT_BM));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, A, R, TG, dir, d, dr, n, m, lp, round_q, ta);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, typename T>
static int topk_norm(int norm, bool vec, bool mfma, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                     int dr, long long n, long long m, float lp, int round_q, const TopkArgs& ta, long long groups,
                     hipStream_t st) {
#define KGE_TK(NM, MF)                                                                                         \
  (vec ? launch_topk<SCORER, T, NM, true, MF>(A, R, TG, dir, d, dr, n, m, lp, round_q, ta, groups, st)         \
       : launch_topk<SCORER, T, NM, false, MF>(A, R, TG, dir, d, dr, n, m, lp, round_q, ta, groups, st))
  if constexpr (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT) {
    return mfma ? KGE_TK(NORM_L1, true) : KGE_TK(NORM_L1, false);
  } else {
    if (norm == NORM_L1) return KGE_TK(NORM_L1, false);
    if (norm == NORM_L2) return KGE_TK(NORM_L2, false);
    return KGE_TK(NORM_LP, false);
  }
#undef KGE_TK
}

// The k best unfiltered columns of every row: `part` receives the groups' lists ([n][groups][k] keys), out_val /
// out_idx the merged result (row pitch ld; -inf / -1 where a row has fewer than k unfiltered columns).  bits: NULL
// entries beyond nfilt.  m == 0: padding only.
int run_topk(int scorer, int dtype, bool use_mfma, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
             int dr, long long n, long long m, float lp, int k, int nfilt, const unsigned int* const* bits,
             long long bits_rs, long long bits_us, unsigned long long* part, long long col_begin, float* out_val,
             long long* out_idx, long long ld, hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (n > 65535LL * PT_BM) return KGE_ERR_UNSUPPORTED;
  int col_tiles = 1;
  const long long groups = topk_groups(n, m, &col_tiles);
  int rc = KGE_OK;
  if (groups > 0) {
    const bool dot = scorer == KGE_COMPLEX || scorer == KGE_DISTMULT;
    const bool vec = topk_vec_ok(dtype, d, dr, scorer, A, R, TG);
    const int norm = norm_mode(lp);
    const int round_q = (dtype == KGE_BF16 && dot) ? 1 : 0;  // the single-pass semantics of bf16 tables (KGE_FLAG_EXACT)
    TopkArgs ta{};
    ta.nfilt = nfilt;
    for (int f = 0; f < nfilt; ++f) ta.bits[f] = bits[f];
    ta.bits_rs = bits_rs;
    ta.bits_us = bits_us;
    ta.col_tiles = col_tiles;
    ta.k = k;
    ta.part = part;
#define KGE_DT(SC)                                                                                                     \
  rc = dtype == KGE_BF16                                                                                               \
           ? topk_norm<SC, unsigned short>(norm, vec, use_mfma, A, R, TG, dir, d, dr, n, m, lp, round_q, ta, groups, st) \
           : topk_norm<SC, float>(norm, vec, use_mfma, A, R, TG, dir, d, dr, n, m, lp, round_q, ta, groups, st);       \
  break
    switch (scorer) {
      case KGE_COMPLEX: KGE_DT(KGE_COMPLEX);
      case KGE_DISTMULT: KGE_DT(KGE_DISTMULT);
      case KGE_TRANSE: KGE_DT(KGE_TRANSE);
      case KGE_ROTATE: KGE_DT(KGE_ROTATE);
      default: rc = KGE_ERR_INVALID_ARG;
    }
#undef KGE_DT
    if (rc != KGE_OK) return rc;
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, part, (int)groups, k, n,
                     col_begin, out_val, out_idx, ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
