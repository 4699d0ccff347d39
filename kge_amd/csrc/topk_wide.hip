// topk_wide.hip -- the wide pair of kge_topk, gfx950: 1 <= k <= 1024.  Same result contract as topk.hip:
// every score has the bits kge_score_sp / kge_score_po store, the order is descending canonical score then ascending id,
// padding is (-inf, -1), the result is a pure function of the arguments.
//
//   topk_select_wide_kernel  the 64 x 64 tile walk and canonical chain of topk_select_kernel; the selection is new.
//                            The sorted list of a (row, column group) lives in the WORKSPACE (two halves of k keys,
//                            L2-resident); LDS holds, per row, 128 pending keys.  The four lanes of a row append the
//                            survivors of a tile (key > the row's threshold) at positions from a shuffle prefix.  A
//                            row whose buffer could overflow on the next tile is flushed by its wave (wave w owns the
//                            rows 16 w .. 16 w + 15, the rows its own lanes scan, so no flush waits for another wave):
//                            the wave sorts the pending keys in registers (two per lane, bitonic network over
//                            __shfl_xor), stages the list in LDS with one coalesced read, and writes the merged list
//                            into the other half BY RANK -- a pending key lands at its own rank plus the number of list
//                            keys above it, a list key at its position plus the number of pending keys above it (two
//                            binary searches in LDS) -- dropping everything past k.  An empty list is the same merge
//                            with a list of length 0: there is no separate fill phase and no sort of k keys.
//   topk_merge_wide_kernel   one workgroup per row folds the groups' lists into an LDS buffer of kp = 2^ceil(log2 k)
//                            keys: max(A[i], B[kp - 1 - i]) is a bitonic sequence holding the kp best of the union,
//                            log2(kp) compare-exchange stages re-sort it.
//
// Every loop is bounded by k, 128, the group count or the tile count; no workgroup waits for another, no atomics.
#include "topk_device.hpp"

namespace kge {

constexpr int TW_PEND = 128;     // pending keys of a row
constexpr int TW_PEND_LD = 130;  // their pitch in keys: rows 4 banks apart (appends of 16 rows hit different banks)
constexpr int TW_FLUSH_AT = 64;  // a row with more pending keys than this is flushed: the next tile adds up to 64
static_assert(TW_PEND == 2 * 64, "tw_sort128: two keys per lane");
static_assert(TW_FLUSH_AT + PT_BN <= TW_PEND && TW_PEND <= TW_PEND_LD, "a tile's survivors fit behind an unflushed buffer");

struct TopkWideArgs {
  TopkArgs t;  // part: [n][groups][2][k]
  int* fin;    // [n][groups]: (entries of the final list << 1) | the half that holds it
};

// Lanes of one wave hand data to each other through LDS / the workspace: order the accesses around the hand-over.
__device__ __forceinline__ void tw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// how many of the descending keys arr[0 .. len) are above x (len <= 1024: at most 11 halvings)
__device__ __forceinline__ int tw_count_above(const unsigned long long* arr, int len, unsigned long long x) {
  int lo = 0, hi = len;
  for (int s = 0; s < 11 && lo < hi; ++s) {
    const int mid = (lo + hi) >> 1;
    if (arr[mid] > x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void tw_cx(unsigned long long& v, int stride, bool keep_max) {
  const unsigned long long o = __shfl_xor(v, stride, 64);
  v = ((o > v) == keep_max) ? o : v;
}

// 128 keys, element e = lane in a, e = lane + 64 in b: descending bitonic sort across the wave
__device__ __forceinline__ void tw_sort128(unsigned long long& a, unsigned long long& b, int lane) {
#pragma unroll
  for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride == 64) {  // (size == 128: one descending run, partners in the same lane)
        const unsigned long long hi = a > b ? a : b, lo = a > b ? b : a;
        a = hi;
        b = lo;
      } else {
        const bool lower = (lane & stride) == 0;
        tw_cx(a, stride, ((lane & size) == 0) == lower);
        tw_cx(b, stride, (((lane + 64) & size) == 0) == lower);
      }
    }
  }
}

extern __shared__ __attribute__((aligned(16))) unsigned long long tw_lds[];  // pending [64][TW_PEND_LD]; stage [4][kw]

// One finished 64 x 64 tile of canonical scores in `QT` ([64][PT_LD] floats): topk_select_kernel's scoring, restated.
// Ends with a workgroup barrier.
template <int SCORER, typename T, int NORM, bool VEC, bool MFMA>
__device__ __forceinline__ void tw_score_tile(float (&QT)[2][2][PT_KC][PT_LD], const Operand& A, const Operand& R,
                                              const Operand& TG, int dir, int d, int dr, long long n, long long m,
                                              float lp, int round_q, long long row0, long long col0) {
  constexpr bool DOT = (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT);
  auto& Qs = QT[0];
  auto& Ts = QT[1];
  const int tid = threadIdx.x;
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
    // chunk tail beyond the row (VEC: hh % 4 == 0): zeros (one guarded block with plain assignments, as in topk.hip)
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
}

template <int SCORER, typename T, int NORM, bool VEC, bool MFMA>
__global__ __launch_bounds__(256) void topk_select_wide_kernel(Operand A, Operand R, Operand TG, int dir, int d, int dr,
                                                               long long n, long long m, float lp, int round_q,
                                                               TopkWideArgs wa, int kw) {
  __shared__ __attribute__((aligned(16))) float QT[2][2][PT_KC][PT_LD];  // operands; then the finished tile [64][PT_LD]
  static_assert(sizeof(QT) >= PT_BM * PT_LD * 4, "the score tile fits the operand buffers");
  __shared__ unsigned long long last_key[4];  // per wave: the key a flush wrote at position k - 1

  const TopkArgs& ta = wa.t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = ta.k;
  const int CT = ta.col_tiles;
  const long long row0 = (long long)blockIdx.y * PT_BM;
  const long long groups = gridDim.x;
  const float* const tile = &QT[0][0][0][0];

  // scan role: the four lanes of row tid / 4 take 16 columns each.  A row's state is held, equal, by its four lanes.
  const int row = tid >> 2, seg = tid & 3;
  const long long orow = row0 + row;
  unsigned long long* const pend = tw_lds + row * TW_PEND_LD;
  int pc = 0;                    // pending keys
  int lc = 0;                    // entries of the list
  int half = 0;                  // the half of the pair that holds it
  unsigned long long thr = 0ull; // admission threshold: the list's last key once it is full, else 0 (below every real key)
  // flush role: the wave's stage for one list, kw = k rounded up to 64 keys
  unsigned long long* const stage = tw_lds + PT_BM * TW_PEND_LD + wave * kw;

  for (int ct = 0; ct < CT; ++ct) {
    const long long col0 = ((long long)blockIdx.x * CT + ct) * PT_BN;
    if (col0 >= m) break;
    if (ct > 0) __syncthreads();  // the previous tile's scans are done with the operand buffers
    tw_score_tile<SCORER, T, NORM, VEC, MFMA>(QT, A, R, TG, dir, d, dr, n, m, lp, round_q, row0, col0);

    // scan: mark the unfiltered columns above the row's threshold
    const long long c0 = col0 + seg * 16;  // first column of the segment, relative to the scored slice
    const float* src = tile + row * PT_LD + seg * 16;
    unsigned int pass = 0u;
    if (orow < n && c0 < m) {
      unsigned int filt = 0u;
#pragma unroll
      for (int f = 0; f < 2; ++f)
        if (f < ta.nfilt) {
          const unsigned int w = ta.bits[f][orow * ta.bits_rs + (c0 >> 5) * ta.bits_us];
          filt |= (w >> (unsigned int)(c0 & 31)) & 0xFFFFu;
        }
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c0 + c < m && !((filt >> c) & 1u) && topk_key(src[c], (unsigned int)(c0 + c)) > thr) pass |= 1u << c;
    }
    // append in ascending column order: positions from a prefix over the four lanes' counts
    const int mine = __builtin_popcount(pass);
    const int q0 = __shfl(mine, (lane & ~3) + 0, 64), q1 = __shfl(mine, (lane & ~3) + 1, 64),
              q2 = __shfl(mine, (lane & ~3) + 2, 64), q3 = __shfl(mine, (lane & ~3) + 3, 64);
    int at = pc + (seg > 0 ? q0 : 0) + (seg > 1 ? q1 : 0) + (seg > 2 ? q2 : 0);  // <= 64 + 48, + mine <= 128
    while (pass) {
      const int c = __builtin_ctz(pass);
      pass &= pass - 1;
      pend[at++] = topk_key(src[c], (unsigned int)(c0 + c));
    }
    pc += q0 + q1 + q2 + q3;
    tw_wave_sync();

    // flush: rows that could overflow on the next tile; after the last tile, every row with pending keys
    const bool last = ct + 1 == CT || col0 + PT_BN >= m;
    unsigned long long todo = __ballot(seg == 0 && (last ? pc > 0 : pc > TW_FLUSH_AT));
    while (todo) {  // (wave-uniform; at most 16 rows)
      const int src_lane = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int fr = 16 * wave + (src_lane >> 2);  // the row being flushed
      const int fpc = __shfl(pc, src_lane, 64), flc = __shfl(lc, src_lane, 64), fhalf = __shfl(half, src_lane, 64);
      unsigned long long* const fp = tw_lds + fr * TW_PEND_LD;
      unsigned long long* const pair = ta.part + (((row0 + fr) * groups + blockIdx.x) * 2) * K;
      const unsigned long long* const from = pair + (long long)fhalf * K;
      unsigned long long* const to = pair + (long long)(fhalf ^ 1) * K;

      for (int i = lane; i < flc; i += 64) stage[i] = from[i];  // (flc <= k <= kw)
      unsigned long long ka = lane < fpc ? fp[lane] : 0ull;
      unsigned long long kb = lane + 64 < fpc ? fp[lane + 64] : 0ull;
      tw_sort128(ka, kb, lane);  // (the zeros sort behind every real key)
      fp[lane] = ka;
      fp[lane + 64] = kb;
      tw_wave_sync();

      if (lane < fpc) {
        const int pos = lane + tw_count_above(stage, flc, ka);
        if (pos < K) to[pos] = ka;
        if (pos == K - 1) last_key[wave] = ka;
      }
      if (lane + 64 < fpc) {
        const int pos = lane + 64 + tw_count_above(stage, flc, kb);
        if (pos < K) to[pos] = kb;
        if (pos == K - 1) last_key[wave] = kb;
      }
      for (int i = lane; i < flc; i += 64) {
        const unsigned long long y = stage[i];
        const int pos = i + tw_count_above(fp, fpc, y);
        if (pos < K) to[pos] = y;
        if (pos == K - 1) last_key[wave] = y;
      }
      tw_wave_sync();
      // (the positions are a bijection onto 0 .. flc + fpc - 1: position k - 1 was written iff the list is full now)
      const int nlc = flc + fpc < K ? flc + fpc : K;
      const unsigned long long nthr = nlc == K ? last_key[wave] : 0ull;
      if ((lane >> 2) == (src_lane >> 2)) {
        pc = 0;
        lc = nlc;
        half ^= 1;
        thr = nthr;
      }
      tw_wave_sync();  // the stage, the row's buffer and last_key are free for the next flush
    }
  }  // column tiles

  if (seg == 0 && orow < n) wa.fin[orow * groups + blockIdx.x] = (lc << 1) | half;
}

// One workgroup per row.  LDS: best[kp] (descending, zero-padded) and one group's list in[kp].
__global__ __launch_bounds__(256) void topk_merge_wide_kernel(const unsigned long long* __restrict__ part,
                                                              const int* __restrict__ fin, int groups, int k, int kp,
                                                              long long col_begin, float* __restrict__ out_val,
                                                              long long* __restrict__ out_idx, long long ld) {
  unsigned long long* const best = tw_lds;
  unsigned long long* const in = tw_lds + kp;
  const int tid = threadIdx.x;
  const long long i = blockIdx.x;
  for (int x = tid; x < kp; x += 256) best[x] = 0ull;
  for (int g = 0; g < groups; ++g) {
    const int f = fin[i * groups + g];  // (the same word for the whole workgroup)
    const int len = f >> 1;
    if (len == 0) continue;
    const unsigned long long* const list = part + ((i * groups + g) * 2 + (f & 1)) * (long long)k;
    __syncthreads();  // the previous fold's last stage
    for (int x = tid; x < kp; x += 256) in[x] = x < len ? list[x] : 0ull;
    __syncthreads();
    for (int x = tid; x < kp; x += 256) {
      const unsigned long long a = best[x], b = in[kp - 1 - x];
      best[x] = a > b ? a : b;
    }
    for (int stride = kp >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int q = tid; q < (kp >> 1); q += 256) {
        const int lo = ((q & ~(stride - 1)) << 1) | (q & (stride - 1)), hi = lo + stride;
        const unsigned long long a = best[lo], b = best[hi];
        if (a < b) {
          best[lo] = b;
          best[hi] = a;
        }
      }
    }
  }
  __syncthreads();
  for (int r = tid; r < k; r += 256) {
    float v;
    long long id;
    topk_unpack(best[r], col_begin, v, id);
    out_val[i * ld + r] = v;
    out_idx[i * ld + r] = id;
  }
}

// ---- host ---------------------------------------------------------------------------------
// topk_groups with one more floor: a group sees about 4 k columns where m allows, so that its lists fill and the
// threshold starts to reject (an admitted key costs a share of a flush; a rejected one a comparison).
long long topk_wide_groups(long long n, long long m, int k, int* col_tiles) {
  const long long tiles = (m + PT_BN - 1) / PT_BN, row_blocks = (n + PT_BM - 1) / PT_BM;
  if (tiles <= 0 || row_blocks <= 0) {
    if (col_tiles) *col_tiles = 1;
    return 0;
  }
  long long want = 512 / row_blocks;
  if (want < 1) want = 1;
  long long ctn = (tiles + want - 1) / want;
  long long floor_tiles = (4LL * k + PT_BN - 1) / PT_BN;
  if (floor_tiles < 4) floor_tiles = 4;
  if (ctn < floor_tiles) ctn = tiles < floor_tiles ? tiles : floor_tiles;
  const long long forced = sw(SW_TOPK_COL_TILES);
  if (forced > 0) ctn = forced;
  const long long least = (tiles + TOPK_MAX_GROUPS - 1) / TOPK_MAX_GROUPS;
  if (ctn < least) ctn = least;
  if (ctn > (1LL << 30)) ctn = 1LL << 30;
  if (col_tiles) *col_tiles = (int)ctn;
  return (tiles + ctn - 1) / ctn;
}

// [n][groups][2][k] keys, then [n][groups] list states
long long topk_wide_part_bytes(long long n, long long m, int k) {
  const long long groups = topk_wide_groups(n, m, k, nullptr);
  return n * groups * 2 * (long long)k * 8 + n * groups * 4;
}

static inline int tw_stage_keys(int k) { return (k + 63) / 64 * 64; }
static inline size_t tw_select_lds(int k) {
  return ((size_t)PT_BM * TW_PEND_LD + 4 * (size_t)tw_stage_keys(k)) * sizeof(unsigned long long);
}

template <int SCORER, typename T, int NORM, bool VEC, bool MFMA>
static int launch_topk_wide(const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr, long long n,
                            long long m, float lp, int round_q, const TopkWideArgs& wa, long long groups,
                            hipStream_t st) {
  auto kern = topk_select_wide_kernel<SCORER, T, NORM, VEC, MFMA>;
  // (more dynamic LDS than a launch gets without asking: 65 KB of pending keys + up to 32 KB of stages)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)tw_select_lds(KGE_TOPK_MAX)) != hipSuccess) {
    (void)hipGetLastError();
    return KGE_ERR_LAUNCH;
  }
  const dim3 grid((unsigned)groups, (unsigned)((n + PT_BM - 1) / PT_BM));
  hipLaunchKernelGGL(kern, grid, dim3(256), tw_select_lds(wa.t.k), st, A, R, TG, dir, d, dr, n, m, lp, round_q, wa,
                     tw_stage_keys(wa.t.k));
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, typename T>
static int topk_wide_norm(int norm, bool vec, bool mfma, const Operand& A, const Operand& R, const Operand& TG, int dir,
                          int d, int dr, long long n, long long m, float lp, int round_q, const TopkWideArgs& wa,
                          long long groups, hipStream_t st) {
#define KGE_TW(NM, MF)                                                                                          \
  (vec ? launch_topk_wide<SCORER, T, NM, true, MF>(A, R, TG, dir, d, dr, n, m, lp, round_q, wa, groups, st)     \
       : launch_topk_wide<SCORER, T, NM, false, MF>(A, R, TG, dir, d, dr, n, m, lp, round_q, wa, groups, st))
  if constexpr (SCORER == KGE_COMPLEX || SCORER == KGE_DISTMULT) {
    return mfma ? KGE_TW(NORM_L1, true) : KGE_TW(NORM_L1, false);
  } else {
    if (norm == NORM_L1) return KGE_TW(NORM_L1, false);
    if (norm == NORM_L2) return KGE_TW(NORM_L2, false);
    return KGE_TW(NORM_LP, false);
  }
#undef KGE_TW
}

// run_topk's contract (topk.hip) on the wide pair; `part` has topk_wide_part_bytes(n, m, k) bytes.
int run_topk_wide(int scorer, int dtype, bool use_mfma, const Operand& A, const Operand& R, const Operand& TG, int dir,
                  int d, int dr, long long n, long long m, float lp, int k, int nfilt, const unsigned int* const* bits,
                  long long bits_rs, long long bits_us, unsigned long long* part, long long col_begin, float* out_val,
                  long long* out_idx, long long ld, hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (n > 65535LL * PT_BM) return KGE_ERR_UNSUPPORTED;
  int col_tiles = 1;
  const long long groups = topk_wide_groups(n, m, k, &col_tiles);
  int* const fin = (int*)(part + n * groups * 2 * (long long)k);
  int rc = KGE_OK;
  if (groups > 0) {
    const bool dot = scorer == KGE_COMPLEX || scorer == KGE_DISTMULT;
    const bool vec = topk_vec_ok(dtype, d, dr, scorer, A, R, TG);
    const int norm = norm_mode(lp);
    const int round_q = (dtype == KGE_BF16 && dot) ? 1 : 0;  // the single-pass semantics of bf16 tables (KGE_FLAG_EXACT)
    TopkWideArgs wa{};
    wa.t.nfilt = nfilt;
    for (int f = 0; f < nfilt; ++f) wa.t.bits[f] = bits[f];
    wa.t.bits_rs = bits_rs;
    wa.t.bits_us = bits_us;
    wa.t.col_tiles = col_tiles;
    wa.t.k = k;
    wa.t.part = part;
    wa.fin = fin;
#define KGE_DT(SC)                                                                                                   \
  rc = dtype == KGE_BF16 ? topk_wide_norm<SC, unsigned short>(norm, vec, use_mfma, A, R, TG, dir, d, dr, n, m, lp,   \
                                                              round_q, wa, groups, st)                               \
                         : topk_wide_norm<SC, float>(norm, vec, use_mfma, A, R, TG, dir, d, dr, n, m, lp, round_q,   \
                                                     wa, groups, st);                                                \
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
  int kp = 2;
  while (kp < k) kp <<= 1;
  hipLaunchKernelGGL(topk_merge_wide_kernel, dim3((unsigned)n), dim3(256), 2 * (size_t)kp * sizeof(unsigned long long),
                     st, part, fin, (int)groups, k, kp, col_begin, out_val, out_idx, ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
