// score_neg_shared.hip -- negative sampling with SHARED samples (negative_sampling.shared: true), gfx950.
//
// NaiveSharedNegativeSample.score / DefaultSharedNegativeSample.score (kge/util/sampler.py:428-463, 537-578): all
// n positives of a batch are scored against the same U distinct entities; the [n, K] block the job gets is defined
// by (unique, drop, repeat):
//   column c < Uc        positive i with its slot replaced by unique[c] -- by unique[Uc] (the spare) if drop[i] == c
//   column Uc + r        column repeat[r] of the same row
// which is samples(indexes) scored per triple (the "triple" implementation that TransE / RotatE are forced to,
// transe.py:58-68, gathers n K rows for it: only U <= K distinct ones exist).
//
// Forward (neg_shared_kernel): a workgroup owns SNS_TN positives x SNS_TU output columns.  The columns' target rows
// (and the spare) are staged ONCE in LDS and read from there by every positive of the tile; a group of G lanes owns
// one positive at a time, its fixed side in registers (load_fixed, as in neg_kernel of score_spo.hip), and walks
// the staged rows.  Lane-to-coordinate layout, per-chunk arithmetic, the xor butterfly and finalize are the ones
// of score_spo.hip (spo_device.hpp): the scores are bit-identical to kge_score_neg on the materialised samples.
// Drop and repeat are resolved while staging / reading: a repeat column stages the row of the column it repeats
// (every output element is written exactly once, by the group that computed it; no search through the repeat list),
// a positive whose drop index names the column reads the spare's slot instead.
//
// Backward (kge_score_neg_shared_bwd_accum): gout is folded over the repeat columns and the drop rule into one weight
// per (positive, physical row) (sns_fold_*), then two passes of neg_shared_bwd_kernel over the [n, U(+1)] pairs:
//   ROLE 0  a wave owns a positive: its relation row and fixed entity row in registers, their gradients summed in
//           registers over a tile of physical rows staged in LDS, one atomic flush per (positive, tile);
//   ROLE 1  a wave owns a physical row: its gradient summed in registers over a tile of positives (their two rows
//           staged in LDS), one atomic flush per (row, tile).
// Tiles are 64 / NC physical rows (ROLE 0) and 32 / NC positives (ROLE 1), NC = 1, 2, 4, 8 coordinate pairs per lane
// for ceil(d / 2) <= 64, 128, 256, 512: the staged rows fill at most SNB_SM = 8192 floats.
// No atomic per (positive, sample) occurrence: ~NC (n U / 64 + U n / 32) row flushes instead of n K.
#include "bwd_device.hpp"
#include "spo_device.hpp"

namespace kge {

constexpr int SNS_TN = 32;  // positives per workgroup
constexpr int SNS_TU = 32;  // output columns (staged target rows) per workgroup; slot SNS_TU holds the spare
constexpr long long SNS_LDS_MAX = 160 * 1024;

// one lane's chunk ci of a staged half-row (vector path).  f32 rows are staged with the two 16-byte halves of every
// chunk apart ([all low halves][all high halves]): lane g reads 16 g and D/2 * 4 + 16 g -- 16 consecutive lanes cover
// 256 consecutive bytes per ds_read_b128 instead of every other 16 (a 2-way bank conflict).  bf16 chunks are 16
// bytes: staged as they are.
__device__ __forceinline__ f32x8 lds_chunk(const float* half_row, int ci, int D) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(half_row + 4 * ci);
  const f32x4 b = *reinterpret_cast<const f32x4*>(half_row + (D >> 1) + 4 * ci);
  f32x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.v[i] = a[i];
    r.v[4 + i] = b[i];
  }
  return r;
}
__device__ __forceinline__ f32x8 lds_chunk(const unsigned short* half_row, int ci, int D) {
  return ld8<unsigned short>(half_row + 8 * ci);
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256) void neg_shared_kernel(Operand S, Operand R, Operand O, int d, int dr, long long n,
                                                         int slot, Index uniq, long long Uc,
                                                         const long long* __restrict__ drop,
                                                         const long long* __restrict__ rep, long long K, float lp,
                                                         float* __restrict__ out, long long ldo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sns_smem[];
  constexpr bool CPLX = IsComplex<SCORER>::value;
  constexpr int GPB = 256 / G;               // groups per workgroup
  constexpr int JG = G < SNS_TU ? G : SNS_TU;  // columns whose scores one round of a group's lanes keeps
  constexpr int NM = SNS_TU / JG;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int lg = lane & (G - 1);
  const int gid = (tid >> 6) * (64 / G) + lane / G;
  const int h = d / 2;
  const int D = CPLX ? h : d;
  const int nchunks = (D + 7) / 8;
  const int pitch = (d + 7) & ~7;  // elements; rows start 16-byte aligned
  T* rows = reinterpret_cast<T*>(sns_smem);
  long long* rowid = reinterpret_cast<long long*>(sns_smem + (size_t)(SNS_TU + 1) * pitch * sizeof(T));
  long long* srccol = rowid + (SNS_TU + 1);
  const long long k0 = (long long)blockIdx.x * SNS_TU;
  const int ncol = (int)(K - k0 < SNS_TU ? K - k0 : SNS_TU);
  const long long i0 = (long long)blockIdx.y * SNS_TN;
  const T* ent = (const T*)S.base;  // S.base == O.base == entity table

  // 1. which table row every slot of the tile holds, and the column of the unique list it stands for
  if (tid <= SNS_TU) {
    long long c = -1, id = -1;
    if (tid < ncol) {
      const long long k = k0 + tid;
      c = k < Uc ? k : rep[k - Uc];
      id = index_at(uniq, c);
    } else if (tid == SNS_TU && drop) {
      c = Uc;
      id = index_at(uniq, Uc);
    }
    rowid[tid] = id;
    srccol[tid] = c;
  }
  __syncthreads();

  // 2. stage the rows: every target row is fetched once per workgroup
  const int nslots = ncol + (drop ? 1 : 0);
  if (VEC) {
    const int ppr = (int)(d * sizeof(T) / 16);  // 16-byte pieces per row
    for (int idx = tid; idx < nslots * ppr; idx += 256) {
      const int js = idx / ppr, q = idx - js * ppr;
      const int j = js < ncol ? js : SNS_TU;
      const u32x4 v = *(reinterpret_cast<const u32x4*>(ent + rowid[j] * S.ld) + q);
      int dst;  // in elements
      if (sizeof(T) == 4) {
        const int e = 4 * q;
        const int hs = (CPLX && e >= D) ? 1 : 0;
        const int w = e - hs * D;
        dst = hs * D + ((w >> 2) & 1) * (D >> 1) + 4 * (w >> 3);
      } else {
        dst = 8 * q;
      }
      *reinterpret_cast<u32x4*>(rows + (size_t)j * pitch + dst) = v;
    }
  } else {
    for (int idx = tid; idx < nslots * d; idx += 256) {
      const int js = idx / d, e = idx - js * d;
      const int j = js < ncol ? js : SNS_TU;
      rows[(size_t)j * pitch + e] = ent[rowid[j] * S.ld + e];
    }
  }
  __syncthreads();

  // 3. every group walks the staged rows for one positive at a time
  auto sweep = [&](auto slot_c) {
    constexpr int SLOT = decltype(slot_c)::value;
    const int c00 = lg * 8;
    const int cnt0 = (D - c00 < 8) ? (D - c00) : 8;
    const bool act = lg < nchunks;
    for (int pp = gid; pp < SNS_TN; pp += GPB) {
      const long long i = i0 + pp;
      if (i >= n) continue;  // (a whole group: the butterfly stays inside it)
      const T* fixrow = ent + index_at(SLOT == 0 ? O.idx : S.idx, i) * S.ld;
      const T* rrow = (const T*)R.base + index_at(R.idx, i) * R.ld;
      const long long dri = drop ? drop[i] : -1;
      Fixed F0;
      if (act) F0 = load_fixed<SCORER, T, VEC>(SLOT, fixrow, rrow, c00, D, h);
      float res[NM];
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        res[m] = 0.0f;
        for (int jj = 0; jj < JG; ++jj) {
          const int j = m * JG + jj;
          if (j >= ncol) break;
          const T* xr = rows + (size_t)(srccol[j] == dri ? SNS_TU : j) * pitch;
          float P = 0.0f;
          if (act) {
            f32x8 x0, x1;
            if (VEC) {
              x0 = lds_chunk(xr, lg, D);
              x1 = x0;
              if (CPLX) x1 = lds_chunk(xr + h, lg, D);
            } else {
              x0 = load_chunk<T, false>(xr, c00, D);
              x1 = x0;
              if (CPLX) x1 = load_chunk<T, false>(xr + h, c00, D);
            }
            P = apply_chunk<SCORER, NORM>(SLOT, P, F0, x0, x1, VEC ? 8 : cnt0, lp);
          }
          for (int ci = lg + 64; ci < nchunks; ci += 64) {  // only when D > 512
            const int c0 = ci * 8;
            const int cnt = (D - c0 < 8) ? (D - c0) : 8;
            Fixed F = load_fixed<SCORER, T, VEC>(SLOT, fixrow, rrow, c0, D, h);
            f32x8 y0, y1;
            if (VEC) {
              y0 = lds_chunk(xr, ci, D);
              y1 = y0;
              if (CPLX) y1 = lds_chunk(xr + h, ci, D);
            } else {
              y0 = load_chunk<T, false>(xr, c0, D);
              y1 = y0;
              if (CPLX) y1 = load_chunk<T, false>(xr + h, c0, D);
            }
            P = apply_chunk<SCORER, NORM>(SLOT, P, F, y0, y1, VEC ? 8 : cnt, lp);
          }
          P = group_butterfly<G>(P);  // every lane of the group holds the sum
          const float sc = finalize<SCORER, NORM>(P, lp);
          if (lg == jj) res[m] = sc;
        }
      }
      // lane jj of the group wrote column m JG + jj: JG consecutive floats of row i per store instruction
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const int j = m * JG + lg;
        if (lg < JG && j < ncol) out[i * ldo + k0 + j] = res[m];
      }
    }
  };
  if (slot == 0) sweep(std::integral_constant<int, 0>{});
  else sweep(std::integral_constant<int, 2>{});
}

static long long sns_lds_bytes(int dtype, int d) {
  const long long es = dtype == KGE_BF16 ? 2 : 4;
  const long long pitch = (d + 7) & ~7;
  return (SNS_TU + 1) * pitch * es + 2LL * (SNS_TU + 1) * 8;
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
static int launch_neg_shared(const Operand& S, const Operand& R, const Operand& O, int d, int dr, long long n, int slot,
                             const Index& uniq, long long Uc, const long long* drop, const long long* rep, long long K,
                             float lp, float* out, long long ldo, long long lds_bytes, hipStream_t st) {
  auto kern = neg_shared_kernel<SCORER, T, NORM, VEC, G>;
  if (lds_bytes > 48 * 1024) {  // (a wide row: more dynamic LDS than a launch gets without asking)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SNS_LDS_MAX) != hipSuccess) {
      (void)hipGetLastError();
      return KGE_ERR_UNSUPPORTED;
    }
  }
  const dim3 grid((unsigned)((K + SNS_TU - 1) / SNS_TU), (unsigned)((n + SNS_TN - 1) / SNS_TN));
  hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds_bytes, st, S, R, O, d, dr, n, slot, uniq, Uc, drop, rep, K, lp,
                     out, ldo);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, typename T, int NORM, bool VEC, typename... A>
static int launch_neg_shared_g(int G, A... a) {
  switch (G) {
    case 8: return launch_neg_shared<SCORER, T, NORM, VEC, 8>(a...);
    case 16: return launch_neg_shared<SCORER, T, NORM, VEC, 16>(a...);
    case 32: return launch_neg_shared<SCORER, T, NORM, VEC, 32>(a...);
    case 64: return launch_neg_shared<SCORER, T, NORM, VEC, 64>(a...);
  }
  return KGE_ERR_UNSUPPORTED;
}

template <int SCORER, typename T, typename... A>
static int dispatch_neg_shared(int norm, bool vec, int G, A... a) {
#define KGE_GO(NORM, VEC) return launch_neg_shared_g<SCORER, T, NORM, VEC>(G, a...)
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

int run_neg_shared(int scorer, int dtype, const Operand& S, const Operand& R, const Operand& O, int d, int dr,
                   long long n, int slot, const Index& uniq, long long Uc, const long long* drop, const long long* rep,
                   long long K, float lp, float* out, long long ldo, hipStream_t st) {
  if (n == 0 || K == 0) return KGE_OK;
  const bool cplx = scorer == KGE_COMPLEX || scorer == KGE_ROTATE;
  if (cplx && (d % 2)) return KGE_ERR_INVALID_ARG;
  const long long lds_bytes = sns_lds_bytes(dtype, d);
  if (lds_bytes > SNS_LDS_MAX) return KGE_ERR_UNSUPPORTED;  // a row that does not fit the LDS tile
  if ((n + SNS_TN - 1) / SNS_TN > 65535 || (K + SNS_TU - 1) / SNS_TU > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  const int D = cplx ? d / 2 : d;
  const int G = group_size(D);
  const bool vec = vec_ok(scorer, dtype, d, dr, S, R, O);
  const int norm = norm_mode(lp);
#define KGE_DT(SC)                                                                                                    \
  return dtype == KGE_BF16 ? dispatch_neg_shared<SC, unsigned short>(norm, vec, G, S, R, O, d, dr, n, slot, uniq, Uc, \
                                                                     drop, rep, K, lp, out, ldo, lds_bytes, st)      \
                           : dispatch_neg_shared<SC, float>(norm, vec, G, S, R, O, d, dr, n, slot, uniq, Uc, drop, rep, \
                                                            K, lp, out, ldo, lds_bytes, st)
  switch (scorer) {
    case KGE_COMPLEX: KGE_DT(KGE_COMPLEX);
    case KGE_DISTMULT: KGE_DT(KGE_DISTMULT);
    case KGE_TRANSE: KGE_DT(KGE_TRANSE);
    case KGE_ROTATE: KGE_DT(KGE_ROTATE);
  }
#undef KGE_DT
  return KGE_ERR_INVALID_ARG;
}

// ---- backward -------------------------------------------------------------------------------------------------------
// workspace: W [n, P] (weights) and Dv [n, P] (distances = -score, for the norms that need them), P = physical rows
long long neg_shared_workspace_bytes(long long n, long long P) {
  const long long one = ((n * P * 4 + 255) / 256) * 256;
  return 2 * one;
}

// weight of pair (i, u) from the column that shows it: column u itself (unless dropped for i), for the spare the
// column drop[i]; pairs no column shows get 0
__global__ __launch_bounds__(256) void sns_fold_base_kernel(long long n, long long Uc, long long P,
                                                            const long long* __restrict__ drop,
                                                            const float* __restrict__ gout, long long ldg,
                                                            const float* __restrict__ scores, long long lds,
                                                            float* __restrict__ W, float* __restrict__ Dv) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * P) return;
  const long long i = idx / P, u = idx - i * P;
  const long long dri = drop ? drop[i] : -1;
  long long c;
  if (u < Uc) c = (dri == u) ? -1 : u;
  else c = (dri >= 0 && dri < Uc) ? dri : -1;
  W[idx] = c >= 0 ? gout[i * ldg + c] : 0.f;
  Dv[idx] = (c >= 0 && scores) ? -scores[i * lds + c] : 0.f;
}

// + the repeat columns (few: only sampling with replacement repeats)
__global__ __launch_bounds__(256) void sns_fold_repeat_kernel(long long n, long long Uc, long long P, long long nrep,
                                                              const long long* __restrict__ drop,
                                                              const long long* __restrict__ rep,
                                                              const float* __restrict__ gout, long long ldg,
                                                              float* __restrict__ W) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nrep) return;
  const long long i = idx / nrep, r = idx - i * nrep;
  const long long c = rep[r];
  if (c < 0 || c >= Uc) return;
  const long long dri = drop ? drop[i] : -1;
  const long long u = (dri == c) ? Uc : c;
  atomicAdd(W + i * P + u, gout[i * ldg + Uc + r]);
}

constexpr int SNB_OPW = 4;         // owners per wave
constexpr int SNB_OB = 4 * SNB_OPW;  // owners per workgroup
constexpr int SNB_SM = 8192;       // floats of staged rows: 64 / NC entity rows, or 32 / NC (entity, relation) row pairs

template <int SCORER, int NORM, int SLOT, int NC, int ROLE>
__global__ __launch_bounds__(256) void neg_shared_bwd_kernel(Operand S, Operand R, Operand O, int d, int dr, long long n,
                                                             Index uniq, long long P, float lp,
                                                             const float* __restrict__ W, const float* __restrict__ Dv,
                                                             float* __restrict__ ge, long long ge_ld,
                                                             float* __restrict__ gr, long long gr_ld) {
  constexpr int TS = (ROLE == 0 ? 64 : 32) / NC;  // streamed items per tile
  __shared__ float sm[SNB_SM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hh = (d + 1) / 2, lim1 = d - hh;
  const int rl0 = (SCORER == KGE_ROTATE) ? dr : hh;
  const int rl1 = (SCORER == KGE_ROTATE) ? 0 : lim1;
  const float* ent = (const float*)S.base;  // S.base == O.base: the entity table
  const float* rel = (const float*)R.base;
  const Index& fix = SLOT == 0 ? O.idx : S.idx;
  const long long nstream = ROLE == 0 ? P : n, nown = ROLE == 0 ? n : P;
  const long long j0 = (long long)blockIdx.x * TS;
  const int cnt = (int)(nstream - j0 < TS ? nstream - j0 : TS);
  float* smr = sm + TS * d;  // ROLE 1: the relation rows

  // stage the streamed rows
  for (int j = wave; j < cnt; j += 4) {
    if (ROLE == 0) {
      const float* src = ent + index_at(uniq, j0 + j) * S.ld;
      for (int c = lane; c < d; c += 64) sm[j * d + c] = src[c];
    } else {
      const float* src = ent + index_at(fix, j0 + j) * S.ld;
      for (int c = lane; c < d; c += 64) sm[j * d + c] = src[c];
      const float* rsrc = rel + index_at(R.idx, j0 + j) * R.ld;
      for (int c = lane; c < dr; c += 64) smr[j * dr + c] = rsrc[c];
    }
  }
  __syncthreads();

  const long long ob = (long long)blockIdx.y * SNB_OB + wave * SNB_OPW;
  for (int q = 0; q < SNB_OPW; ++q) {
    const long long w = ob + q;
    if (w >= nown) break;
    // this owner's weights / distances against the tile, one streamed item per lane
    float m_g = 0.f, m_dist = 0.f;
    if (lane < cnt) {
      const long long at = ROLE == 0 ? w * P + j0 + lane : (j0 + lane) * P + w;
      m_g = W[at];
      m_dist = Dv[at];
    }
    float a0[NC], a1[NC], b0[NC], b1[NC];  // ROLE 0: fixed entity row, relation row; ROLE 1: the physical row (a)
    float acc_a0[NC], acc_a1[NC], acc_b0[NC], acc_b1[NC];
    long long ea, eb = 0;
    if (ROLE == 0) {
      ea = index_at(fix, w);
      eb = index_at(R.idx, w);
    } else {
      ea = index_at(uniq, w);
    }
    const float* arow = ent + ea * S.ld;
    const float* brow = rel + eb * R.ld;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = lane + 64 * k;
      a0[k] = c < hh ? arow[c] : 0.f;
      a1[k] = c < lim1 ? arow[hh + c] : 0.f;
      b0[k] = (ROLE == 0 && c < rl0) ? brow[c] : 0.f;
      b1[k] = (ROLE == 0 && c < rl1) ? brow[hh + c] : 0.f;
      acc_a0[k] = acc_a1[k] = acc_b0[k] = acc_b1[k] = 0.f;
    }
    for (int j = 0; j < cnt; ++j) {
      const float g = __shfl(m_g, j, 64);
      if (g == 0.f) continue;  // (wave-uniform) a pair no column shows, or a zero weight: contributes nothing
      const float dist = __shfl(m_dist, j, 64);
      const float* er = sm + j * d;
      const float* rr = smr + j * dr;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = lane + 64 * k;
        if (c >= hh) break;
        const bool has1 = c < lim1;
        const float e0 = er[c], e1 = has1 ? er[hh + c] : 0.f;
        float f0, f1, r0, r1, v0, v1;  // fixed entity row, relation row, varying (physical) row
        if (ROLE == 0) {
          f0 = a0[k]; f1 = a1[k]; r0 = b0[k]; r1 = b1[k]; v0 = e0; v1 = e1;
        } else {
          f0 = e0; f1 = e1; v0 = a0[k]; v1 = a1[k];
          r0 = c < rl0 ? rr[c] : 0.f;
          r1 = c < rl1 ? rr[hh + c] : 0.f;
        }
        float ds0, ds1, dp0, dp1, do0, do1;
        if (SLOT == 0)
          spo_pair_grads<SCORER, NORM>(v0, v1, r0, r1, f0, f1, has1, g, dist, lp, ds0, ds1, dp0, dp1, do0, do1);
        else
          spo_pair_grads<SCORER, NORM>(f0, f1, r0, r1, v0, v1, has1, g, dist, lp, ds0, ds1, dp0, dp1, do0, do1);
        if (ROLE == 0) {
          acc_a0[k] += SLOT == 0 ? do0 : ds0;
          acc_a1[k] += SLOT == 0 ? do1 : ds1;
          acc_b0[k] += dp0;
          acc_b1[k] += dp1;
        } else {
          acc_a0[k] += SLOT == 0 ? ds0 : do0;
          acc_a1[k] += SLOT == 0 ? ds1 : do1;
        }
      }
    }
    float* ga = ge + ea * ge_ld;
    float* gb = gr + eb * gr_ld;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = lane + 64 * k;
      if (c < hh) unsafeAtomicAdd(ga + c, acc_a0[k]);
      if (c < lim1) unsafeAtomicAdd(ga + hh + c, acc_a1[k]);
      if (ROLE == 0) {
        if (c < rl0) unsafeAtomicAdd(gb + c, acc_b0[k]);
        if (c < rl1) unsafeAtomicAdd(gb + hh + c, acc_b1[k]);
      }
    }
  }
}

template <int SCORER, int NORM, int SLOT, int NC>
static int launch_neg_shared_bwd(const Operand& S, const Operand& R, const Operand& O, int d, int dr, long long n,
                                 const Index& uniq, long long P, float lp, const float* W, const float* Dv, float* ge,
                                 long long ge_ld, float* gr, long long gr_ld, hipStream_t st) {
  constexpr int TS0 = 64 / NC, TS1 = 32 / NC;
  const long long gx0 = (P + TS0 - 1) / TS0, gy0 = (n + SNB_OB - 1) / SNB_OB;
  const long long gx1 = (n + TS1 - 1) / TS1, gy1 = (P + SNB_OB - 1) / SNB_OB;
  if (gy0 > 65535 || gy1 > 65535 || gx0 > 0x7fffffffLL || gx1 > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((neg_shared_bwd_kernel<SCORER, NORM, SLOT, NC, 0>), dim3((unsigned)gx0, (unsigned)gy0), dim3(256),
                     0, st, S, R, O, d, dr, n, uniq, P, lp, W, Dv, ge, ge_ld, gr, gr_ld);
  hipLaunchKernelGGL((neg_shared_bwd_kernel<SCORER, NORM, SLOT, NC, 1>), dim3((unsigned)gx1, (unsigned)gy1), dim3(256),
                     0, st, S, R, O, d, dr, n, uniq, P, lp, W, Dv, ge, ge_ld, gr, gr_ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, int NORM, typename... A>
static int dispatch_neg_shared_bwd(int slot, int nc, A... a) {
#define KGE_NC(SL)                                                              \
  switch (nc) {                                                                 \
    case 1: return launch_neg_shared_bwd<SCORER, NORM, SL, 1>(a...);            \
    case 2: return launch_neg_shared_bwd<SCORER, NORM, SL, 2>(a...);            \
    case 4: return launch_neg_shared_bwd<SCORER, NORM, SL, 4>(a...);            \
    case 8: return launch_neg_shared_bwd<SCORER, NORM, SL, 8>(a...);            \
  }                                                                             \
  return KGE_ERR_UNSUPPORTED
  if (slot == 0) { KGE_NC(0); }
  KGE_NC(2);
#undef KGE_NC
}

int run_neg_shared_bwd_accum(int scorer, float lp, const Operand& S, const Operand& R, const Operand& O, int d, int dr,
                             long long n, int slot, const Index& uniq, long long Uc, const long long* drop,
                             const long long* rep, long long nrep, const float* gout, long long ldg,
                             const float* scores, long long lds, float* ge, long long ge_ld, float* gr, long long gr_ld,
                             void* ws, long long ws_bytes, hipStream_t st) {
  if (n == 0 || Uc + nrep == 0) return KGE_OK;
  const int hh = (d + 1) / 2;
  if (hh > 64 * 8) return KGE_ERR_UNSUPPORTED;
  int nc = 1;
  while (64 * nc < hh) nc <<= 1;
  const int norm = norm_mode(lp);
  const bool dot = scorer == KGE_COMPLEX || scorer == KGE_DISTMULT;
  if (!dot && norm != NORM_L1 && !scores) return KGE_ERR_INVALID_ARG;
  const long long P = Uc + (drop ? 1 : 0);
  if (n * P > (1LL << 40)) return KGE_ERR_UNSUPPORTED;
  const long long need = neg_shared_workspace_bytes(n, P);
  if (!ws || ws_bytes < need) return KGE_ERR_WORKSPACE;
  float* W = (float*)ws;
  float* Dv = (float*)((char*)ws + need / 2);
  const long long fb = (n * P + 255) / 256, fr = (n * nrep + 255) / 256;
  if (fb > 0x7fffffffLL || fr > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sns_fold_base_kernel, dim3((unsigned)fb), dim3(256), 0, st, n, Uc, P, drop, gout, ldg,
                     (dot || norm == NORM_L1) ? (const float*)nullptr : scores, lds, W, Dv);
  if (nrep > 0)
    hipLaunchKernelGGL(sns_fold_repeat_kernel, dim3((unsigned)fr), dim3(256), 0, st, n, Uc, P, nrep, drop, rep, gout,
                       ldg, W);
  if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
#define KGE_SB(SC, NM) \
  return dispatch_neg_shared_bwd<SC, NM>(slot, nc, S, R, O, d, dr, n, uniq, P, lp, (const float*)W, (const float*)Dv, ge, ge_ld, gr, gr_ld, st)
  switch (scorer) {
    case KGE_COMPLEX: KGE_SB(KGE_COMPLEX, NORM_L1);
    case KGE_DISTMULT: KGE_SB(KGE_DISTMULT, NORM_L1);
    case KGE_TRANSE:
      if (norm == NORM_L1) KGE_SB(KGE_TRANSE, NORM_L1);
      if (norm == NORM_L2) KGE_SB(KGE_TRANSE, NORM_L2);
      KGE_SB(KGE_TRANSE, NORM_LP);
    case KGE_ROTATE:
      if (norm == NORM_L1) KGE_SB(KGE_ROTATE, NORM_L1);
      if (norm == NORM_L2) KGE_SB(KGE_ROTATE, NORM_L2);
      KGE_SB(KGE_ROTATE, NORM_LP);
  }
#undef KGE_SB
  return KGE_ERR_INVALID_ARG;
}

}  // namespace kge
