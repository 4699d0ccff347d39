// score_so.hip -- relation prediction: KgeModel.score_so (kge_model.py:727-747), gfx950.
//
// out[i, j] = score(s[i], rels[j], o[i]): n (s, o) pairs against m relations (all of them, or a listed subset).  The
// reference composes it from three repeats to [n m, d] and the spo scorer (RelationalScorer.score_emb, "s_o":
// kge_model.py:202-209); here nothing but the [n, m] scores is written.  The relation table is small and every pair
// reads all of it: the call is bound by LDS and VALU, not by HBM.
//
// Forward (so_kernel): a workgroup owns SO_TN pairs x `tr` relation rows (32, or 16 where 32 staged rows do not fit
// the LDS).  The relation rows are staged ONCE per workgroup with 16-byte loads; RotatE stages cos / sin of the
// phases (sincos_canon once per staged element -- n / 32 * m * d / 2 evaluations per call, not n * m * d / 2).  A
// group of G lanes owns one pair at a time: its s and o chunks in registers, it walks the staged rows, forms the
// query with prep_chunk_staged and accumulates against o with apply_chunk(slot = 2).  Lane-to-coordinate layout,
// per-chunk arithmetic, the xor butterfly and finalize are those of score_spo.hip (spo_device.hpp): every score has
// the bits kge_score_spo stores for (s[i], rels[j], o[i]).
//
// Backward (kge_score_so_bwd_accum): two passes of so_bwd_kernel over the [n, m] block, the structure of
// neg_shared_bwd_kernel (score_neg_shared.hip):
//   ROLE 0  a wave owns a pair: its s and o rows in registers, both gradients summed in registers over a tile of
//           relation rows staged in LDS (RotatE: as cos / sin), one atomic flush of each per (pair, tile);
//   ROLE 1  a wave owns an entry of rels: its relation row in registers (RotatE: cos / sin), its gradient summed in
//           registers over a tile of pairs (their s and o rows staged in LDS), one atomic flush per (relation, tile).
// Tiles are 64 / NC relation rows (ROLE 0) and 32 / NC pairs (ROLE 1), NC = 1, 2, 4, 8 coordinate pairs per lane for
// ceil(d / 2) <= 64, 128, 256, 512.  gout and the forward scores are read in place: no workspace.
#include "bwd_device.hpp"
#include "spo_device.hpp"

namespace kge {

constexpr int SO_TN = 32;  // pairs per workgroup
constexpr int SO_TR = 32;  // staged relation rows per workgroup, at most
constexpr long long SO_LDS_MAX = 160 * 1024;

// one lane's chunk ci of a staged half-row (vector path): the layout of score_neg_shared.hip -- f32 half-rows are
// staged as [all low 16-byte halves of the chunks][all high halves], so that 16 consecutive lanes read 256
// consecutive bytes per ds_read_b128; bf16 chunks are 16 bytes and staged as they are
__device__ __forceinline__ f32x8 so_lds_chunk(const float* half_row, int ci, int D) {
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
__device__ __forceinline__ f32x8 so_lds_chunk(const unsigned short* half_row, int ci, int D) {
  return ld8<unsigned short>(half_row + 8 * ci);
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
__global__ __launch_bounds__(256) void so_kernel(Operand S, Operand R, Operand O, int d, long long n, long long m,
                                                 int tr, float lp, float* __restrict__ out, long long ldo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char so_smem[];
  constexpr bool CPLX = IsComplex<SCORER>::value;
  constexpr bool ROT = SCORER == KGE_ROTATE;
  using LT = typename std::conditional<ROT, float, T>::type;  // what a staged row holds (RotatE: cos | sin)
  constexpr int GPB = 256 / G;                 // groups per workgroup
  constexpr int JG = G < SO_TR ? G : SO_TR;    // columns whose scores one round of a group's lanes keeps
  constexpr int NM = SO_TR / JG;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int lg = lane & (G - 1);
  const int gid = (tid >> 6) * (64 / G) + lane / G;
  const int h = d / 2;
  const int D = CPLX ? h : d;
  const int nchunks = (D + 7) / 8;
  const int pitch = (d + 7) & ~7;  // elements of LT (RotatE: 2 D = d floats); rows start 16-byte aligned
  LT* rows = reinterpret_cast<LT*>(so_smem);
  long long* rowid = reinterpret_cast<long long*>(so_smem + (size_t)tr * pitch * sizeof(LT));
  const long long k0 = (long long)blockIdx.x * tr;
  const int ncol = (int)(m - k0 < tr ? m - k0 : tr);
  const long long i0 = (long long)blockIdx.y * SO_TN;
  const T* ent = (const T*)S.base;  // S.base == O.base == entity table
  const T* rel = (const T*)R.base;

  // 1. the relation row behind every column of the tile
  if (tid < ncol) rowid[tid] = index_at(R.idx, k0 + tid);
  __syncthreads();

  // 2. stage the rows: every relation row is fetched once per workgroup
  if (ROT) {
    for (int idx = tid; idx < ncol * D; idx += 256) {
      const int j = idx / D, w = idx - j * D;
      float sn, cs;
      sincos_canon(ld1<T>(rel + rowid[j] * R.ld + w), sn, cs);
      const int pos = VEC ? ((w >> 2) & 1) * (D >> 1) + 4 * (w >> 3) + (w & 3) : w;
      rows[(size_t)j * pitch + pos] = (LT)cs;
      rows[(size_t)j * pitch + D + pos] = (LT)sn;
    }
  } else if (VEC) {
    const int ppr = (int)(d * sizeof(T) / 16);  // 16-byte pieces per row
    for (int idx = tid; idx < ncol * ppr; idx += 256) {
      const int j = idx / ppr, q = idx - j * ppr;
      const u32x4 v = *(reinterpret_cast<const u32x4*>(rel + rowid[j] * R.ld) + q);
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
    for (int idx = tid; idx < ncol * d; idx += 256) {
      const int j = idx / d, e = idx - j * d;
      rows[(size_t)j * pitch + e] = (LT)rel[rowid[j] * R.ld + e];
    }
  }
  __syncthreads();

  // 3. every group walks the staged rows for one pair at a time
  const int c00 = lg * 8;
  const int cnt0 = (D - c00 < 8) ? (D - c00) : 8;
  const bool act = lg < nchunks;
  auto staged = [&](const LT* rr, int ci, int c0, f32x8& r0, f32x8& r1) {
    if (VEC) {
      r0 = so_lds_chunk(rr, ci, D);
      r1 = r0;
      if (CPLX) r1 = so_lds_chunk(rr + D, ci, D);
    } else {
      r0 = load_chunk<LT, false>(rr, c0, D);
      r1 = r0;
      if (CPLX) r1 = load_chunk<LT, false>(rr + D, c0, D);
    }
  };
  for (int pp = gid; pp < SO_TN; pp += GPB) {
    const long long i = i0 + pp;
    if (i >= n) continue;  // (a whole group: the butterfly stays inside it)
    const T* srow = ent + index_at(S.idx, i) * S.ld;
    const T* orow = (const T*)O.base + index_at(O.idx, i) * O.ld;
    f32x8 e0, e1, x0, x1;  // the pair's first chunk: s halves, o halves
    if (act) {
      e0 = load_chunk<T, VEC>(srow, c00, D);
      x0 = load_chunk<T, VEC>(orow, c00, D);
      e1 = e0;
      x1 = x0;
      if (CPLX) {
        e1 = load_chunk<T, VEC>(srow + h, c00, D);
        x1 = load_chunk<T, VEC>(orow + h, c00, D);
      }
    }
    float res[NM];
#pragma unroll
    for (int mm = 0; mm < NM; ++mm) {
      res[mm] = 0.0f;
      for (int jj = 0; jj < JG; ++jj) {
        const int j = mm * JG + jj;
        if (j >= ncol) break;
        const LT* rr = rows + (size_t)j * pitch;
        float P = 0.0f;
        if (act) {
          f32x8 r0, r1;
          staged(rr, lg, c00, r0, r1);
          const Fixed F = prep_chunk_staged<SCORER>(e0, e1, r0, r1);
          P = apply_chunk<SCORER, NORM>(2, P, F, x0, x1, VEC ? 8 : cnt0, lp);
        }
        for (int ci = lg + 64; ci < nchunks; ci += 64) {  // only when D > 512
          const int c0 = ci * 8;
          const int cnt = (D - c0 < 8) ? (D - c0) : 8;
          f32x8 f0 = load_chunk<T, VEC>(srow, c0, D), y0 = load_chunk<T, VEC>(orow, c0, D);
          f32x8 f1 = f0, y1 = y0;
          if (CPLX) {
            f1 = load_chunk<T, VEC>(srow + h, c0, D);
            y1 = load_chunk<T, VEC>(orow + h, c0, D);
          }
          f32x8 r0, r1;
          staged(rr, ci, c0, r0, r1);
          const Fixed F = prep_chunk_staged<SCORER>(f0, f1, r0, r1);
          P = apply_chunk<SCORER, NORM>(2, P, F, y0, y1, VEC ? 8 : cnt, lp);
        }
        P = group_butterfly<G>(P);  // every lane of the group holds the sum
        const float sc = finalize<SCORER, NORM>(P, lp);
        if (lg == jj) res[mm] = sc;
      }
    }
    // lane jj of the group holds column mm JG + jj: JG consecutive floats of row i per store instruction
#pragma unroll
    for (int mm = 0; mm < NM; ++mm) {
      const int j = mm * JG + lg;
      if (lg < JG && j < ncol) out[i * ldo + k0 + j] = res[mm];
    }
  }
}

// bytes of one staged relation row (RotatE: cos | sin as float whatever the table holds)
static long long so_row_bytes(int scorer, int dtype, int d) {
  const long long es = (scorer == KGE_ROTATE || dtype != KGE_BF16) ? 4 : 2;
  return (long long)((d + 7) & ~7) * es;
}

template <int SCORER, typename T, int NORM, bool VEC, int G>
static int launch_so(const Operand& S, const Operand& R, const Operand& O, int d, long long n, long long m, int tr,
                     float lp, float* out, long long ldo, long long lds_bytes, hipStream_t st) {
  auto kern = so_kernel<SCORER, T, NORM, VEC, G>;
  if (lds_bytes > 48 * 1024) {  // (a wide row: more dynamic LDS than a launch gets without asking)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)SO_LDS_MAX) != hipSuccess) {
      (void)hipGetLastError();
      return KGE_ERR_UNSUPPORTED;
    }
  }
  const dim3 grid((unsigned)((m + tr - 1) / tr), (unsigned)((n + SO_TN - 1) / SO_TN));
  hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds_bytes, st, S, R, O, d, n, m, tr, lp, out, ldo);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, typename T, int NORM, bool VEC, typename... A>
static int launch_so_g(int G, A... a) {
  switch (G) {
    case 8: return launch_so<SCORER, T, NORM, VEC, 8>(a...);
    case 16: return launch_so<SCORER, T, NORM, VEC, 16>(a...);
    case 32: return launch_so<SCORER, T, NORM, VEC, 32>(a...);
    case 64: return launch_so<SCORER, T, NORM, VEC, 64>(a...);
  }
  return KGE_ERR_UNSUPPORTED;
}

template <int SCORER, typename T, typename... A>
static int dispatch_so(int norm, bool vec, int G, A... a) {
#define KGE_GO(NORM, VEC) return launch_so_g<SCORER, T, NORM, VEC>(G, a...)
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

// can kge_score_so take these tables at all?  (KGE_ERR_UNSUPPORTED before any launch otherwise)
bool so_tables_ok(int scorer, int dtype, long long d) {
  if (scorer != KGE_COMPLEX && scorer != KGE_DISTMULT && scorer != KGE_TRANSE && scorer != KGE_ROTATE) return false;
  return d <= (dtype == KGE_BF16 ? 2048 : 1024);  // the limits of kge_score_neg_shared
}

int run_so(int scorer, int dtype, const Operand& S, const Operand& R, const Operand& O, int d, int dr, long long n,
           long long m, float lp, float* out, long long ldo, hipStream_t st) {
  if (n == 0 || m == 0) return KGE_OK;
  if (!so_tables_ok(scorer, dtype, d)) return KGE_ERR_UNSUPPORTED;
  const bool cplx = scorer == KGE_COMPLEX || scorer == KGE_ROTATE;
  if (cplx && (d % 2)) return KGE_ERR_INVALID_ARG;
  const long long row_bytes = so_row_bytes(scorer, dtype, d);
  int tr = SO_TR;
  if (tr * (row_bytes + 8) > SO_LDS_MAX) tr = SO_TR / 2;
  const long long lds_bytes = tr * (row_bytes + 8);
  if (lds_bytes > SO_LDS_MAX) return KGE_ERR_UNSUPPORTED;  // a row that does not fit the LDS tile
  if ((n + SO_TN - 1) / SO_TN > 65535 || (m + tr - 1) / tr > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  const int D = cplx ? d / 2 : d;
  const int G = group_size(D);
  const bool vec = vec_ok(scorer, dtype, d, dr, S, R, O);
  const int norm = norm_mode(lp);
#define KGE_DT(SC)                                                                                                   \
  return dtype == KGE_BF16                                                                                           \
             ? dispatch_so<SC, unsigned short>(norm, vec, G, S, R, O, d, n, m, tr, lp, out, ldo, lds_bytes, st)      \
             : dispatch_so<SC, float>(norm, vec, G, S, R, O, d, n, m, tr, lp, out, ldo, lds_bytes, st)
  switch (scorer) {
    case KGE_COMPLEX: KGE_DT(KGE_COMPLEX);
    case KGE_DISTMULT: KGE_DT(KGE_DISTMULT);
    case KGE_TRANSE: KGE_DT(KGE_TRANSE);
    case KGE_ROTATE: KGE_DT(KGE_ROTATE);
  }
#undef KGE_DT
  return KGE_ERR_UNSUPPORTED;
}

// ---- backward -------------------------------------------------------------------------------------------------------
constexpr int SOB_OPW = 4;           // owners per wave
constexpr int SOB_OB = 4 * SOB_OPW;  // owners per workgroup
constexpr int SOB_SM = 8192;         // floats of staged rows: 64 / NC relation rows, or 32 / NC (s, o) row pairs

template <int SCORER, int NORM, int NC, int ROLE>
__global__ __launch_bounds__(256) void so_bwd_kernel(Operand S, Operand R, Operand O, int d, int dr, long long n,
                                                     long long m, float lp, const float* __restrict__ gout,
                                                     long long ldg, const float* __restrict__ scores, long long lds,
                                                     float* __restrict__ ge, long long ge_ld, float* __restrict__ gr,
                                                     long long gr_ld) {
  constexpr bool ROT = SCORER == KGE_ROTATE;
  constexpr int TS = (ROLE == 0 ? 64 : 32) / NC;  // streamed items per tile
  __shared__ float sm[SOB_SM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hh = (d + 1) / 2, lim1 = d - hh;
  const int rl0 = ROT ? dr : hh;
  const int rl1 = ROT ? 0 : lim1;
  const float* ent = (const float*)S.base;  // S.base == O.base: the entity table
  const float* rel = (const float*)R.base;
  const long long nstream = ROLE == 0 ? m : n, nown = ROLE == 0 ? n : m;
  const long long j0 = (long long)blockIdx.x * TS;
  const int cnt = (int)(nstream - j0 < TS ? nstream - j0 : TS);
  float* smo = sm + TS * d;  // ROLE 1: the o rows

  // stage the streamed rows (ROLE 0, RotatE: [cos | sin] of the phases, d = 2 dr floats per row)
  for (int j = wave; j < cnt; j += 4) {
    if (ROLE == 0) {
      const float* src = rel + index_at(R.idx, j0 + j) * R.ld;
      for (int c = lane; c < dr; c += 64) {
        if (ROT) {
          float sn, cs;
          sincos_canon(src[c], sn, cs);
          sm[j * d + c] = cs;
          sm[j * d + dr + c] = sn;
        } else {
          sm[j * d + c] = src[c];
        }
      }
    } else {
      const float* ssrc = ent + index_at(S.idx, j0 + j) * S.ld;
      const float* osrc = ent + index_at(O.idx, j0 + j) * O.ld;
      for (int c = lane; c < d; c += 64) {
        sm[j * d + c] = ssrc[c];
        smo[j * d + c] = osrc[c];
      }
    }
  }
  __syncthreads();

  const long long ob = (long long)blockIdx.y * SOB_OB + wave * SOB_OPW;
  for (int q = 0; q < SOB_OPW; ++q) {
    const long long w = ob + q;
    if (w >= nown) break;
    // this owner's weights / distances against the tile, one streamed item per lane
    float m_g = 0.f, m_dist = 0.f;
    if (lane < cnt) {
      const long long row = ROLE == 0 ? w : j0 + lane, col = ROLE == 0 ? j0 + lane : w;
      m_g = gout[row * ldg + col];
      if (scores) m_dist = -scores[row * lds + col];
    }
    // ROLE 0: a = the s row, b = the o row; ROLE 1: a = the relation row (RotatE: a0 = cos, a1 = sin)
    float a0[NC], a1[NC], b0[NC], b1[NC];
    float acc_a0[NC], acc_a1[NC], acc_b0[NC], acc_b1[NC];
    long long ea, eb = 0;
    if (ROLE == 0) {
      ea = index_at(S.idx, w);
      eb = index_at(O.idx, w);
    } else {
      ea = index_at(R.idx, w);
    }
    const float* arow = ROLE == 0 ? ent + ea * S.ld : rel + ea * R.ld;
    const float* brow = ent + eb * O.ld;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = lane + 64 * k;
      if (ROLE == 0) {
        a0[k] = c < hh ? arow[c] : 0.f;
        a1[k] = c < lim1 ? arow[hh + c] : 0.f;
        b0[k] = c < hh ? brow[c] : 0.f;
        b1[k] = c < lim1 ? brow[hh + c] : 0.f;
      } else {
        a0[k] = c < rl0 ? arow[c] : 0.f;
        a1[k] = c < rl1 ? arow[hh + c] : 0.f;
        if (ROT) {
          float sn, cs;
          sincos_canon(a0[k], sn, cs);
          a0[k] = cs;
          a1[k] = sn;
        }
        b0[k] = b1[k] = 0.f;
      }
      acc_a0[k] = acc_a1[k] = acc_b0[k] = acc_b1[k] = 0.f;
    }
    for (int j = 0; j < cnt; ++j) {
      const float g = __shfl(m_g, j, 64);
      if (g == 0.f) continue;  // (wave-uniform) a zero weight contributes nothing
      const float dist = __shfl(m_dist, j, 64);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = lane + 64 * k;
        if (c >= hh) break;
        const bool has1 = c < lim1;
        float s0, s1, r0, r1, o0, o1;
        if (ROLE == 0) {
          const float* rr = sm + j * d;
          s0 = a0[k]; s1 = a1[k]; o0 = b0[k]; o1 = b1[k];
          r0 = c < rl0 ? rr[c] : 0.f;
          if (ROT) r1 = c < rl0 ? rr[dr + c] : 0.f;
          else r1 = c < rl1 ? rr[hh + c] : 0.f;
        } else {
          const float* sr = sm + j * d;
          const float* orw = smo + j * d;
          s0 = sr[c]; s1 = has1 ? sr[hh + c] : 0.f;
          o0 = orw[c]; o1 = has1 ? orw[hh + c] : 0.f;
          r0 = a0[k]; r1 = a1[k];
        }
        float ds0, ds1, dp0, dp1, do0, do1;
        spo_pair_grads<SCORER, NORM, ROT>(s0, s1, r0, r1, o0, o1, has1, g, dist, lp, ds0, ds1, dp0, dp1, do0, do1);
        if (ROLE == 0) {
          acc_a0[k] += ds0;
          acc_a1[k] += ds1;
          acc_b0[k] += do0;
          acc_b1[k] += do1;
        } else {
          acc_a0[k] += dp0;
          acc_a1[k] += dp1;
        }
      }
    }
    if (ROLE == 0) {
      float* ga = ge + ea * ge_ld;
      float* gb = ge + eb * ge_ld;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = lane + 64 * k;
        if (c < hh) {
          unsafeAtomicAdd(ga + c, acc_a0[k]);
          unsafeAtomicAdd(gb + c, acc_b0[k]);
        }
        if (c < lim1) {
          unsafeAtomicAdd(ga + hh + c, acc_a1[k]);
          unsafeAtomicAdd(gb + hh + c, acc_b1[k]);
        }
      }
    } else {
      float* ga = gr + ea * gr_ld;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = lane + 64 * k;
        if (c < rl0) unsafeAtomicAdd(ga + c, acc_a0[k]);
        if (c < rl1) unsafeAtomicAdd(ga + hh + c, acc_a1[k]);
      }
    }
  }
}

template <int SCORER, int NORM, int NC>
static int launch_so_bwd(const Operand& S, const Operand& R, const Operand& O, int d, int dr, long long n, long long m,
                         float lp, const float* gout, long long ldg, const float* scores, long long lds, float* ge,
                         long long ge_ld, float* gr, long long gr_ld, hipStream_t st) {
  constexpr int TS0 = 64 / NC, TS1 = 32 / NC;
  const long long gx0 = (m + TS0 - 1) / TS0, gy0 = (n + SOB_OB - 1) / SOB_OB;
  const long long gx1 = (n + TS1 - 1) / TS1, gy1 = (m + SOB_OB - 1) / SOB_OB;
  if (gy0 > 65535 || gy1 > 65535 || gx0 > 0x7fffffffLL || gx1 > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((so_bwd_kernel<SCORER, NORM, NC, 0>), dim3((unsigned)gx0, (unsigned)gy0), dim3(256), 0, st, S, R,
                     O, d, dr, n, m, lp, gout, ldg, scores, lds, ge, ge_ld, gr, gr_ld);
  hipLaunchKernelGGL((so_bwd_kernel<SCORER, NORM, NC, 1>), dim3((unsigned)gx1, (unsigned)gy1), dim3(256), 0, st, S, R,
                     O, d, dr, n, m, lp, gout, ldg, scores, lds, ge, ge_ld, gr, gr_ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int SCORER, int NORM, typename... A>
static int dispatch_so_bwd(int nc, A... a) {
  switch (nc) {
    case 1: return launch_so_bwd<SCORER, NORM, 1>(a...);
    case 2: return launch_so_bwd<SCORER, NORM, 2>(a...);
    case 4: return launch_so_bwd<SCORER, NORM, 4>(a...);
    case 8: return launch_so_bwd<SCORER, NORM, 8>(a...);
  }
  return KGE_ERR_UNSUPPORTED;
}

// do the forward scores have to be given?  (TransE / RotatE with l_norm != 1: the distance enters the weights)
bool so_bwd_needs_scores(int scorer, float lp) {
  return (scorer == KGE_TRANSE || scorer == KGE_ROTATE) && norm_mode(lp) != NORM_L1;
}

int run_so_bwd_accum(int scorer, float lp, const Operand& S, const Operand& R, const Operand& O, int d, int dr,
                     long long n, long long m, const float* gout, long long ldg, const float* scores, long long lds,
                     float* ge, long long ge_ld, float* gr, long long gr_ld, hipStream_t st) {
  if (n == 0 || m == 0) return KGE_OK;
  const int hh = (d + 1) / 2;
  if (hh > 64 * 8) return KGE_ERR_UNSUPPORTED;
  int nc = 1;
  while (64 * nc < hh) nc <<= 1;
  const int norm = norm_mode(lp);
  const bool need = so_bwd_needs_scores(scorer, lp);
  if (need && !scores) return KGE_ERR_INVALID_ARG;
  const float* sc = need ? scores : (const float*)nullptr;
#define KGE_SB(SC, NM) \
  return dispatch_so_bwd<SC, NM>(nc, S, R, O, d, dr, n, m, lp, gout, ldg, sc, lds, ge, ge_ld, gr, gr_ld, st)
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
  return KGE_ERR_UNSUPPORTED;
}

}  // namespace kge
