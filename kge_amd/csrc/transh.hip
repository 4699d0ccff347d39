// transh.hip -- TransH (kge/model/transh.py) on gfx950: float32 tables, l_norm 1 / 2, exact VALU arithmetic
// (transh_device.hpp).
//
// The reference projects every target onto every relation's hyperplane and materialises [m, n, d]
// (transh.py:39-78; its own TODO at transh.py:28-29).  Here nothing of size n m d exists:
//
//   transh_pairs_kernel   sp_ / _po.  A workgroup owns 16 query rows and walks target tiles of 64 rows.  Prologue:
//                         per query row ||w||, a = w^ . q (8-lane groups, REDUCE8).  The rows sit in LDS in slices of
//                         128 coordinates: (fixed, w^) of the 16 queries and the 64 target rows.  A thread scores
//                         1 query x 4 targets: pass 1  c = w^ . t  (8 partial sums per pair in registers), pass 2 the
//                         norm of fixed - t + c w^ + eps.  d <= 128: a target row is read from HBM once per query tile
//                         and both passes run from LDS; wider rows are sliced and the slices loaded once per pass.
//   transh_spo_kernel     kge_score_spo: an 8-lane group per triple, three passes over the rows.
//   transh_neg_kernel     kge_score_neg: the positive's ||w|| and fixed-side coefficient are reduced once per run of
//                         negatives of a group; the corrupted rows stream.
//   backward              a wave per row, lane l owns the coordinates l, l + 64, ...  ||v|| of L2 is RECOMPUTED (the
//                         `scores` argument of the backward entry points is not read).
//                         kge_score_pairs_bwd: no float atomics -- transh_bwd_tgt_kernel sums over the query rows per
//                         target (g_tgt), transh_bwd_rows_kernel over the targets per query row (g_a, g_p): the same
//                         pairs twice, each output with one owner and a fixed order; two runs give the same bits.
//                         The _accum entry points run transh_bwd_rows_kernel with float atomics into the tables'
//                         gradients.
#include "transh_device.hpp"

namespace kge {

static inline bool th_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// every group of four coordinates of every row readable with one aligned 16-byte load
static bool th_vec_ok(int d, const Operand& A, const Operand& R, const Operand& B) {
  return d % 4 == 0 && th_aligned16(A.base) && th_aligned16(R.base) && th_aligned16(B.base) && A.ld % 4 == 0 &&
         R.ld % 4 == 0 && B.ld % 4 == 0;
}

// =====================================================================================================
// forward, pairs
// =====================================================================================================
constexpr int TH_TQ = 16, TH_TT = 64, TH_DC = 128, TH_LDP = TH_DC + 4;  // pitch = 4 mod 64 banks

// one group of 8 x 4 coordinates at LDS offset kb of the slice; KIND 0: dot products, 1: the norm's sum
template <int NORM, int KIND, bool GUARD>
__device__ __forceinline__ void th_tile_group(const float* __restrict__ sF, const float* __restrict__ sW,
                                              const float* __restrict__ sT, int kb, int kglobal, int d,
                                              const float (&c)[4], float (&acc)[4][8]) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(sW + kb + g * 4);
    f32x4 f4 = w4;
    if (KIND == 1) f4 = *reinterpret_cast<const f32x4*>(sF + kb + g * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(sT + u * 16 * TH_LDP + kb + g * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (KIND == 0) {
          acc[u][g] = __builtin_fmaf(w4[i], t4[i], acc[u][g]);
        } else if (!GUARD || kglobal + g * 4 + i < d) {
          acc[u][g] = th_acc<NORM>(acc[u][g], th_v(f4[i], t4[i], c[u], w4[i]));
        }
      }
    }
    // keep the LDS reads of the next group of four behind this one's arithmetic: hoisted to the front of the unrolled
    // body they took every register (256 VGPRs, scratch) -- the workgroups resident beside this one hide the latency
    asm volatile("" ::: "memory");
  }
}

template <int NORM, bool VEC>
__global__ __launch_bounds__(256) void transh_pairs_kernel(Operand A, Operand R, Operand TG, int dir, int d, long long n,
                                                           long long m, int tiles_per_wg, float* __restrict__ out,
                                                           long long ldo) {
  __shared__ __attribute__((aligned(16))) float sF[TH_TQ * TH_LDP];
  __shared__ __attribute__((aligned(16))) float sW[TH_TQ * TH_LDP];
  __shared__ __attribute__((aligned(16))) float sT[TH_TT * TH_LDP];
  __shared__ float sDen[TH_TQ], sA[TH_TQ];
  const int tid = threadIdx.x;
  const long long q0 = (long long)blockIdx.y * TH_TQ;
  const float* ent = (const float*)A.base;
  const float* rel = (const float*)R.base;

  // prologue: threads 0..127 = 16 groups of 8 lanes, one per query row (whole waves: the shuffles see all lanes)
  if (tid < 128) {
    const int g = tid >> 3, lg = tid & 7;
    long long row = q0 + g;
    if (row >= n) row = n - 1;
    const float* e = ent + index_at(A.idx, row) * A.ld;
    const float* w = rel + index_at(R.idx, row) * R.ld + d;
    const float den = th_den(th_group_nw2<VEC>(w, d, lg));
    const float a = th_group_dot<VEC>(w, den, e, d, lg);
    if (lg == 0) {
      sDen[g] = den;
      sA[g] = a;
    }
  }
  __syncthreads();

  const int nslices = (d + TH_DC - 1) / TH_DC;
  const int tq = tid >> 4, tt = tid & 15;
  const long long mt = (m + TH_TT - 1) / TH_TT;
  const long long tile0 = (long long)blockIdx.x * tiles_per_wg;
  for (long long tile = tile0; tile < tile0 + tiles_per_wg && tile < mt; ++tile) {
    const long long t0 = tile * TH_TT;
    float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float acc[4][8];
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < 8; ++g) acc[u][g] = 0.0f;
      for (int sl = 0; sl < nslices; ++sl) {
        const int kbase = sl * TH_DC;
        const bool load_q = nslices > 1 || (tile == tile0 && pass == 0);
        const bool load_t = nslices > 1 || pass == 0;
        if (load_q || load_t) __syncthreads();  // the readers of the previous slice are done
        if (load_q) {
          for (int x = tid; x < TH_TQ * (TH_DC / 4); x += 256) {
            const int r = x / (TH_DC / 4), c4 = x % (TH_DC / 4);
            const int k0 = kbase + c4 * 4;
            f32x4 F = {0.0f, 0.0f, 0.0f, 0.0f}, W = F;
            if (q0 + r < n && k0 < d) {
              const float* e = ent + index_at(A.idx, q0 + r) * A.ld;
              const float* rr = rel + index_at(R.idx, q0 + r) * R.ld;
              const f32x4 e4 = th_ld4<VEC>(e, k0, d), d4 = th_ld4<VEC>(rr, k0, d), w4 = th_ld4<VEC>(rr + d, k0, d);
              const float den = sDen[r], a = sA[r];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (VEC || k0 + i < d) {
                  W[i] = th_what(w4[i], den);
                  F[i] = dir == KGE_SP_ ? th_fixed<1>(e4[i], W[i], a, d4[i]) : th_fixed<-1>(e4[i], W[i], a, d4[i]);
                }
            }
            *reinterpret_cast<f32x4*>(sF + r * TH_LDP + c4 * 4) = F;
            *reinterpret_cast<f32x4*>(sW + r * TH_LDP + c4 * 4) = W;
          }
        }
        if (load_t) {
          for (int x = tid; x < TH_TT * (TH_DC / 4); x += 256) {
            const int r = x / (TH_DC / 4), c4 = x % (TH_DC / 4);
            const int k0 = kbase + c4 * 4;
            f32x4 T4 = {0.0f, 0.0f, 0.0f, 0.0f};
            if (t0 + r < m && k0 < d)
              T4 = th_ld4<VEC>((const float*)TG.base + index_at(TG.idx, t0 + r) * TG.ld, k0, d);
            *reinterpret_cast<f32x4*>(sT + r * TH_LDP + c4 * 4) = T4;
          }
        }
        if (load_q || load_t) __syncthreads();
        const int left = d - kbase < TH_DC ? d - kbase : TH_DC;
        const float* pF = sF + tq * TH_LDP;
        const float* pW = sW + tq * TH_LDP;
        const float* pT = sT + tt * TH_LDP;
#pragma unroll 1
        for (int kb = 0; kb < left; kb += 32) {
          if (pass == 0) th_tile_group<NORM, 0, false>(pF, pW, pT, kb, kbase + kb, d, c, acc);
          else if (kb + 32 <= left) th_tile_group<NORM, 1, false>(pF, pW, pT, kb, kbase + kb, d, c, acc);
          else th_tile_group<NORM, 1, true>(pF, pW, pT, kb, kbase + kb, d, c, acc);
        }
      }
      if (pass == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = th_combine8(acc[u]);
      }
    }
    if (q0 + tq < n) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long j = t0 + tt + 16 * u;
        if (j < m) out[(q0 + tq) * ldo + j] = th_score<NORM>(th_combine8(acc[u]));
      }
    }
  }
}

int run_transh_pairs(const Operand& A, const Operand& R, const Operand& TG, int dir, int d, long long n, long long m,
                     float lp, float* out, long long ldo, hipStream_t st) {
  if (n == 0 || m == 0) return KGE_OK;
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || d > 1024) return KGE_ERR_UNSUPPORTED;
  const long long qt = (n + TH_TQ - 1) / TH_TQ, mt = (m + TH_TT - 1) / TH_TT;
  if (qt > 65535) return KGE_ERR_UNSUPPORTED;
  // target tiles per workgroup: the prologue and (d <= 128) the query slice are paid once per workgroup; as many
  // tiles as still leave ~1024 workgroups, at most 8
  int per = 8;
  while (per > 1 && qt * ((mt + per - 1) / per) < 1024) per >>= 1;
  const dim3 grid((unsigned)((mt + per - 1) / per), (unsigned)qt);
  const bool vec = th_vec_ok(d, A, R, TG);
#define KGE_TH_GO(NORM, VEC)                                                                                       \
  hipLaunchKernelGGL((transh_pairs_kernel<NORM, VEC>), grid, dim3(256), 0, st, A, R, TG, dir, d, n, m, per, out, ldo)
  if (norm == NORM_L1) {
    if (vec) KGE_TH_GO(NORM_L1, true); else KGE_TH_GO(NORM_L1, false);
  } else {
    if (vec) KGE_TH_GO(NORM_L2, true); else KGE_TH_GO(NORM_L2, false);
  }
#undef KGE_TH_GO
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// =====================================================================================================
// forward, row-wise: kge_score_spo and kge_score_neg (the sampler's "triple" form, both slots)
// =====================================================================================================
template <int NORM, bool VEC>
__global__ __launch_bounds__(256) void transh_spo_kernel(Operand S, Operand R, Operand O, int d, long long n,
                                                         float* __restrict__ out) {
  const int lg = threadIdx.x & 7;
  long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool valid = row < n;
  if (!valid) row = n - 1;  // (all lanes of a wave take part in the group shuffles)
  const float* s = (const float*)S.base + index_at(S.idx, row) * S.ld;
  const float* r = (const float*)R.base + index_at(R.idx, row) * R.ld;
  const float* o = (const float*)O.base + index_at(O.idx, row) * O.ld;
  const float den = th_den(th_group_nw2<VEC>(r + d, d, lg));
  const float a_s = th_group_dot<VEC>(r + d, den, s, d, lg);
  const float c_o = th_group_dot<VEC>(r + d, den, o, d, lg);
  const float sc = th_group_score<NORM, VEC>(s, r, r + d, o, den, a_s, c_o, d, lg);
  if (valid && lg == 0) out[row] = sc;
}

// grid.x = positive i, grid.y strides the groups over its K negatives
template <int NORM, bool VEC>
__global__ __launch_bounds__(256) void transh_neg_kernel(Operand S, Operand R, Operand O, int d, int slot,
                                                         const void* neg, int neg_itype, long long neg_ld, long long K,
                                                         float* __restrict__ out, long long ldo) {
  const int lg = threadIdx.x & 7;
  const int gid = threadIdx.x >> 3;
  const long long i = blockIdx.x;
  const float* ent = (const float*)S.base;
  const float* s = ent + index_at(S.idx, i) * S.ld;
  const float* o = ent + index_at(O.idx, i) * O.ld;
  const float* r = (const float*)R.base + index_at(R.idx, i) * R.ld;
  const Index nix = {neg, 1, neg_itype};
  // once per run of negatives: ||w|| and the coefficient of the row that stays
  const float den = th_den(th_group_nw2<VEC>(r + d, d, lg));
  const float keep = th_group_dot<VEC>(r + d, den, slot == 0 ? o : s, d, lg);
  const long long step = (long long)gridDim.y * 32;
  for (long long k = (long long)blockIdx.y * 32 + gid; k < K; k += step) {
    const float* x = ent + index_at(nix, i * neg_ld + k) * S.ld;
    const float var = th_group_dot<VEC>(r + d, den, x, d, lg);
    float sc;
    if (slot == 0) sc = th_group_score<NORM, VEC>(x, r, r + d, o, den, var, keep, d, lg);
    else sc = th_group_score<NORM, VEC>(s, r, r + d, x, den, keep, var, d, lg);
    if (lg == 0) out[i * ldo + k] = sc;
  }
}

int run_transh_spo(bool neg_mode, const Operand& S, const Operand& R, const Operand& O, int d, long long n, int slot,
                   const void* neg, int neg_itype, long long neg_ld, long long K, float lp, float* out, long long ldo,
                   hipStream_t st) {
  if (n == 0 || (neg_mode && K == 0)) return KGE_OK;
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || d > 1024) return KGE_ERR_UNSUPPORTED;
  const bool vec = th_vec_ok(d, S, R, O);
  if (!neg_mode) {
    const dim3 grid((unsigned)((n + 31) / 32));
#define KGE_TH_GO(NORM, VEC) \
  hipLaunchKernelGGL((transh_spo_kernel<NORM, VEC>), grid, dim3(256), 0, st, S, R, O, d, n, out)
    if (norm == NORM_L1) {
      if (vec) KGE_TH_GO(NORM_L1, true); else KGE_TH_GO(NORM_L1, false);
    } else {
      if (vec) KGE_TH_GO(NORM_L2, true); else KGE_TH_GO(NORM_L2, false);
    }
#undef KGE_TH_GO
  } else {
    // 16 negatives per group where that still leaves ~2048 workgroups, 4 otherwise
    long long per = 16;
    while (per > 4 && n * ((K + 32 * per - 1) / (32 * per)) < 2048) per >>= 1;
    long long by = (K + 32 * per - 1) / (32 * per);
    if (by < 1) by = 1;
    if (by > 64) by = 64;
    const dim3 grid((unsigned)n, (unsigned)by);
#define KGE_TH_GO(NORM, VEC)                                                                                        \
  hipLaunchKernelGGL((transh_neg_kernel<NORM, VEC>), grid, dim3(256), 0, st, S, R, O, d, slot, neg, neg_itype, neg_ld, \
                     K, out, ldo)
    if (norm == NORM_L1) {
      if (vec) KGE_TH_GO(NORM_L1, true); else KGE_TH_GO(NORM_L1, false);
    } else {
      if (vec) KGE_TH_GO(NORM_L2, true); else KGE_TH_GO(NORM_L2, false);
    }
#undef KGE_TH_GO
  }
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// =====================================================================================================
// backward
// =====================================================================================================
// With u = d score / d v (L1: -sign(v), sign(0) = 0; L2: -v / ||v||, 0 where ||v|| = 0), U = gout * u and
// P = I - w^ w^T, the triple form v = (P s + d_r) - P o + eps gives
//   g_s = P U,  g_d = U,  g_o = -P U,  g_w^ = (w^.o - w^.s) U + (w^.U) (o - s),
//   g_w = (g_w^ - (w^.g_w^) w^) / ||w||  where ||w|| >= 1e-12,  g_w^ / 1e-12  otherwise;
// the _po form v = (P o - d_r) - P s + eps has s and o swapped and g_d = -U.
// A wave keeps one row e that stays (its w^, its coefficient al_e = w^.e) and walks the rows x_j that vary
// (al_j = w^.x_j); with A = sum U_j, B = sum (w^.U_j) x_j, C = sum al_j U_j, beta = sum w^.U_j and sg = +1 where the
// varying row is the subtracted one (sp_, _po, spo, neg slot 2), -1 for neg slot 0:
//   g_e = sg P A,   g_x_j = -sg P U_j,   g_w^ = sg ((C + B) - al_e A - beta e),   g_d = +-A.
__device__ __forceinline__ float th_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}

struct ThBwd {
  Operand E, R, X;       // the row that stays, the relation row, the rows that vary (X.idx by j, or by i when by_row)
  const void* neg;       // != NULL: x_j = entity neg[i * neg_ld + j] (X.base = the entity table)
  int neg_itype;
  long long neg_ld;
  int x_by_row;          // neg == NULL: 1 = one varying row per row i, X.idx[i] (spo); 0 = X.idx[j] (pairs)
  int form;              // 0: fixed from e, v = fma(al_j, w^, fixed - x_j) + eps;  1: neg slot 0, fixed from x_j
  int dsign;             // form 0: +1 (sp_ / spo / neg slot 2), -1 (_po)
  int d;
  long long n, K;
  int chunk;             // varying rows per wave (K: one wave per row)
  const float* gout;
  long long ldg;
  float* ge; long long ge_ld;   // gradient rows of e / of the relation row: row i, or the table row where by_id
  float* gr; long long gr_ld;
  float* gx; long long gx_ld;   // gradient of the varying rows, or NULL (pairs: transh_bwd_tgt_kernel's)
  int by_id;             // 1: float atomics into table gradients;  0: plain stores to row i
};

template <int NORM, int RR>
__device__ __forceinline__ void th_pair_u(const float (&fixed)[RR], const float (&wh)[RR], const float (&x)[RR],
                                          float al, float g, int d, int lane, float (&U)[RR], float& wu) {
  float v[RR];
  float ss = 0.0f;
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    v[r] = (lane + 64 * r < d) ? th_v(fixed[r], x[r], al, wh[r]) : 0.0f;
    ss = __builtin_fmaf(v[r], v[r], ss);
  }
  float nv = 1.0f;
  if (NORM == NORM_L2) nv = sqrt_rn(th_wave_sum(ss));
  float p = 0.0f;
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    float u;
    if (NORM == NORM_L1) u = v[r] > 0.0f ? -1.0f : (v[r] < 0.0f ? 1.0f : 0.0f);
    else u = nv > 0.0f ? -(v[r] / nv) : 0.0f;
    U[r] = g * u;
    p = __builtin_fmaf(wh[r], U[r], p);
  }
  wu = th_wave_sum(p);
}

template <int RR>
__device__ __forceinline__ void th_load_row(const float* row, int d, int lane, float (&x)[RR]) {
#pragma unroll
  for (int r = 0; r < RR; ++r) x[r] = (lane + 64 * r < d) ? row[lane + 64 * r] : 0.0f;
}
template <int RR>
__device__ __forceinline__ float th_wave_dot(const float (&a)[RR], const float (&b)[RR]) {
  float p = 0.0f;
#pragma unroll
  for (int r = 0; r < RR; ++r) p = __builtin_fmaf(a[r], b[r], p);
  return th_wave_sum(p);
}

template <int NORM, int RR>
__global__ __launch_bounds__(64) void transh_bwd_rows_kernel(ThBwd a) {
  const int lane = threadIdx.x, d = a.d;
  const long long i = blockIdx.x;
  const long long j0 = (long long)blockIdx.y * a.chunk;
  const long long j1 = j0 + a.chunk < a.K ? j0 + a.chunk : a.K;
  const long long id_e = index_at(a.E.idx, i), id_r = index_at(a.R.idx, i);
  const float* rrow = (const float*)a.R.base + id_r * a.R.ld;
  float e[RR], dr[RR], wh[RR], fixed[RR];
  th_load_row<RR>((const float*)a.E.base + id_e * a.E.ld, d, lane, e);
  th_load_row<RR>(rrow, d, lane, dr);
  th_load_row<RR>(rrow + d, d, lane, wh);
  const float nrm = sqrt_rn(th_wave_dot<RR>(wh, wh));
  const float den = __builtin_fmaxf(nrm, TH_NORM_EPS);
#pragma unroll
  for (int r = 0; r < RR; ++r) wh[r] = th_what(wh[r], den);
  const float al_e = th_wave_dot<RR>(wh, e);
#pragma unroll
  for (int r = 0; r < RR; ++r)
    fixed[r] = a.form == 0 ? (a.dsign > 0 ? th_fixed<1>(e[r], wh[r], al_e, dr[r]) : th_fixed<-1>(e[r], wh[r], al_e, dr[r]))
                           : e[r];
  const float sg = a.form == 0 ? 1.0f : -1.0f;
  float A[RR], B[RR], C[RR], x[RR], U[RR];
  float beta = 0.0f;
#pragma unroll
  for (int r = 0; r < RR; ++r) A[r] = B[r] = C[r] = 0.0f;
  const Index nix = {a.neg, 1, a.neg_itype};
  for (long long j = j0; j < j1; ++j) {
    long long id_x;
    if (a.neg != nullptr) id_x = index_at(nix, i * a.neg_ld + j);
    else id_x = index_at(a.X.idx, a.x_by_row ? i : j);
    th_load_row<RR>((const float*)a.X.base + id_x * a.X.ld, d, lane, x);
    const float al_x = th_wave_dot<RR>(wh, x);
    const float g = a.gout[i * a.ldg + j];
    float wu;
    if (a.form == 0) {
      th_pair_u<NORM, RR>(fixed, wh, x, al_x, g, d, lane, U, wu);
    } else {  // neg slot 0: the fixed side comes from the varying row, the row that stays is subtracted
      float fx[RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) fx[r] = th_fixed<1>(x[r], wh[r], al_x, dr[r]);
      th_pair_u<NORM, RR>(fx, wh, e, al_e, g, d, lane, U, wu);
    }
    beta += wu;
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      A[r] += U[r];
      B[r] = __builtin_fmaf(wu, x[r], B[r]);
      C[r] = __builtin_fmaf(al_x, U[r], C[r]);
    }
    if (a.gx != nullptr) {
      float* gx = a.gx + (a.by_id ? id_x : i) * a.gx_ld;
#pragma unroll
      for (int r = 0; r < RR; ++r)
        if (lane + 64 * r < d) {
          const float val = -sg * (U[r] - wu * wh[r]);
          if (a.by_id) atomicAdd(gx + lane + 64 * r, val);
          else gx[lane + 64 * r] = val;
        }
    }
  }
  const float wA = th_wave_dot<RR>(wh, A);
  float gwh[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) gwh[r] = sg * ((C[r] + B[r]) - al_e * A[r] - beta * e[r]);
  const float wg = th_wave_dot<RR>(wh, gwh);
  float* ge = a.ge + (a.by_id ? id_e : i) * a.ge_ld;
  float* gr = a.gr + (a.by_id ? id_r : i) * a.gr_ld;
  const float dsg = a.form == 0 && a.dsign < 0 ? -1.0f : 1.0f;
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const int k = lane + 64 * r;
    if (k < d) {
      const float v_e = sg * (A[r] - wA * wh[r]);
      const float v_d = dsg * A[r];
      const float v_w = nrm >= TH_NORM_EPS ? (gwh[r] - wg * wh[r]) / nrm : gwh[r] / TH_NORM_EPS;
      if (a.by_id) {
        atomicAdd(ge + k, v_e);
        atomicAdd(gr + k, v_d);
        atomicAdd(gr + d + k, v_w);
      } else {
        ge[k] = v_e;
        gr[k] = v_d;
        gr[d + k] = v_w;
      }
    }
  }
}

// kge_score_pairs_bwd, stage 0: (fixed_i, w^_i) of every query row, parked in the outputs the last stage overwrites
// (fixed in g_a[i, :], w^ in g_p[i, d:2d])
template <int RR>
__global__ __launch_bounds__(64) void transh_bwd_build_kernel(Operand E, Operand R, int dsign, int d, float* g_a,
                                                              float* g_p) {
  const int lane = threadIdx.x;
  const long long i = blockIdx.x;
  const float* rrow = (const float*)R.base + index_at(R.idx, i) * R.ld;
  float e[RR], dr[RR], wh[RR];
  th_load_row<RR>((const float*)E.base + index_at(E.idx, i) * E.ld, d, lane, e);
  th_load_row<RR>(rrow, d, lane, dr);
  th_load_row<RR>(rrow + d, d, lane, wh);
  const float den = __builtin_fmaxf(sqrt_rn(th_wave_dot<RR>(wh, wh)), TH_NORM_EPS);
#pragma unroll
  for (int r = 0; r < RR; ++r) wh[r] = th_what(wh[r], den);
  const float al_e = th_wave_dot<RR>(wh, e);
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const int k = lane + 64 * r;
    if (k < d) {
      g_a[i * d + k] = dsign > 0 ? th_fixed<1>(e[r], wh[r], al_e, dr[r]) : th_fixed<-1>(e[r], wh[r], al_e, dr[r]);
      g_p[i * 2 * d + d + k] = wh[r];
    }
  }
}

// stage 1: a wave per target row j sums -P_i U_ij over the query rows i = 0, 1, ..., n - 1 (that order)
template <int NORM, int RR>
__global__ __launch_bounds__(64) void transh_bwd_tgt_kernel(Operand TG, int d, long long n, const float* __restrict__ gout,
                                                            long long ldg, const float* __restrict__ fixed_rows,
                                                            const float* __restrict__ wh_rows, float* __restrict__ g_tgt) {
  const int lane = threadIdx.x;
  const long long j = blockIdx.x;
  float x[RR], acc[RR], fixed[RR], wh[RR], U[RR];
  th_load_row<RR>((const float*)TG.base + index_at(TG.idx, j) * TG.ld, d, lane, x);
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = 0.0f;
  for (long long i = 0; i < n; ++i) {
    th_load_row<RR>(fixed_rows + i * d, d, lane, fixed);
    th_load_row<RR>(wh_rows + i * 2 * d + d, d, lane, wh);
    const float al_x = th_wave_dot<RR>(wh, x);
    float wu;
    th_pair_u<NORM, RR>(fixed, wh, x, al_x, gout[i * ldg + j], d, lane, U, wu);
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] -= U[r] - wu * wh[r];
  }
#pragma unroll
  for (int r = 0; r < RR; ++r)
    if (lane + 64 * r < d) g_tgt[j * d + lane + 64 * r] = acc[r];
}

static int th_rr(int d) {
  int rr = 1;
  while (rr * 64 < d) rr <<= 1;
  return rr;
}

template <int NORM>
static int th_launch_rows(const ThBwd& a, hipStream_t st) {
  const dim3 grid((unsigned)a.n, (unsigned)((a.K + a.chunk - 1) / a.chunk));
  switch (th_rr(a.d)) {
#define KGE_TH_CASE(RRV) \
  case RRV: hipLaunchKernelGGL((transh_bwd_rows_kernel<NORM, RRV>), grid, dim3(64), 0, st, a); break;
    KGE_TH_CASE(1) KGE_TH_CASE(2) KGE_TH_CASE(4) KGE_TH_CASE(8) KGE_TH_CASE(16)
#undef KGE_TH_CASE
    default: return KGE_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}
static int th_run_rows(const ThBwd& a, float lp, hipStream_t st) {
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || a.d > 1024) return KGE_ERR_UNSUPPORTED;
  if (a.n == 0 || a.K == 0) return KGE_OK;
  if ((a.K + a.chunk - 1) / a.chunk > 65535) return KGE_ERR_UNSUPPORTED;
  return norm == NORM_L1 ? th_launch_rows<NORM_L1>(a, st) : th_launch_rows<NORM_L2>(a, st);
}

template <int NORM>
static int th_launch_pairs_bwd(const Operand& A, const Operand& R, const Operand& TG, int dsign, int d, long long n,
                               long long m, const float* gout, long long ldg, float* g_a, float* g_p, float* g_tgt,
                               hipStream_t st) {
  switch (th_rr(d)) {
#define KGE_TH_CASE(RRV)                                                                                          \
  case RRV:                                                                                                       \
    hipLaunchKernelGGL((transh_bwd_build_kernel<RRV>), dim3((unsigned)n), dim3(64), 0, st, A, R, dsign, d, g_a, g_p); \
    hipLaunchKernelGGL((transh_bwd_tgt_kernel<NORM, RRV>), dim3((unsigned)m), dim3(64), 0, st, TG, d, n, gout, ldg, \
                       (const float*)g_a, (const float*)g_p, g_tgt);                                              \
    break;
    KGE_TH_CASE(1) KGE_TH_CASE(2) KGE_TH_CASE(4) KGE_TH_CASE(8) KGE_TH_CASE(16)
#undef KGE_TH_CASE
    default: return KGE_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// n > 0 and m > 0 (the empty sides are the caller's)
int run_transh_pairs_bwd(float lp, int dir, const Operand& A, const Operand& R, const Operand& TG, int d, long long n,
                         long long m, const float* gout, long long ldg, float* g_a, float* g_p, float* g_tgt,
                         hipStream_t st) {
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || d > 1024) return KGE_ERR_UNSUPPORTED;
  const int dsign = dir == KGE_SP_ ? 1 : -1;
  const int rc = norm == NORM_L1 ? th_launch_pairs_bwd<NORM_L1>(A, R, TG, dsign, d, n, m, gout, ldg, g_a, g_p, g_tgt, st)
                                 : th_launch_pairs_bwd<NORM_L2>(A, R, TG, dsign, d, n, m, gout, ldg, g_a, g_p, g_tgt, st);
  if (rc) return rc;
  ThBwd a = {};
  a.E = A; a.R = R; a.X = TG;
  a.form = 0; a.dsign = dsign; a.d = d; a.n = n; a.K = m;
  a.chunk = (int)(m < (1LL << 30) ? m : (1LL << 30));  // one wave per query row: plain stores, a fixed order
  if (m >= (1LL << 30)) return KGE_ERR_UNSUPPORTED;
  a.gout = gout; a.ldg = ldg;
  a.ge = g_a; a.ge_ld = d; a.gr = g_p; a.gr_ld = 2 * d;
  return th_run_rows(a, lp, st);
}

// kge_score_spo_bwd (accum == false: g_s / g_p / g_o rows) and kge_score_spo_bwd_accum (table gradients)
int run_transh_spo_bwd(float lp, const Operand& S, const Operand& R, const Operand& O, int d, long long n,
                       const float* gout, bool accum, float* g_s, long long g_s_ld, float* g_p, long long g_p_ld,
                       float* g_o, long long g_o_ld, hipStream_t st) {
  ThBwd a = {};
  a.E = S; a.R = R; a.X = O;
  a.x_by_row = 1; a.form = 0; a.dsign = 1; a.d = d; a.n = n; a.K = 1; a.chunk = 1;
  a.gout = gout; a.ldg = 1;
  a.ge = g_s; a.ge_ld = g_s_ld; a.gr = g_p; a.gr_ld = g_p_ld; a.gx = g_o; a.gx_ld = g_o_ld;
  a.by_id = accum ? 1 : 0;
  return th_run_rows(a, lp, st);
}

int run_transh_neg_bwd_accum(float lp, const Operand& S, const Operand& R, const Operand& O, int d, long long n, int slot,
                             const void* neg, int neg_itype, long long neg_ld, long long K, const float* gout,
                             long long ldg, float* ge, long long ge_ld, float* gr, long long gr_ld, hipStream_t st) {
  ThBwd a = {};
  a.E = slot == 0 ? O : S; a.R = R; a.X = S;  // X.base = the entity table
  a.neg = neg; a.neg_itype = neg_itype; a.neg_ld = neg_ld;
  a.form = slot == 0 ? 1 : 0; a.dsign = 1; a.d = d; a.n = n; a.K = K;
  a.chunk = 32;  // a positive's own gradients are summed in registers over 32 negatives, then one atomic row flush
  a.gout = gout; a.ldg = ldg;
  a.ge = ge; a.ge_ld = ge_ld; a.gr = gr; a.gr_ld = gr_ld; a.gx = ge; a.gx_ld = ge_ld;
  a.by_id = 1;
  return th_run_rows(a, lp, st);
}

}  // namespace kge
