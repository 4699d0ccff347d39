// rescal.hip -- RESCAL (kge/model/rescal.py) on gfx950: float32 tables, the relation row a d x d mixing matrix
// (rescal_device.hpp).
//
// score(s, p, o) = s^T M_p o.  Every entry first contracts M_p with the row that stays -- q = M_p^T s (sp_) or
// q = M_p o (_po), the only d^2 work -- and then scores q against the rows that vary, which is DistMult's arithmetic
// with a relation row of ones:
//
//   rescal_queries_kernel  kge_rescal_queries and the first stage of kge_score_sp / _po / _sp_po.  A workgroup per
//                          query: the entity row goes to LDS, M_p is read once, coalesced along its contiguous axis
//                          in both directions (rs_matvec_t runs down the columns, rs_matvec reduces a row across an
//                          8-lane group), no atomics.  The second stage is the float32 pair kernel of
//                          score_pairs_f32.hip on the dense q rows (api.hip) -- not copied here.
//   rescal_rows_kernel     kge_score_spo / kge_score_neg: a workgroup per triple / positive builds q in LDS and its
//                          lane groups take the row-wise dots (rs_row_dot: score_spo.hip's summation); q never goes
//                          to memory.  kge_score_neg builds q once per positive, for both slots.
//   rescal_bwd_kernel      g_q = sum_j gout_ij x_j (summed in registers over the rows that vary; kge_score_pairs_bwd
//                          gets it from the float32 gradient products of bwd_gemm32.hip instead), then ONE mat-vec
//                          g_e = M g_q / M^T g_q and ONE outer product e (x) g_q / g_q (x) e per row and chunk.
//                          Plain stores (kge_score_pairs_bwd, kge_score_spo_bwd) or float atomics into the tables'
//                          gradients (the _accum entries).
#include "rescal_device.hpp"
#include "spo_device.hpp"

namespace kge {

// bwd_gemm32.hip: C[M, N] = A * B on the f32 matrix cores
bool run_gemm32(bool a_kcont, int in16, long long M, long long N, long long K, const void* A, long long lda,
                const void* B, long long ldb, float* C, long long ldc, float* scratch, size_t scratch_bytes,
                hipStream_t st, int* parts = nullptr);

// rows of M_p readable in aligned groups of four columns
static bool rs_vec_ok(int d, const Operand& R) { return d % 4 == 0 && aligned16(R.base) && R.ld % 4 == 0; }
// rows of the entity table readable in aligned chunks of eight coordinates
static bool rs_vec8_ok(int d, const Operand& E) { return d % 8 == 0 && aligned16(E.base) && E.ld % 4 == 0; }

__device__ __forceinline__ void rs_load_row(const float* __restrict__ row, int d, float* dst) {
  for (int c = threadIdx.x; c < d; c += RS_THREADS) dst[c] = row[c];
}

// =====================================================================================================
// forward
// =====================================================================================================
// grid.x = query i; grid.y == 2: the second block of a two-sided call (rows A2, _po form, q2).  `ones` (may be NULL):
// d floats set to 1 on the way -- the relation row of the second stage.
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void rescal_queries_kernel(Operand A, Operand A2, Operand R, int dir, int d,
                                                                    float* __restrict__ q, float* __restrict__ q2,
                                                                    long long q_ld, float* __restrict__ ones) {
  __shared__ __attribute__((aligned(16))) float sX[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sQ[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sPart[8 * RS_LDV];
  const long long i = blockIdx.x;
  if (blockIdx.y == 1) {
    A = A2;
    dir = KGE_PO_;
    q = q2;
  } else if (ones != nullptr && i == 0) {
    for (int c = threadIdx.x; c < d; c += RS_THREADS) ones[c] = 1.0f;
  }
  const float* M = (const float*)R.base + index_at(R.idx, i) * R.ld;
  rs_load_row((const float*)A.base + index_at(A.idx, i) * A.ld, d, sX);
  __syncthreads();
  if (dir == KGE_SP_) rs_matvec_t<VEC>(M, sX, d, sPart, sQ);
  else rs_matvec<VEC>(M, sX, d, sQ);
  for (int c = threadIdx.x; c < d; c += RS_THREADS) q[i * q_ld + c] = sQ[c];
}

int run_rescal_queries(const Operand& A, const Operand* A2, const Operand& R, int dir, int d, long long n, float* q,
                       float* q2, long long q_ld, float* ones, hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (d > RS_MAX_DIM || n > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)n, A2 != nullptr ? 2u : 1u);
  const Operand B = A2 != nullptr ? *A2 : A;
  if (rs_vec_ok(d, R))
    hipLaunchKernelGGL((rescal_queries_kernel<true>), grid, dim3(RS_THREADS), 0, st, A, B, R, dir, d, q, q2, q_ld, ones);
  else
    hipLaunchKernelGGL((rescal_queries_kernel<false>), grid, dim3(RS_THREADS), 0, st, A, B, R, dir, d, q, q2, q_ld, ones);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// kge_score_spo (neg == NULL, K = 1: x = row O.idx[i], out[i]) and kge_score_neg (x = entity neg[i, k], out[i, k]).
// slot 2: q = M^T s_i against the objects; slot 0: q = M o_i against the subjects.  grid.y strides the groups over K.
// G = group_size(d): the lanes of a row's group, as score_spo.hip chooses them.
template <bool VEC, bool VEC8>
__global__ __launch_bounds__(RS_THREADS) void rescal_rows_kernel(Operand S, Operand R, Operand O, int d, int slot,
                                                                 const void* neg, int neg_itype, long long neg_ld,
                                                                 long long K, int G, float* __restrict__ out,
                                                                 long long ldo) {
  __shared__ __attribute__((aligned(16))) float sX[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sQ[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sPart[8 * RS_LDV];
  const long long i = blockIdx.x;
  const float* M = (const float*)R.base + index_at(R.idx, i) * R.ld;
  const Operand& E = slot == 0 ? O : S;
  rs_load_row((const float*)E.base + index_at(E.idx, i) * E.ld, d, sX);
  __syncthreads();
  if (slot == 0) rs_matvec<VEC>(M, sX, d, sQ);
  else rs_matvec_t<VEC>(M, sX, d, sPart, sQ);
  const int lg = threadIdx.x & (G - 1), gid = threadIdx.x / G, groups = RS_THREADS / G;
  const Index nix = {neg, 1, neg_itype};
  const long long step = (long long)gridDim.y * groups;
  for (long long k = (long long)blockIdx.y * groups + gid; k < K; k += step) {
    const float* x;
    if (neg != nullptr) x = (const float*)S.base + index_at(nix, i * neg_ld + k) * S.ld;  // S.base == the entity table
    else x = (const float*)O.base + index_at(O.idx, i) * O.ld;
    const float P = rs_row_dot<VEC8>(sQ, x, d, lg, G);
    if (lg == 0) out[neg != nullptr ? i * ldo + k : i] = P;
  }
}

int run_rescal_rows(bool neg_mode, const Operand& S, const Operand& R, const Operand& O, int d, long long n, int slot,
                    const void* neg, int neg_itype, long long neg_ld, long long K, float* out, long long ldo,
                    hipStream_t st) {
  if (n == 0 || (neg_mode && K == 0)) return KGE_OK;
  if (d > RS_MAX_DIM || n > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  if (!neg_mode) {
    K = 1;
    neg = nullptr;
    slot = 2;
  }
  // every workgroup of a positive builds its query again: split K only while the grid is small
  const int G = group_size(d);
  const long long groups = RS_THREADS / G;
  long long by = (K + groups * 8 - 1) / (groups * 8);
  if (by > 1024 / n) by = 1024 / n;
  if (by > 64) by = 64;
  if (by < 1) by = 1;
  const dim3 grid((unsigned)n, (unsigned)by);
  const bool vec = rs_vec_ok(d, R), vec8 = rs_vec8_ok(d, S);
#define KGE_RS_GO(V, V8)                                                                                              \
  hipLaunchKernelGGL((rescal_rows_kernel<V, V8>), grid, dim3(RS_THREADS), 0, st, S, R, O, d, slot, neg, neg_itype, neg_ld, \
                     K, G, out, ldo)
  if (vec) {
    if (vec8) KGE_RS_GO(true, true); else KGE_RS_GO(true, false);
  } else {
    if (vec8) KGE_RS_GO(false, true); else KGE_RS_GO(false, false);
  }
#undef KGE_RS_GO
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// =====================================================================================================
// backward
// =====================================================================================================
// With q the query of the row e that stays, x_j the rows that vary and g_j = gout[i, j]:
//   g_x_j = g_j q          g_q = sum_j g_j x_j
//   sp_ form (q = M^T e):  g_e = M g_q,    g_M[a][b] = e_a g_q_b
//   _po form (q = M e):    g_e = M^T g_q,  g_M[a][b] = g_q_a e_b
constexpr int RS_NEG_CHUNK = 256;  // rows that vary per workgroup: g_q is summed over them in a register

struct RsBwd {
  Operand E, R, X;      // the row that stays, the relation row, the rows that vary
  const void* neg;      // != NULL: x_j = entity neg[i * neg_ld + j] (X.base = the entity table); NULL: x = row X.idx[i]
  int neg_itype;
  long long neg_ld;
  const float* gq;      // != NULL: g_q rows [n, d] are given (kge_score_pairs_bwd); nothing varies here
  int dir;              // KGE_SP_ / KGE_PO_: the form of q
  int d;
  long long K;
  int chunk;
  const float* gout;
  long long ldg;
  float* ge; long long ge_ld;   // gradient rows of e / of the relation row: row i, or the table row where by_id
  float* gr; long long gr_ld;
  float* gx; long long gx_ld;   // gradient of the varying rows
  int by_id;            // 1: float atomics into table gradients;  0: plain stores to row i
};

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void rescal_bwd_kernel(RsBwd a) {
  __shared__ __attribute__((aligned(16))) float sX[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sQ[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sG[RS_LDV];
  __shared__ __attribute__((aligned(16))) float sPart[8 * RS_LDV];
  const int d = a.d, tid = threadIdx.x;
  const long long i = blockIdx.x;
  const long long id_e = index_at(a.E.idx, i), id_r = index_at(a.R.idx, i);
  const float* M = (const float*)a.R.base + id_r * a.R.ld;
  rs_load_row((const float*)a.E.base + id_e * a.E.ld, d, sX);
  if (a.gq != nullptr) {
    rs_load_row(a.gq + i * d, d, sG);
    __syncthreads();
  } else {
    __syncthreads();
    if (a.dir == KGE_SP_) rs_matvec_t<VEC>(M, sX, d, sPart, sQ);
    else rs_matvec<VEC>(M, sX, d, sQ);
    const long long j0 = (long long)blockIdx.y * a.chunk;
    const long long j1 = j0 + a.chunk < a.K ? j0 + a.chunk : a.K;
    const Index nix = {a.neg, 1, a.neg_itype};
    if (tid < d) {  // (d <= 256: one coordinate per thread)
      const float qc = sQ[tid];
      float acc = 0.0f;
      for (long long j = j0; j < j1; ++j) {
        const long long id_x = a.neg != nullptr ? index_at(nix, i * a.neg_ld + j) : index_at(a.X.idx, i);
        const float g = a.gout[i * a.ldg + j];
        acc = __builtin_fmaf(g, ((const float*)a.X.base + id_x * a.X.ld)[tid], acc);
        const float val = g * qc;
        if (a.by_id) atomicAdd(a.gx + id_x * a.gx_ld + tid, val);
        else a.gx[i * a.gx_ld + tid] = val;
      }
      sG[tid] = acc;
    }
    __syncthreads();
  }
  // one mat-vec and one outer product per row and chunk
  if (a.dir == KGE_SP_) rs_matvec<VEC>(M, sG, d, sQ);
  else rs_matvec_t<VEC>(M, sG, d, sPart, sQ);
  if (tid < d) {
    if (a.by_id) atomicAdd(a.ge + id_e * a.ge_ld + tid, sQ[tid]);
    else a.ge[i * a.ge_ld + tid] = sQ[tid];
  }
  float* gr = a.gr + (a.by_id ? id_r : i) * a.gr_ld;
  const float* left = a.dir == KGE_SP_ ? sX : sG;
  const float* right = a.dir == KGE_SP_ ? sG : sX;
  int ra = 0, cb = tid;  // (row, column) of element tid of the d x d gradient, advanced without a division
  while (cb >= d) {
    cb -= d;
    ++ra;
  }
  const int dr = RS_THREADS / d, dc = RS_THREADS - dr * d;
  for (; ra < d;) {
    const float val = left[ra] * right[cb];
    if (a.by_id) atomicAdd(gr + ra * d + cb, val);
    else gr[ra * d + cb] = val;
    ra += dr;
    cb += dc;
    if (cb >= d) {
      cb -= d;
      ++ra;
    }
  }
}

static int rs_launch_bwd(const RsBwd& a, long long n, hipStream_t st) {
  if (a.d > RS_MAX_DIM || n > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  const long long by = a.gq != nullptr ? 1 : (a.K + a.chunk - 1) / a.chunk;
  if (n == 0 || by == 0) return KGE_OK;
  if (by > 65535) return KGE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)n, (unsigned)by);
  if (rs_vec_ok(a.d, a.R)) hipLaunchKernelGGL((rescal_bwd_kernel<true>), grid, dim3(RS_THREADS), 0, st, a);
  else hipLaunchKernelGGL((rescal_bwd_kernel<false>), grid, dim3(RS_THREADS), 0, st, a);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// out[j, :] = table row TG.idx[j] (listed targets), ld = d
__global__ __launch_bounds__(256) void rescal_gather_kernel(Operand TG, int d, long long m, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long j = t / d;
  const int c = (int)(t - j * d);
  if (j >= m) return;
  out[j * d + c] = ((const float*)TG.base + index_at(TG.idx, j) * TG.ld)[c];
}

long long rescal_pairs_bwd_workspace_bytes(int d, long long n) { return 2 * n * d * (long long)sizeof(float); }

// kge_score_pairs_bwd, n > 0 and m > 0.  Workspace: Q [n, d] | g_Q [n, d].  The two products are bwd_gemm.hip's:
// g_Q = G T (split-K partials in g_tgt while the targets are the table itself; listed targets are gathered into g_tgt
// first), g_tgt = G^T Q.  No float atomics anywhere: every output has one owner and a fixed order.
int run_rescal_pairs_bwd(int dir, const Operand& A, const Operand& R, const Operand& TG, int d, long long n, long long m,
                         const float* gout, long long ldg, float* g_a, float* g_p, float* g_tgt, void* ws,
                         long long ws_bytes, hipStream_t st) {
  if (d > RS_MAX_DIM) return KGE_ERR_UNSUPPORTED;
  if (ws == nullptr || ws_bytes < rescal_pairs_bwd_workspace_bytes(d, n)) return KGE_ERR_WORKSPACE;
  if (n >= (1LL << 31) || m >= (1LL << 31) || ldg >= (1LL << 31) || TG.ld >= (1LL << 31)) return KGE_ERR_UNSUPPORTED;
  float* Q = (float*)ws;
  float* GQ = Q + n * d;
  int rc = run_rescal_queries(A, nullptr, R, dir, d, n, Q, nullptr, d, nullptr, st);
  if (rc != KGE_OK) return rc;
  const float* T = (const float*)TG.base;
  long long ldt = TG.ld;
  if (TG.idx.ptr != nullptr) {
    if ((m * d + 255) / 256 > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(rescal_gather_kernel, dim3((unsigned)((m * d + 255) / 256)), dim3(256), 0, st, TG, d, m, g_tgt);
    if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
    T = g_tgt;
    ldt = d;
  }
  float* scratch = TG.idx.ptr == nullptr ? g_tgt : nullptr;
  const size_t scratch_bytes = TG.idx.ptr == nullptr ? (size_t)m * d * sizeof(float) : 0;
  if (!run_gemm32(true, 0, n, d, m, gout, ldg, T, ldt, GQ, d, scratch, scratch_bytes, st)) return KGE_ERR_UNSUPPORTED;
  if (!run_gemm32(false, 0, m, d, n, gout, ldg, Q, d, g_tgt, d, nullptr, 0, st)) return KGE_ERR_UNSUPPORTED;
  RsBwd a = {};
  a.E = A; a.R = R; a.gq = GQ; a.dir = dir; a.d = d; a.K = 0; a.chunk = 1;
  a.ge = g_a; a.ge_ld = d; a.gr = g_p; a.gr_ld = (long long)d * d;
  return rs_launch_bwd(a, n, st);
}

// kge_score_spo_bwd (accum == false: g_s / g_p / g_o rows) and kge_score_spo_bwd_accum (table gradients)
int run_rescal_spo_bwd(const Operand& S, const Operand& R, const Operand& O, int d, long long n, const float* gout,
                       bool accum, float* g_s, long long g_s_ld, float* g_p, long long g_p_ld, float* g_o,
                       long long g_o_ld, hipStream_t st) {
  RsBwd a = {};
  a.E = S; a.R = R; a.X = O;
  a.dir = KGE_SP_; a.d = d; a.K = 1; a.chunk = 1;
  a.gout = gout; a.ldg = 1;
  a.ge = g_s; a.ge_ld = g_s_ld; a.gr = g_p; a.gr_ld = g_p_ld; a.gx = g_o; a.gx_ld = g_o_ld;
  a.by_id = accum ? 1 : 0;
  return rs_launch_bwd(a, n, st);
}

int run_rescal_neg_bwd_accum(const Operand& S, const Operand& R, const Operand& O, int d, long long n, int slot,
                             const void* neg, int neg_itype, long long neg_ld, long long K, const float* gout,
                             long long ldg, float* ge, long long ge_ld, float* gr, long long gr_ld, hipStream_t st) {
  RsBwd a = {};
  a.E = slot == 0 ? O : S; a.R = R; a.X = S;  // X.base = the entity table
  a.neg = neg; a.neg_itype = neg_itype; a.neg_ld = neg_ld;
  a.dir = slot == 0 ? KGE_PO_ : KGE_SP_; a.d = d; a.K = K; a.chunk = RS_NEG_CHUNK;
  a.gout = gout; a.ldg = ldg;
  a.ge = ge; a.ge_ld = ge_ld; a.gr = gr; a.gr_ld = gr_ld; a.gx = ge; a.gx_ld = ge_ld;
  a.by_id = 1;
  return rs_launch_bwd(a, n, st);
}

}  // namespace kge
