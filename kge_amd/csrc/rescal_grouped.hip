// rescal_grouped.hip -- RESCAL with the rows of a batch brought together by relation: the d^2 work of a relation runs
// as small matrix products on the f32 matrix cores, and the relation gradient has one owner per output tile
// (rescal_grouped_device.hpp holds the workspace and the tile geometry).  An opt-in route beside
// rescal.hip, whose kernels are untouched.
//
//   rsg_rank_kernel / rsg_groups_kernel   kge_rescal_group: the STABLE order of the batch by relation id and the
//                          groups' ranges, by counting -- every position counts the keys below it and the equal keys in
//                          front of it: no atomics, no host wait, the same arrays on every run.
//   rsg_queries_kernel     kge_rescal_queries_grouped: Q_p = S_p M_p (sp_) / O_p M_p^T (_po).  A workgroup owns a tile of
//                          16 rows of one group and 64 output columns; the tile's entity rows go to LDS once, M_p streams
//                          through LDS in panels of 32 k-rows, each wave accumulates one 16 x 16 tile with
//                          v_mfma_f32_16x16x4_f32.  The same kernel with the dense g_q rows as its left operand and float
//                          atomics as its epilogue is the fixed-row gradient g_S_p = Gq_p M_p^T / g_O_p = Gq_p M_p.
//   rsg_neg_kernel         per positive: g_q = sum_k gout_k x_k summed in registers (chunks of 256 samples staged in
//                          LDS), written as a dense row; gout_k q into grad_ent[neg_k] by float atomics.
//   rsg_relgrad_kernel     per (relation group, 64 x 64 block of the d x d gradient): g_M_p = S_p^T Gq_p (slot 2) /
//                          Gq_p^T O_p (slot 0) over the group's rows in perm order on the MFMA, then ONE plain
//                          load-add-store into grad_rel[p] -- no float atomics, the same bits on every run.
#include "rescal_grouped_device.hpp"

namespace kge {

// =====================================================================================================
// grouping
// =====================================================================================================
// Position i counts, over the whole batch: the keys below its own (less), the equal keys (cnt) and the equal keys in
// front of it (eqb).  perm[less + eqb] = i is the stable order; n^2 / 256 broadcast reads of LDS per thread.
__global__ __launch_bounds__(RG_THREADS) void rsg_rank_kernel(Index P, int n, RgWs w) {
  __shared__ int sK[RG_STAGE];
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  const int ki = i < n ? (int)index_at(P, i) : 0;
  int less = 0, eq = 0, eqb = 0;
  for (int j0 = 0; j0 < n; j0 += RG_STAGE) {
    __syncthreads();
    for (int j = threadIdx.x; j < RG_STAGE; j += RG_THREADS) sK[j] = j0 + j < n ? (int)index_at(P, j0 + j) : 0;
    __syncthreads();
    const int m = n - j0 < RG_STAGE ? n - j0 : RG_STAGE;
    for (int j = 0; j < m; ++j) {
      const int kj = sK[j];
      less += kj < ki ? 1 : 0;
      eq += kj == ki ? 1 : 0;
      eqb += (kj == ki && j0 + j < i) ? 1 : 0;
    }
  }
  if (i < n) {
    w.key[i] = ki;
    w.less[i] = less;
    w.cnt[i] = eq;
    w.eqb[i] = eqb;
    w.perm[less + eqb] = i;
  }
}

// The first position of every key (eqb == 0) stands for its group: it counts the groups below its key (its group
// number) and their row tiles (its first tile).  Position 0 writes the totals.
__global__ __launch_bounds__(RG_THREADS) void rsg_groups_kernel(int n, RgWs w) {
  __shared__ int sK[RG_STAGE], sT[RG_STAGE];  // key, and the row tiles of the group a FIRST position stands for (else 0)
  const int i = blockIdx.x * RG_THREADS + threadIdx.x;
  const int ki = i < n ? w.key[i] : 0;
  int g = 0, tiles = 0, G = 0, T = 0;
  for (int j0 = 0; j0 < n; j0 += RG_STAGE) {
    __syncthreads();
    for (int j = threadIdx.x; j < RG_STAGE; j += RG_THREADS) {
      const bool first = j0 + j < n && w.eqb[j0 + j] == 0;
      sK[j] = j0 + j < n ? w.key[j0 + j] : 0;
      sT[j] = first ? (w.cnt[j0 + j] + RG_TM - 1) / RG_TM : 0;
    }
    __syncthreads();
    const int m = n - j0 < RG_STAGE ? n - j0 : RG_STAGE;
    for (int j = 0; j < m; ++j) {
      const int tj = sT[j];  // >= 1 exactly at a first position
      G += tj > 0 ? 1 : 0;
      T += tj;
      if (tj > 0 && sK[j] < ki) {
        g += 1;
        tiles += tj;
      }
    }
  }
  if (i < n && w.eqb[i] == 0) {
    w.group_rel[g] = ki;
    w.group_begin[g] = w.less[i];
    w.tile_begin[g] = tiles;
  }
  if (i == 0) {
    w.counts[0] = G;
    w.counts[1] = T;
    w.group_begin[G] = n;
    w.tile_begin[G] = T;
  }
}

static int run_rescal_group(const Index& P, long long n, const RgWs& w, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + RG_THREADS - 1) / RG_THREADS);
  hipLaunchKernelGGL(rsg_rank_kernel, dim3(blocks), dim3(RG_THREADS), 0, st, P, (int)n, w);
  hipLaunchKernelGGL(rsg_groups_kernel, dim3(blocks), dim3(RG_THREADS), 0, st, (int)n, w);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

long long rescal_grouped_workspace_bytes(int d, long long n) { return rg_workspace_bytes(n, d); }

// kge_rescal_group, n > 0
int run_rescal_group_ws(const Index& P, long long n, int d, void* ws, hipStream_t st) {
  return run_rescal_group(P, n, rg_workspace(ws, n, d), st);
}

// =====================================================================================================
// Q_p = X_p M_p / X_p M_p^T on the MFMA
// =====================================================================================================
struct RgBuild {
  Operand X;        // the left rows in BATCH order: entity rows X.idx[i], or dense rows (X.idx.ptr == NULL: row i)
  Operand R;        // the relation table (its index is not read: the group's relation is group_rel[g])
  int dir;          // KGE_SP_: out = x M;  KGE_PO_: out = x M^T
  int d;
  float* out;       // STORE: row i at out + i * out_ld;  ATOMIC: row i ADDED to out + out_idx[i] * out_ld
  long long out_ld;
  Index out_idx;
};

// grid.x = row tile (of at most RG_MAX_TILES: workgroups behind the batch's last tile return), grid.y = column block.
// One chain per output element: acc = +0, then one v_mfma_f32_16x16x4_f32 per four k in ascending k -- k runs to d
// rounded up to 4, the padding is zero on both sides in LDS.
template <bool ATOMIC>
__global__ __launch_bounds__(RG_THREADS) void rsg_queries_kernel(RgBuild a, RgWs w) {
  __shared__ __attribute__((aligned(16))) float sX[RG_TM * RG_LDX];
  __shared__ __attribute__((aligned(16))) float sP[RG_KP * RG_LDP];
  __shared__ int sRow[RG_TM];
  const int tid = threadIdx.x, d = a.d, dk = (d + 3) & ~3;
  const int t = blockIdx.x;
  if (t >= w.counts[1]) return;
  const int g = rg_tile_group(w.tile_begin, w.counts[0], t);
  const int row0 = w.group_begin[g] + (t - w.tile_begin[g]) * RG_TM;
  const int rows = w.group_begin[g + 1] - row0 < RG_TM ? w.group_begin[g + 1] - row0 : RG_TM;
  const float* __restrict__ M = (const float*)a.R.base + (long long)w.group_rel[g] * a.R.ld;
  if (tid < RG_TM) sRow[tid] = tid < rows ? w.perm[row0 + tid] : -1;
  __syncthreads();
  for (int e = tid; e < RG_TM * dk; e += RG_THREADS) {
    const int r = e / dk, c = e - r * dk;
    const int bi = sRow[r];
    float v = 0.0f;
    if (bi >= 0 && c < d) v = ((const float*)a.X.base + index_at(a.X.idx, bi) * a.X.ld)[c];
    sX[r * RG_LDX + c] = v;
  }
  const int c0 = blockIdx.y * RG_CB;
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const bool live = c0 + wave * 16 < d;  // (wave-uniform: a wave whose 16 columns lie behind d issues nothing)
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = 0; k0 < dk; k0 += RG_KP) {
    __syncthreads();  // sX complete; the previous panel consumed
    if (a.dir == KGE_SP_) {  // panel[k][c] = M[k0 + k][c0 + c]: rows of M, read along their columns
      for (int e = tid; e < RG_KP * RG_CB; e += RG_THREADS) {
        const int k = e / RG_CB, c = e % RG_CB;
        const int gk = k0 + k, gc = c0 + c;
        sP[k * RG_LDP + c] = (gk < d && gc < d) ? M[(long long)gk * d + gc] : 0.0f;
      }
    } else {  // panel[k][c] = M[c0 + c][k0 + k]: the transpose, still read along the rows of M
      for (int e = tid; e < RG_KP * RG_CB; e += RG_THREADS) {
        const int k = e % RG_KP, c = e / RG_KP;
        const int gk = k0 + k, gc = c0 + c;
        sP[k * RG_LDP + c] = (gk < d && gc < d) ? M[(long long)gc * d + gk] : 0.0f;
      }
    }
    __syncthreads();
    const int kend = dk - k0 < RG_KP ? dk - k0 : RG_KP;
    if (live) {
      for (int kk = 0; kk < kend; kk += 4) {
        const float av = sX[lr * RG_LDX + k0 + kk + lq];       // A[m = lr][k = lq]
        const float bv = sP[(kk + lq) * RG_LDP + wave * 16 + lr];  // B[k = lq][n = lr]
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
    }
  }
  // acc[j] = C[m = 4 lq + j][n = lr]
  const int col = c0 + wave * 16 + lr;
  if (live && col < d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * lq + j;
      if (r < rows) {
        const long long bi = sRow[r];
        if (ATOMIC) atomicAdd(a.out + index_at(a.out_idx, bi) * a.out_ld + col, acc[j]);
        else a.out[bi * a.out_ld + col] = acc[j];
      }
    }
  }
}

static int rg_launch_build(const RgBuild& a, bool atomic, long long n, long long num_rel, const RgWs& w, hipStream_t st) {
  const dim3 grid((unsigned)rg_max_tiles(n, num_rel), (unsigned)((a.d + RG_CB - 1) / RG_CB));
  if (atomic) hipLaunchKernelGGL((rsg_queries_kernel<true>), grid, dim3(RG_THREADS), 0, st, a, w);
  else hipLaunchKernelGGL((rsg_queries_kernel<false>), grid, dim3(RG_THREADS), 0, st, a, w);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// kge_rescal_queries_grouped, n > 0
int run_rescal_queries_grouped(const Operand& A, const Operand& R, int dir, int d, long long n, long long num_rel,
                               float* q, long long q_ld, void* ws, hipStream_t st) {
  const RgWs w = rg_workspace(ws, n, d);
  int rc = run_rescal_group(R.idx, n, w, st);
  if (rc != KGE_OK) return rc;
  RgBuild b = {};
  b.X = A; b.R = R; b.dir = dir; b.d = d; b.out = q; b.out_ld = q_ld;
  return rg_launch_build(b, false, n, num_rel, w, st);
}

// =====================================================================================================
// backward
// =====================================================================================================
struct RgNeg {
  const float* ent; long long ent_ld;  // the entity table
  const void* neg; int neg_itype; long long neg_ld, K;
  const float* gout; long long ldg;
  const float* Q;                      // [n, d] the queries (workspace)
  float* GQ;                           // [n, d] out: g_q rows
  int d;
  float* ge; long long ge_ld;
};

// A workgroup per positive.  L = the power of two >= d (at least 32) lanes take a row's coordinates, the 256 / L lane
// sets take the samples k = set, set + sets, ...: each set one fma chain in ascending k from +0, the sets added in
// ascending order -- g_q is a function of (K, d) and the row's own samples, the same bits on every run.
__global__ __launch_bounds__(RG_THREADS) void rsg_neg_kernel(RgNeg a) {
  __shared__ long long sId[RG_NEG_CHUNK];
  __shared__ float sG[RG_NEG_CHUNK];
  __shared__ float sPart[8 * RG_LDX];
  const int tid = threadIdx.x, d = a.d;
  const long long i = blockIdx.x;
  int L = 32;
  while (L < d) L <<= 1;
  const int sets = RG_THREADS / L, c = tid & (L - 1), set = tid / L;
  const Index nix = {a.neg, 1, a.neg_itype};
  const float qc = c < d ? a.Q[i * d + c] : 0.0f;
  float acc = 0.0f;
  for (long long j0 = 0; j0 < a.K; j0 += RG_NEG_CHUNK) {
    __syncthreads();
    if (j0 + tid < a.K) {
      sId[tid] = index_at(nix, i * a.neg_ld + j0 + tid);
      sG[tid] = a.gout[i * a.ldg + j0 + tid];
    }
    __syncthreads();
    const int m = a.K - j0 < RG_NEG_CHUNK ? (int)(a.K - j0) : RG_NEG_CHUNK;
    if (c < d) {
      for (int j = set; j < m; j += sets) {  // (RG_NEG_CHUNK % sets == 0: sample k stays with set k % sets)
        const long long id = sId[j];
        const float gk = sG[j];
        acc = __builtin_fmaf(gk, a.ent[id * a.ent_ld + c], acc);
        atomicAdd(a.ge + id * a.ge_ld + c, gk * qc);
      }
      if (j0 + RG_NEG_CHUNK >= a.K) sPart[set * RG_LDX + c] = acc;
    }
  }
  __syncthreads();
  if (tid < d) {
    float s = sPart[tid];
    for (int k = 1; k < sets; ++k) s = s + sPart[k * RG_LDX + tid];
    a.GQ[i * d + tid] = s;
  }
}

struct RgRel {
  Operand E;        // the fixed entity rows, batch order
  const float* GQ;  // [n, d]
  int d, slot;
  float* gr; long long gr_ld;
};

// grid.x = group (of at most min(n, num_rel): workgroups behind the last group return), grid.y = 64 x 64 block of the
// d x d gradient.  Wave w owns rows [16 w, 16 w + 16) of the block and its four 16-column tiles.  One chain per element:
// acc = +0, one MFMA per four rows of the group in perm order (zero rows behind the group's end), then
// grad_rel[p][a][b] = grad_rel[p][a][b] + acc.
__global__ __launch_bounds__(RG_THREADS) void rsg_relgrad_kernel(RgRel a, RgWs w) {
  __shared__ __attribute__((aligned(16))) float sL[RG_TM * RG_LDP];
  __shared__ __attribute__((aligned(16))) float sR[RG_TM * RG_LDP];
  __shared__ int sRow[RG_TM];
  const int g = blockIdx.x;
  if (g >= w.counts[0]) return;
  const int tid = threadIdx.x, d = a.d;
  const int nb = (d + RG_CB - 1) / RG_CB;
  const int a0 = (blockIdx.y / nb) * RG_CB, b0 = (blockIdx.y % nb) * RG_CB;
  const int beg = w.group_begin[g], end = w.group_begin[g + 1];
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int r0 = beg; r0 < end; r0 += RG_TM) {
    __syncthreads();
    if (tid < RG_TM) sRow[tid] = r0 + tid < end ? w.perm[r0 + tid] : -1;
    __syncthreads();
    for (int e = tid; e < RG_TM * RG_CB; e += RG_THREADS) {
      const int r = e / RG_CB, c = e % RG_CB;
      const long long bi = sRow[r];
      float lv = 0.0f, rv = 0.0f;
      if (bi >= 0) {
        const float* er = (const float*)a.E.base + index_at(a.E.idx, bi) * a.E.ld;
        const float* gq = a.GQ + bi * d;
        const float* lp = a.slot == 2 ? er : gq;  // slot 2: g_M = s (x) g_q;  slot 0: g_M = g_q (x) o
        const float* rp = a.slot == 2 ? gq : er;
        if (a0 + c < d) lv = lp[a0 + c];
        if (b0 + c < d) rv = rp[b0 + c];
      }
      sL[r * RG_LDP + c] = lv;
      sR[r * RG_LDP + c] = rv;
    }
    __syncthreads();
    const int here = end - r0 < RG_TM ? end - r0 : RG_TM;
    for (int kk = 0; kk < here; kk += 4) {
      const float av = sL[(kk + lq) * RG_LDP + wave * 16 + lr];  // A[m = lr][k = lq]: column a of row kk + lq
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float bv = sR[(kk + lq) * RG_LDP + t * 16 + lr];
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  float* dst = a.gr + (long long)w.group_rel[g] * a.gr_ld;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cb = b0 + t * 16 + lr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ra = a0 + wave * 16 + 4 * lq + j;
      if (ra < d && cb < d) dst[(long long)ra * d + cb] = dst[(long long)ra * d + cb] + acc[t][j];
    }
  }
}

// kge_score_neg_bwd_accum_grouped, n > 0 and K > 0
int run_rescal_neg_bwd_accum_grouped(const Operand& S, const Operand& R, const Operand& O, int d, long long n,
                                     long long num_rel, int slot, const void* neg, int neg_itype, long long neg_ld,
                                     long long K, const float* gout, long long ldg, float* ge, long long ge_ld, float* gr,
                                     long long gr_ld, void* ws, hipStream_t st) {
  const RgWs w = rg_workspace(ws, n, d);
  const Operand& E = slot == 0 ? O : S;
  const int dir = slot == 0 ? KGE_PO_ : KGE_SP_;
  int rc = run_rescal_group(R.idx, n, w, st);
  if (rc != KGE_OK) return rc;
  RgBuild b = {};
  b.X = E; b.R = R; b.dir = dir; b.d = d; b.out = w.Q; b.out_ld = d;
  if ((rc = rg_launch_build(b, false, n, num_rel, w, st)) != KGE_OK) return rc;
  RgNeg ng = {(const float*)S.base, S.ld, neg, neg_itype, neg_ld, K, gout, ldg, w.Q, w.GQ, d, ge, ge_ld};
  hipLaunchKernelGGL(rsg_neg_kernel, dim3((unsigned)n), dim3(RG_THREADS), 0, st, ng);
  const int nb = (d + RG_CB - 1) / RG_CB;
  RgRel rl = {E, w.GQ, d, slot, gr, gr_ld};
  hipLaunchKernelGGL(rsg_relgrad_kernel, dim3((unsigned)(n < num_rel ? n : num_rel), (unsigned)(nb * nb)),
                     dim3(RG_THREADS), 0, st, rl, w);
  if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
  // the fixed rows: g_s = M g_q is the _po product of the g_q rows, g_o = M^T g_q the sp_ product
  RgBuild f = {};
  f.X = Operand{w.GQ, d, Index{nullptr, 1, 1}};
  f.R = R; f.dir = dir == KGE_SP_ ? KGE_PO_ : KGE_SP_; f.d = d; f.out = ge; f.out_ld = ge_ld; f.out_idx = E.idx;
  return rg_launch_build(f, true, n, num_rel, w, st);
}

}  // namespace kge
