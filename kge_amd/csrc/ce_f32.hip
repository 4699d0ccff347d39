// ce_f32.hip -- 1vsAll cross entropy of ComplEx / DistMult on FLOAT32 tables without a score matrix, gfx950:
// kge_ce_f32_fwd / kge_ce_f32_bwd (include/kge_amd.h).
//
// What the reference runs per direction (kge/job/train_1vsAll.py:64-81): score_sp / score_po -> an [n, E] score matrix,
// KLDivWithSoftmaxKgeLoss = cross entropy with index labels (kge/util/loss.py:192-207) -> an [n, E] log-softmax kept for
// the backward, and autograd's [n, E] gradient of the scores.  Here:
//
//   forward   pairs_f32_kernel<.., F3_CE> (score_pairs_f32.hip): the exact f32 matrix-core tile of kge_score_sp /
//             kge_score_po -- every score has the bits they store -- with a fold epilogue: a workgroup owns 128 query
//             rows and walks a run of column tiles, and one (max, sum exp, label score) record per (row, column group)
//             goes to the workspace.  ce_dist_merge_kernel (ce_dist.hip: the same record layout) merges a row's records
//             in column-group order.  No atomics: the same bits on every run.
//   backward  chunks of C entity columns.  pairs_f32_kernel<.., F3_GRAD> writes G [n, C] = d loss / d score of the chunk
//             (the scores are formed again and never stored); dT[c0 : c0 + C] = G^T Q overwrites the chunk's rows of
//             g_tgt (gemm32_kernel, K = n in one piece: the bits do not depend on the chunk width); dQ += G T[c0 : c0 + C]
//             leaves its split-K partials in the workspace, and ce_f32_dq_sum_kernel adds them to the running dQ in
//             chunk order, then split-K order (no atomics, no zero fill: the first chunk starts the sum).  Q is built
//             once (bwdg_build_q_kernel), the chain rule (bwdg_chain_kernel) runs once after the last chunk.
//
// Workspace: records (12 n G bytes, G <= 256) | dQ [n, d] | Q [n, d] | split-K partials | G [n, C]: nothing that grows
// with n E.  No allocation, no host wait, no library call: stream-ordered and capturable.
//
// The KvsAll losses of the same tables (kge_kl_f32_* / kge_bce_f32_*; train_KvsAll.py:216-294, loss.py:137-159 and
// :192-213) join this file with the label machinery of ce_dist.hip: labels are an int64 CSR per row.
//   forward   pairs_f32_kernel<.., F3_KL> keeps F3_CE's (max, sum exp) and tracks no label -- merged in
//             ce_dist_merge_kernel's order and expressions, lse has the bits of kge_ce_f32_fwd's --, F3_BCE folds
//             sum softplus(score + offset).  ml_f32_finish_kernel -- one wave per row -- scores the row's CSR entries
//             as f32 dot products <Q_i, T_j> (Q: bwdg_build_q_kernel, in the workspace's Q buffer; one fmaf chain over
//             the coordinates 0 .. d - 1: the operands of the tile in another summation order), sums them in CSR order
//             and merges the row's records in column-group order.
//   backward  the chunk loop of the 1vsAll loss; per chunk the label bits (n x C, cleared by fill_words_async, set by
//             ml_mask_kernel of ce_dist.hip) turn the gradient epilogue into F3_GRAD_KL / F3_GRAD_BCE; g_i and w_i per
//             row come from ml_rows_kernel (they live where the forward's records were).  The scores are linear in
//             the target row, so label smoothing's uniform term is a bias b_i inside the epilogue (label_bias).  The
//             bits are cleared once more after the last chunk.
// Workspace: the layout above | label bits (n C / 8 bytes).
#include "common.hpp"

namespace kge {

int run_pairs_f32_loss(int scorer, int mode, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                       long long n, long long m, float* out, long long ldo, const F32LossArgs& ce, hipStream_t st);
bool run_gemm32(bool a_kcont, int in16, long long M, long long N, long long K, const void* A, long long lda,
                const void* B, long long ldb, float* C, long long ldc, float* scratch, size_t scratch_bytes,
                hipStream_t st, int* parts = nullptr);
int run_bwdg_build_q(int scorer, const Operand& A, const Operand& R, int dir, int d, long long n, float* Q,
                     hipStream_t st);
int run_bwdg_chain(int scorer, const Operand& A, const Operand& R, int dir, int d, long long n, float* g_a, float* g_p,
                   hipStream_t st);
// ce_dist.hip; `col_tiles` counts ITS 64-column tiles per group
__global__ void ce_dist_merge_kernel(const float* __restrict__ rec, int groups, int col_tiles, long long n, long long m,
                                     Index label, float* __restrict__ loss_rows, float* __restrict__ lse);
// ce_dist.hip: the rows' g_i / w_i (fold 1 = kl, 2 = bce) and the chunk's label bits
__global__ void ml_rows_kernel(long long n, const long long* __restrict__ rowptr, const float* __restrict__ label_weight,
                               int fold, const float* __restrict__ g_rows, float g_scalar, float* __restrict__ grow,
                               float* __restrict__ wrow);
__global__ void ml_mask_kernel(long long n, const long long* __restrict__ rowptr, const long long* __restrict__ col,
                               long long col_lo, long long mc, unsigned int* __restrict__ mask, long long maskw);

constexpr int CF_TILE = 128;                        // rows and columns of a pairs_f32_kernel tile
constexpr int CF_MAX_GROUPS = 256;                  // column groups per row (records of the forward)
constexpr long long CF_CHUNK_BYTES = 32LL << 20;    // default gradient chunk of the backward
constexpr long long CF_SPLIT_BYTES = 8LL << 20;     // split-K partials of dQ: at most this much, at most 32 of them

static inline long long cf_align(long long b) { return (b + 255) / 256 * 256; }

// column tiles per workgroup of the forward: ~1024 workgroups where the shape has them, at most CF_MAX_GROUPS groups
// (cd_groups of ce_dist.hip on 128-wide tiles)
static inline void cf_groups(long long n, long long m, int& col_tiles, int& groups) {
  const long long rg = (n + CF_TILE - 1) / CF_TILE, tiles = (m + CF_TILE - 1) / CF_TILE;
  long long want = 1024 / (rg > 0 ? rg : 1);
  if (want < 1) want = 1;
  if (want > CF_MAX_GROUPS) want = CF_MAX_GROUPS;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const long long ct = (tiles + want - 1) / want;
  col_tiles = (int)(ct < 1 ? 1 : ct);
  groups = (int)((tiles + col_tiles - 1) / col_tiles);
  if (groups < 1) groups = 1;
}

static long long cf_records_bytes(long long n, long long m) {
  int ct, g;
  cf_groups(n, m, ct, g);
  return cf_align(n * g * 3 * (long long)sizeof(float));
}
static long long cf_nd_bytes(long long n, int d) { return cf_align(n * d * (long long)sizeof(float)); }
static long long cf_split_bytes(long long n, int d) {
  const long long one = n * d * (long long)sizeof(float);
  long long p = CF_SPLIT_BYTES / one;
  if (p > 32) p = 32;
  if (p < 1) p = 1;
  return cf_align(p * one);
}
static long long cf_fixed_bytes(long long n, long long m, int d) {
  return cf_records_bytes(n, m) + 2 * cf_nd_bytes(n, d) + cf_split_bytes(n, d);
}

// the backward's chunk width for a workspace of `bytes`: a multiple of 128, clamped to E rounded up; 0 = too small
static long long cf_chunk_cols(long long n, long long m, int d, long long bytes) {
  const long long left = bytes - cf_fixed_bytes(n, m, d);
  if (left <= 0 || n <= 0) return 0;
  const long long c = left / (4 * n) / CF_TILE * CF_TILE;
  const long long cap = (m + CF_TILE - 1) / CF_TILE * CF_TILE;
  return c > cap ? cap : c;
}

// the chunk width a caller asked for: 0 = at most CF_CHUNK_BYTES of G (at least one tile), clamped to E rounded up
static long long cf_asked_cols(long long n, long long m, long long chunk_cols) {
  const long long cap = (m + CF_TILE - 1) / CF_TILE * CF_TILE;
  long long c = chunk_cols;
  if (c == 0) {
    c = CF_CHUNK_BYTES / (4 * n) / CF_TILE * CF_TILE;
    if (c < CF_TILE) c = CF_TILE;
  }
  return c > cap ? cap : c;
}

long long ce_f32_workspace_bytes(long long n, long long m, int d, long long chunk_cols) {
  return cf_fixed_bytes(n, m, d) + cf_align(4 * n * cf_asked_cols(n, m, chunk_cols));
}

// KvsAll: ... | G [n, C] | label bits [n, C / 32] words (C % 128 == 0: a tile's columns fall on whole words)
static inline long long mf_chunk_bytes(long long n, long long c) { return cf_align(4 * n * c) + cf_align(n * c / 8); }

long long ml_f32_workspace_bytes(long long n, long long m, int d, long long chunk_cols) {
  return cf_fixed_bytes(n, m, d) + mf_chunk_bytes(n, cf_asked_cols(n, m, chunk_cols));
}

// what the forward touches: the records and, behind dQ, the Q buffer
static long long mf_fwd_bytes(long long n, long long m, int d) { return cf_records_bytes(n, m) + 2 * cf_nd_bytes(n, d); }

static long long mf_chunk_cols(long long n, long long m, int d, long long bytes) {
  const long long left = bytes - cf_fixed_bytes(n, m, d);
  if (left <= 0 || n <= 0) return 0;
  long long c = left / n * 8 / 33 / CF_TILE * CF_TILE;  // 4 + 1/8 bytes per row and column
  const long long cap = (m + CF_TILE - 1) / CF_TILE * CF_TILE;
  if (c > cap) c = cap;
  while (c >= CF_TILE && mf_chunk_bytes(n, c) > left) c -= CF_TILE;
  return c < CF_TILE ? 0 : c;
}

// what run_pairs_f32 takes: d % 8 == 0 (whole quads in both halves), 16-byte aligned float32 rows
bool ce_f32_layout_ok(int d, const Operand& A, const Operand& R, const Operand& TG) {
  if (d <= 0 || d % 8) return false;
  if (((uintptr_t)A.base | (uintptr_t)R.base | (uintptr_t)TG.base) & 15) return false;
  return !((A.ld * 4) % 16 || (R.ld * 4) % 16 || (TG.ld * 4) % 16);
}

int run_ce_f32_fwd(int scorer, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, long long n,
                   long long m, const Index& label, float* loss_rows, float* lse, void* ws, long long ws_bytes,
                   hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (!ce_f32_layout_ok(d, A, R, TG)) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255) || ws_bytes < cf_records_bytes(n, m)) return KGE_ERR_WORKSPACE;
  F32LossArgs ce{};
  ce.label = label;
  ce.rec = (float*)ws;
  cf_groups(n, m, ce.col_tiles, ce.groups);
  const int rc = run_pairs_f32_loss(scorer, F3_CE, A, R, TG, dir, d, n, m, nullptr, 0, ce, st);
  if (rc != KGE_OK) return rc;
  hipLaunchKernelGGL(ce_dist_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ce.rec, ce.groups,
                     ce.col_tiles * (CF_TILE / 64), n, m, label, loss_rows, lse);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// out = base (NULL: nothing) + part[0] + part[1] + ... in that order; out may be base
__global__ __launch_bounds__(256) void ce_f32_dq_sum_kernel(const float* part, long long cnt, int P, const float* base,
                                                            float* out) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= cnt) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int p = 0;
  if (base != nullptr) acc = *reinterpret_cast<const f32x4*>(base + i);
  else acc = *reinterpret_cast<const f32x4*>(part + i), p = 1;
  for (; p < P; ++p) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + (long long)p * cnt + i);
    acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
  }
  *reinterpret_cast<f32x4*>(out + i) = acc;
}

// The chunk loop of all three losses.  mode F3_GRAD: label / g_rows / g_scalar; F3_GRAD_KL / F3_GRAD_BCE: the CSR,
// label_weight, label_bias and offset.  TG: ALL rows of the entity table (identity index)
static int run_f32_bwd(int mode, int scorer, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                       long long n, long long m, const Index& label, const long long* rowptr, const long long* col,
                       const float* label_weight, const float* label_bias, float offset, const float* lse,
                       const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt, void* ws,
                       long long ws_bytes, hipStream_t st) {
  const bool ml = mode != F3_GRAD;
  if (n == 0)  // no query: the entity rows get a zero gradient
    return fill_words_async(g_tgt, 0, (size_t)m * d * sizeof(float), st) ? KGE_OK : KGE_ERR_LAUNCH;
  if (!ce_f32_layout_ok(d, A, R, TG)) return KGE_ERR_UNSUPPORTED;
  if (n >= (1LL << 31) || m >= (1LL << 31) || TG.ld >= (1LL << 31)) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255)) return KGE_ERR_WORKSPACE;
  const long long C = ml ? mf_chunk_cols(n, m, d, ws_bytes) : cf_chunk_cols(n, m, d, ws_bytes);
  if (C < CF_TILE) return KGE_ERR_WORKSPACE;
  float* dq = (float*)((char*)ws + cf_records_bytes(n, m));
  float* Q = (float*)((char*)dq + cf_nd_bytes(n, d));
  float* part = (float*)((char*)Q + cf_nd_bytes(n, d));
  const long long part_bytes = cf_split_bytes(n, d);
  float* G = (float*)((char*)part + part_bytes);
  int rc = run_bwdg_build_q(scorer, A, R, dir, d, n, Q, st);
  if (rc != KGE_OK) return rc;
  F32LossArgs ce{};
  ce.label = label;
  ce.lse = lse;
  ce.g_rows = g_rows;
  ce.g_scalar = g_scalar;
  unsigned int* mask = nullptr;
  const size_t mask_bytes = (size_t)(n * C / 8);
  if (ml) {
    mask = (unsigned int*)((char*)G + cf_align(4 * n * C));
    float* rows = (float*)ws;  // (where the forward's records were: 12 n G bytes >= 8 n)
    ce.mask = mask;
    ce.maskw = C / 32;
    ce.grow = rows;
    ce.wrow = rows + n;
    ce.bias = label_bias;
    ce.offset = offset;
    hipLaunchKernelGGL(ml_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr, label_weight,
                       mode == F3_GRAD_KL ? 1 : 2, g_rows, g_scalar, rows, rows + n);
  }
  const long long cnt = n * d;  // d % 8 == 0: whole quads
  for (long long lo = 0; lo < m; lo += C) {
    const long long mc = m - lo < C ? m - lo : C;
    const float* Tc = (const float*)TG.base + lo * TG.ld;
    const Operand TGc{Tc, TG.ld, Index{nullptr, 1, KGE_I64}};
    ce.col_lo = lo;
    if (ml) {
      if (!fill_words_async(mask, 0, mask_bytes, st)) return KGE_ERR_LAUNCH;
      hipLaunchKernelGGL(ml_mask_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, rowptr, col, lo, mc, mask,
                         C / 32);
    }
    rc = run_pairs_f32_loss(scorer, mode, A, R, TGc, dir, d, n, mc, G, C, ce, st);
    if (rc != KGE_OK) return rc;
    // dT[lo : lo + mc] = G^T Q  (K = n, one piece)
    if (!run_gemm32(false, 0, mc, d, n, G, C, Q, d, g_tgt + lo * d, d, nullptr, 0, st)) return KGE_ERR_UNSUPPORTED;
    // dQ (+)= G T[lo : lo + mc]  (K = mc, split): chunk order, then split-K order; the last sum lands in g_a
    int parts = 0;
    if (!run_gemm32(true, 0, n, d, mc, G, C, Tc, TG.ld, nullptr, d, part, (size_t)part_bytes, st, &parts) || parts < 1)
      return KGE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ce_f32_dq_sum_kernel, dim3((unsigned)((cnt / 4 + 255) / 256)), dim3(256), 0, st, part, cnt, parts,
                       lo == 0 ? (const float*)nullptr : dq, lo + C >= m ? g_a : dq);
  }
  // (the mask is left all-zero: a workspace handed on holds no label of this call)
  if (ml && !fill_words_async(mask, 0, mask_bytes, st)) return KGE_ERR_LAUNCH;
  return run_bwdg_chain(scorer, A, R, dir, d, n, g_a, g_p, st);
}

int run_ce_f32_bwd(int scorer, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, long long n,
                   long long m, const Index& label, const float* lse, const float* g_rows, float g_scalar, float* g_a,
                   float* g_p, float* g_tgt, void* ws, long long ws_bytes, hipStream_t st) {
  return run_f32_bwd(F3_GRAD, scorer, A, R, TG, dir, d, n, m, label, nullptr, nullptr, nullptr, nullptr, 0.0f, lse,
                     g_rows, g_scalar, g_a, g_p, g_tgt, ws, ws_bytes, st);
}

// ---- KvsAll ---------------------------------------------------------------------------------------------------------
// One WAVE per row: the scores of the row's CSR entries (64 at a time, one per lane) as f32 dot products <Q_i, T_j> --
// one fmaf chain over the coordinates 0 .. d - 1 --, summed in CSR order, and the row's records merged in column-group
// order with the expressions of ml_dist_finish_kernel (ce_dist.hip):
//   BCE == false  lse[i] as ce_dist_merge_kernel; loss_rows[i] = lse - w_i sum (label_weight given: every row) or
//                 lse - sum / k_i - log k_i (0 for k_i = 0)
//   BCE == true   loss_rows[i] = sum_g rec - sum over the labels of (score + offset)
// A label outside [0, m) is not scored: loss_rows[i] = NaN.  T: the entity table, row pitch ldt; d % 4 == 0, 16-byte rows.
template <bool BCE>
__global__ __launch_bounds__(256) void ml_f32_finish_kernel(const float* __restrict__ Q, const float* __restrict__ T,
                                                            long long ldt, int d, long long n, long long m,
                                                            const float* __restrict__ rec, int groups,
                                                            const long long* __restrict__ rowptr,
                                                            const long long* __restrict__ col,
                                                            const float* __restrict__ label_weight, float offset,
                                                            float* __restrict__ loss_rows, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const long long b = rowptr[i], e = rowptr[i + 1];
  const float* q = Q + i * d;
  float sum = 0.0f;
  bool bad = false;
  for (long long base = b; base < e; base += 64) {
    const long long x = base + lane;
    float sc = 0.0f;
    bool oob = false;
    if (x < e) {
      const long long j = col[x];
      oob = j < 0 || j >= m;
      if (!oob) {
        const float* t = T + j * ldt;
        for (int c = 0; c < d; c += 4) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(q + c), tv = *reinterpret_cast<const f32x4*>(t + c);
          sc = __builtin_fmaf(qv[0], tv[0], sc);
          sc = __builtin_fmaf(qv[1], tv[1], sc);
          sc = __builtin_fmaf(qv[2], tv[2], sc);
          sc = __builtin_fmaf(qv[3], tv[3], sc);
        }
        if (BCE) sc += offset;
      }
    }
    bad = bad || __ballot(oob) != 0ULL;
    const int cnt = e - base < 64 ? (int)(e - base) : 64;
    for (int l = 0; l < cnt; ++l) sum += __shfl(sc, l, 64);
  }
  if (lane != 0) return;
  const float* r = rec + i * groups * 3;
  const long long k = e - b;
  const float nan = __builtin_nanf("");
  if (BCE) {
    float tot = 0.0f;
    for (int g = 0; g < groups; ++g) tot += r[g * 3];
    loss_rows[i] = bad ? nan : tot - sum;
    return;
  }
  float mm = -__builtin_inff();
  for (int g = 0; g < groups; ++g)
    if (r[g * 3 + 1] > 0.0f) mm = __builtin_fmaxf(mm, r[g * 3]);
  float ss = 0.0f;
  for (int g = 0; g < groups; ++g)
    if (r[g * 3 + 1] > 0.0f) ss += r[g * 3 + 1] * expf(r[g * 3] - mm);
  const float z = mm + logf(ss);
  lse[i] = z;
  float out;
  if (label_weight != nullptr) out = z - label_weight[i] * (k > 0 ? sum : 0.0f);
  else out = k > 0 ? z - sum / (float)k - logf((float)k) : 0.0f;
  loss_rows[i] = bad ? nan : out;
}

// bce: lse is not touched.  TG: ALL rows of the entity table (identity index)
int run_ml_f32_fwd(bool bce, int scorer, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                   long long n, long long m, const long long* rowptr, const long long* col, const float* label_weight,
                   float offset, float* loss_rows, float* lse, void* ws, long long ws_bytes, hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (!ce_f32_layout_ok(d, A, R, TG)) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255) || ws_bytes < mf_fwd_bytes(n, m, d)) return KGE_ERR_WORKSPACE;
  F32LossArgs ce{};
  ce.rec = (float*)ws;
  ce.offset = offset;
  cf_groups(n, m, ce.col_tiles, ce.groups);
  float* Q = (float*)((char*)ws + cf_records_bytes(n, m) + cf_nd_bytes(n, d));
  int rc = run_pairs_f32_loss(scorer, bce ? F3_BCE : F3_KL, A, R, TG, dir, d, n, m, nullptr, 0, ce, st);
  if (rc != KGE_OK) return rc;
  rc = run_bwdg_build_q(scorer, A, R, dir, d, n, Q, st);
  if (rc != KGE_OK) return rc;
  const dim3 grid((unsigned)((n + 3) / 4));
  if (bce)
    hipLaunchKernelGGL((ml_f32_finish_kernel<true>), grid, dim3(256), 0, st, Q, (const float*)TG.base, TG.ld, d, n, m,
                       ce.rec, ce.groups, rowptr, col, label_weight, offset, loss_rows, lse);
  else
    hipLaunchKernelGGL((ml_f32_finish_kernel<false>), grid, dim3(256), 0, st, Q, (const float*)TG.base, TG.ld, d, n, m,
                       ce.rec, ce.groups, rowptr, col, label_weight, offset, loss_rows, lse);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

int run_ml_f32_bwd(bool bce, int scorer, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                   long long n, long long m, const long long* rowptr, const long long* col, const float* label_weight,
                   const float* label_bias, float offset, const float* lse, const float* g_rows, float g_scalar,
                   float* g_a, float* g_p, float* g_tgt, void* ws, long long ws_bytes, hipStream_t st) {
  return run_f32_bwd(bce ? F3_GRAD_BCE : F3_GRAD_KL, scorer, A, R, TG, dir, d, n, m, Index{nullptr, 1, KGE_I64}, rowptr,
                     col, label_weight, label_bias, offset, lse, g_rows, g_scalar, g_a, g_p, g_tgt, ws, ws_bytes, st);
}

}  // namespace kge
