// ce_dist.hip -- 1vsAll cross entropy of the DISTANCE scorers (TransE, RotatE) on float32 tables without a score
// matrix, gfx950: kge_ce_dist_fwd / kge_ce_dist_bwd (include/kge_amd.h).
//
// What the reference runs per direction (kge/job/train_1vsAll.py:64-81): score_sp / score_po -> an [n, E] score matrix
// (transe.py:18-34, rotate.py:30-64), KLDivWithSoftmaxKgeLoss = cross entropy with index labels (kge/util/loss.py:192-207)
// -> an [n, E] log-softmax kept for the backward, and autograd's [n, E] gradient of the scores.  Here:
//
//   forward   ce_dist_fwd_kernel: the 64 x 64 tile of pairs_kernel (score_pairs.hip; the same staging, the same micro-tile
//             -- pairs_device.hpp --, the same finish: every score has the bits kge_score_sp / kge_score_po store).  A
//             workgroup owns 64 query rows and walks a run of column tiles; each finished tile goes through the operand
//             LDS buffers and is folded into a per-thread running (max, sum exp) -- four threads per row, 16 columns
//             each --; at the end the four are merged in a fixed order and ONE (max, sum, label score) record per
//             (row, column group) goes to the workspace.  ce_dist_merge_kernel merges a row's records in column-group
//             order: no atomics, the same bits on every run.
//   backward  chunks of C entity columns: the scoring route (run_pairs_exact) writes S[n, C] into the workspace, and the
//             two gradient kernels -- laid out like bwd_pairs_kernel (bwd.hip): 64 rows x 32 coordinate pairs, the other
//             side streamed through LDS 16 rows at a time -- form the weight g_i (exp(S_ij - lse_i) - [j == label_i])
//             and the distance -S_ij while they stage: d loss / d score is never written.  The target side overwrites
//             the chunk's own rows of g_tgt; the query side adds its partial dQ into an [n, d] workspace buffer
//             (atomics: the chunk's columns are split over blockIdx.z), and ce_dist_chain_kernel applies the chain rule
//             to the gathered a / p rows once, after the last chunk.
//
// Extra device memory: 4 n C bytes (the score chunk) + 4 n d (dQ) + 12 n G (the forward's records, G <= 256 column
// groups): nothing that grows with n E.  No allocation, no host wait, no library call: stream-ordered and capturable.
//
// The KvsAll losses of the same scorers (kge_kl_dist_* / kge_bce_dist_*; train_KvsAll.py:216-294, loss.py:137-159 and
// :192-213) run on the same kernels with another FOLD: labels are an int64 CSR per row instead of one index.
//   forward   FOLD_KL keeps the running (max, sum exp) and tracks no label, FOLD_BCE folds sum softplus(score + offset);
//             ml_dist_finish_kernel -- one wave per row -- scores the row's CSR entries with the tile's arithmetic (the
//             same operations per coordinate pair in the same order: the bits of kge_score_sp / kge_score_po), sums them
//             in CSR order and merges the row's records in column-group order.
//   backward  per chunk a bit mask of n x C bits (ml_mask_kernel: one vector atomicOr per CSR entry whose column falls
//             into the chunk) tells the gradient kernels whether (i, j) is a label: the weight becomes
//             g_i (exp(S_ij - lse_i) - w_i [j in labels_i]) or g_i (sigmoid(S_ij + offset) - [j in labels_i]); g_i and
//             w_i per row come from ml_rows_kernel (they live where the forward's records were).  Everything else --
//             the chunk loop, dQ, the chain rule -- is the 1vsAll code.  The mask is cleared before every chunk and
//             after the last one.
#include "bwd_device.hpp"
#include "pairs_device.hpp"

namespace kge {

int run_pairs_exact(int scorer, int dtype, bool use_mfma, const Operand& A, const Operand& R, const Operand& TG, int dir,
                    int d, int dr, long long n, long long m, float lp, float* out, long long ldo, hipStream_t st,
                    bool round_query, const RankArgs* rk = nullptr);

enum { FOLD_CE = 0, FOLD_KL = 1, FOLD_BCE = 2 };  // index label + log-sum-exp | CSR labels + log-sum-exp | + softplus

// what the KvsAll folds of the backward read besides S: the chunk's label bits (row pitch `maskw` words), the per-row
// upstream gradient (0 for a row without labels under the unweighted kl loss) and label weight, the bce offset
struct MlArgs {
  const unsigned int* mask;
  long long maskw;
  const float* grow;
  const float* wrow;
  float offset;
};

constexpr int CD_MAX_GROUPS = 256;                  // column groups per row (records of the forward)
constexpr long long CD_CHUNK_BYTES = 32LL << 20;    // default score chunk of the backward

static inline long long cd_align(long long b) { return (b + 255) / 256 * 256; }

// column tiles per workgroup of the forward: ~1024 workgroups where the shape has them, at most CD_MAX_GROUPS groups
static inline void cd_groups(long long n, long long m, int& col_tiles, int& groups) {
  const long long rg = (n + PT_BM - 1) / PT_BM, tiles = (m + PT_BN - 1) / PT_BN;
  long long want = 1024 / (rg > 0 ? rg : 1);
  if (want < 1) want = 1;
  if (want > CD_MAX_GROUPS) want = CD_MAX_GROUPS;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const long long ct = (tiles + want - 1) / want;
  col_tiles = (int)(ct < 1 ? 1 : ct);
  groups = (int)((tiles + col_tiles - 1) / col_tiles);
  if (groups < 1) groups = 1;
}

long long ce_dist_records_bytes(long long n, long long m) {
  int ct, g;
  cd_groups(n, m, ct, g);
  return cd_align(n * g * 3 * (long long)sizeof(float));
}
long long ce_dist_dq_bytes(long long n, int d) { return cd_align(n * d * (long long)sizeof(float)); }

// the backward's chunk width for a workspace of `bytes`: a multiple of 64, clamped to E rounded up; 0 = too small
long long ce_dist_chunk_cols(long long n, long long m, int d, long long bytes) {
  const long long left = bytes - ce_dist_records_bytes(n, m) - ce_dist_dq_bytes(n, d);
  if (left <= 0 || n <= 0) return 0;
  long long c = left / (4 * n) / 64 * 64;
  const long long cap = (m + 63) / 64 * 64;
  return c > cap ? cap : c;
}

long long ce_dist_workspace_bytes(long long n, long long m, int d, long long chunk_cols) {
  const long long cap = (m + 63) / 64 * 64;
  long long c = chunk_cols;
  if (c == 0) {
    c = CD_CHUNK_BYTES / (4 * n) / 64 * 64;
    if (c < 64) c = 64;
  }
  if (c > cap) c = cap;
  return ce_dist_records_bytes(n, m) + ce_dist_dq_bytes(n, d) + cd_align(4 * n * c);
}

// KvsAll: records | dQ | S [n, C] | label bits [n, C / 32] words.  The backward keeps its per-row g_i and w_i (2 n floats)
// where the forward's records were (12 n G bytes >= 8 n).
static inline long long ml_chunk_bytes(long long n, long long c) { return cd_align(4 * n * c) + cd_align(n * c / 8); }

long long ml_dist_chunk_cols(long long n, long long m, int d, long long bytes) {
  const long long left = bytes - ce_dist_records_bytes(n, m) - ce_dist_dq_bytes(n, d);
  if (left <= 0 || n <= 0) return 0;
  long long c = left / n * 8 / 33 / 64 * 64;  // 4 + 1/8 bytes per row and column
  const long long cap = (m + 63) / 64 * 64;
  if (c > cap) c = cap;
  while (c >= 64 && ml_chunk_bytes(n, c) > left) c -= 64;
  return c < 64 ? 0 : c;
}

long long ml_dist_workspace_bytes(long long n, long long m, int d, long long chunk_cols) {
  const long long cap = (m + 63) / 64 * 64;
  long long c = chunk_cols;
  if (c == 0) {
    c = CD_CHUNK_BYTES / (4 * n) / 64 * 64;
    if (c < 64) c = 64;
  }
  if (c > cap) c = cap;
  return ce_dist_records_bytes(n, m) + ce_dist_dq_bytes(n, d) + ml_chunk_bytes(n, c);
}

// ---- forward ------------------------------------------------------------------------------------------------------
// rec[(row * groups + g) * 3 + {0, 1, 2}] = max, sum exp(score - max), score(row, label_row) (0 where the label's
// column is not in group g) over the group's valid columns.  A group of padding alone cannot exist (groups cover [0, m)).
// FOLD_KL: the same without a label (`label` is not read; rec[.. + 2] is not written).  FOLD_BCE: rec[.. + 0] =
// sum softplus(score + offset) over the group's valid columns.
__device__ __forceinline__ float softplus_f(float x) {  // max(x, 0) + log1p(exp(-|x|)) (loss.py:137-159)
  return __builtin_fmaxf(x, 0.0f) + log1pf(expf(-__builtin_fabsf(x)));
}

template <int SCORER, int NORM, bool VEC, int FOLD>
__global__ __launch_bounds__(256) void ce_dist_fwd_kernel(Operand A, Operand R, Operand TG, int dir, int d, int dr,
                                                          long long n, long long m, float lp, Index label, int col_tiles,
                                                          int groups, float* __restrict__ rec, float offset) {
  __shared__ __attribute__((aligned(16))) float QT[2][2][PT_KC][PT_LD];  // operands; then the finished score tile
  auto& Qs = QT[0];
  auto& Ts = QT[1];
  static_assert(sizeof(QT) >= PT_BM * PT_LD * 4, "the score tile fits the operand buffers");
  float* const tile = &QT[0][0][0][0];  // [64][PT_LD]

  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.y * PT_BM;
  const int hh = (d + 1) / 2;  // coordinate pairs
  const int lim1 = d - hh;     // valid second-half elements
  const int nchunk = (hh + PT_KC - 1) / PT_KC;
  const int sr = tid >> 2, scq = tid & 3;
  const int tx = tid & 15, ty = tid >> 4;
  long long qrow = row0 + sr;
  if (qrow >= n) qrow = n - 1;  // clamp: rows beyond n are computed but never stored
  const float* arow = (const float*)A.base + index_at(A.idx, qrow) * A.ld;
  const float* rrow = (const float*)R.base + index_at(R.idx, qrow) * R.ld;
  const int rl0 = (SCORER == KGE_ROTATE) ? dr : hh;
  const int rl1 = (SCORER == KGE_ROTATE) ? 0 : lim1;

  // fold role: row fr of the tile (the staging row: qrow), columns 16 * fq .. + 15
  const int fr = sr, fq = scq;
  const long long lbl = FOLD == FOLD_CE ? index_at(label, qrow) : -1;
  float run_m = -__builtin_inff(), run_s = 0.0f, lbl_score = 0.0f;

  for (int ct = 0; ct < col_tiles; ++ct) {
    const long long col0 = ((long long)blockIdx.x * col_tiles + ct) * PT_BN;
    if (col0 >= m) break;  // (uniform over the workgroup)
    if (ct > 0) __syncthreads();  // the previous tile's fold is done with the buffers
    long long trow = col0 + sr;
    if (trow >= m) trow = m - 1;
    const float* tgrow = (const float*)TG.base + index_at(TG.idx, trow) * TG.ld;

    f32x4 a0, a1, r0, r1, t0, t1;
    auto gload = [&](int ch) {
      const int cw = ch * PT_KC + scq * 4;
      // chunk tail beyond the row (VEC: hh % 4 == 0, whole quads): the row's first quad is loaded instead and zeros are
      // selected -- no branch around the loads, the six quads stay in registers (a branch put them into scratch)
      const bool tail = VEC && cw >= hh;
      const int c = tail ? 0 : cw;
      a0 = load4<float, VEC>(arow, c, hh);
      a1 = load4<float, VEC>(arow + hh, c, lim1);
      r0 = load4<float, VEC>(rrow, c, rl0);
      if (SCORER != KGE_ROTATE) r1 = load4<float, VEC>(rrow + hh, c, rl1);
      else r1 = r0;
      t0 = load4<float, VEC>(tgrow, c, hh);
      t1 = load4<float, VEC>(tgrow + hh, c, lim1);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      a0 = tail ? z : a0; a1 = tail ? z : a1; r0 = tail ? z : r0; r1 = tail ? z : r1; t0 = tail ? z : t0; t1 = tail ? z : t1;
    };
    auto sstore = [&]() {
      f32x4 q0, q1;
      build_q4<SCORER>(dir, a0, a1, r0, r1, q0, q1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Qs[0][scq * 4 + i][sr] = q0[i];
        Qs[1][scq * 4 + i][sr] = q1[i];
        Ts[0][scq * 4 + i][sr] = t0[i];
        Ts[1][scq * 4 + i][sr] = t1[i];
      }
    };

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

    gload(0);
    sstore();
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
      if (ch + 1 < nchunk) gload(ch + 1);
#pragma unroll 4
      for (int cc = 0; cc < PT_KC; ++cc) {
        f32x4 q0 = *reinterpret_cast<const f32x4*>(&Qs[0][cc][ty * 4]);
        f32x4 q1 = *reinterpret_cast<const f32x4*>(&Qs[1][cc][ty * 4]);
        f32x4 t0v = *reinterpret_cast<const f32x4*>(&Ts[0][cc][tx * 4]);
        f32x4 t1v = *reinterpret_cast<const f32x4*>(&Ts[1][cc][tx * 4]);
        dist_micro_tile<SCORER, NORM>(q0, q1, t0v, t1v, acc, lp);
      }
      __syncthreads();
      if (ch + 1 < nchunk) sstore();
      __syncthreads();
    }

    // the finished tile through the operand buffers (the loop ended with a barrier)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(ty * 4 + i) * PT_LD + tx * 4 + j] = dist_score<NORM>(acc[i][j], lp);
    __syncthreads();

    // fold: this thread's 16 columns of row fr; padding columns (>= m) take no part -- a thread that has seen only
    // padding keeps (-inf, 0), which the merges below skip
    const long long cbase = col0 + fq * 16;
    long long valid = m - cbase;
    if (valid > 16) valid = 16;
    if (valid > 0) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(&tile[fr * PT_LD + fq * 16 + q * 4]);
        v[q * 4 + 0] = x[0]; v[q * 4 + 1] = x[1]; v[q * 4 + 2] = x[2]; v[q * 4 + 3] = x[3];
      }
      if (FOLD == FOLD_BCE) {
        float s = run_s;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < valid) s += softplus_f(v[k] + offset);
        run_s = s;
      } else {
        float tm = v[0];
#pragma unroll
        for (int k = 1; k < 16; ++k)
          if (k < valid) tm = __builtin_fmaxf(tm, v[k]);
        const float nm = __builtin_fmaxf(run_m, tm);
        float s = run_s * expf(run_m - nm);  // (first tile: 0 * exp(-inf) = 0)
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k < valid) s += expf(v[k] - nm);
        run_m = nm;
        run_s = s;
      }
      if (FOLD == FOLD_CE) {
        const long long off = lbl - cbase;
        if (off >= 0 && off < valid) {
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (k == (int)off) lbl_score = v[k];
        }
      }
    }
  }

  // merge the row's four threads (neighbouring lanes 4 sr .. 4 sr + 3) in lane order
  float pm[4], ps[4], pl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int src = (tid & 63 & ~3) | k;
    pm[k] = __shfl(run_m, src, 64);
    ps[k] = __shfl(run_s, src, 64);
    pl[k] = __shfl(lbl_score, src, 64);
  }
  if (FOLD == FOLD_BCE) {
    if (fq == 0 && row0 + fr < n) rec[((row0 + fr) * groups + blockIdx.x) * 3] = ((ps[0] + ps[1]) + ps[2]) + ps[3];
    return;
  }
  if (fq == 0 && row0 + fr < n) {
    float mm = pm[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) mm = __builtin_fmaxf(mm, pm[k]);
    float ss = 0.0f, ll = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (ps[k] > 0.0f) ss += ps[k] * expf(pm[k] - mm);
      ll += pl[k];  // (at most one of the four is not zero)
    }
    float* out = rec + ((row0 + fr) * groups + blockIdx.x) * 3;
    out[0] = mm;
    out[1] = ss;
    if (FOLD == FOLD_CE) out[2] = ll;
  }
}

// lse[i] = log sum_j exp(score_ij), loss_rows[i] = lse[i] - score(i, label_i): the row's records in group order
__global__ __launch_bounds__(256) void ce_dist_merge_kernel(const float* __restrict__ rec, int groups, int col_tiles,
                                                            long long n, long long m, Index label,
                                                            float* __restrict__ loss_rows, float* __restrict__ lse) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* r = rec + i * groups * 3;
  float mm = -__builtin_inff();
  for (int g = 0; g < groups; ++g)
    if (r[g * 3 + 1] > 0.0f) mm = __builtin_fmaxf(mm, r[g * 3]);
  float ss = 0.0f;
  for (int g = 0; g < groups; ++g)
    if (r[g * 3 + 1] > 0.0f) ss += r[g * 3 + 1] * expf(r[g * 3] - mm);
  const float l = mm + logf(ss);
  lse[i] = l;
  const long long lb = index_at(label, i);
  float out = __builtin_nanf("");
  if (lb >= 0 && lb < m) out = l - r[(lb / PT_BN / col_tiles) * 3 + 2];
  loss_rows[i] = out;
}

template <int SCORER, int NORM>
static int launch_fwd(bool vec, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr, long long n,
                      long long m, float lp, const Index& label, float* loss_rows, float* lse, float* rec, hipStream_t st) {
  int ct, groups;
  cd_groups(n, m, ct, groups);
  const dim3 grid((unsigned)groups, (unsigned)((n + PT_BM - 1) / PT_BM));
  if (vec)
    hipLaunchKernelGGL((ce_dist_fwd_kernel<SCORER, NORM, true, FOLD_CE>), grid, dim3(256), 0, st, A, R, TG, dir, d, dr, n, m,
                       lp, label, ct, groups, rec, 0.0f);
  else
    hipLaunchKernelGGL((ce_dist_fwd_kernel<SCORER, NORM, false, FOLD_CE>), grid, dim3(256), 0, st, A, R, TG, dir, d, dr, n, m,
                       lp, label, ct, groups, rec, 0.0f);
  hipLaunchKernelGGL(ce_dist_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rec, groups, ct, n, m,
                     label, loss_rows, lse);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// score(i, j) with the bits the tile stores at (i, j): the operations of dist_micro_tile on one live element, coordinate
// pairs 0 .. hh - 1 in order (the tile's padding pairs add |0 - 0| = 0: no change), then dist_score.  RotatE takes the
// IEEE square root: both branches of the micro-tile are correctly rounded, so the bits do not depend on the branch.
template <int SCORER, int NORM>
__device__ __forceinline__ float dist_label_score(const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                                                  int dr, long long i, long long j, float lp) {
  const int hh = (d + 1) / 2, lim1 = d - hh;
  const int rl0 = (SCORER == KGE_ROTATE) ? dr : hh;
  const int rl1 = (SCORER == KGE_ROTATE) ? 0 : lim1;
  const float* arow = (const float*)A.base + index_at(A.idx, i) * A.ld;
  const float* rrow = (const float*)R.base + index_at(R.idx, i) * R.ld;
  const float* trow = (const float*)TG.base + index_at(TG.idx, j) * TG.ld;
  float acc = 0.0f;
  for (int c = 0; c < hh; ++c) {
    const f32x4 a0v{ldf(arow, c, hh), 0, 0, 0}, a1v{ldf(arow + hh, c, lim1), 0, 0, 0};
    f32x4 r0v{ldf(rrow, c, rl0), 0, 0, 0}, r1v{0, 0, 0, 0};
    if (SCORER != KGE_ROTATE) r1v[0] = ldf(rrow + hh, c, rl1);
    f32x4 q0v, q1v;
    build_q4<SCORER>(dir, a0v, a1v, r0v, r1v, q0v, q1v);
    const float t0 = ldf(trow, c, hh), t1 = ldf(trow + hh, c, lim1);
    if (SCORER == KGE_TRANSE) {
      acc = norm_acc<NORM>(acc, __builtin_fabsf(q0v[0] - t0), lp);
      acc = norm_acc<NORM>(acc, __builtin_fabsf(q1v[0] - t1), lp);
    } else {
      const float dre = q0v[0] - t0, dim_ = q1v[0] - t1;
      acc = norm_acc<NORM>(acc, __builtin_sqrtf(__builtin_fmaf(dim_, dim_, dre * dre)), lp);
    }
  }
  return dist_score<NORM>(acc, lp);
}

// One WAVE per row: the scores of the row's CSR entries (64 at a time, one per lane), summed in CSR order, and the
// row's records merged in column-group order.
//   FOLD_KL   lse[i] as ce_dist_merge_kernel; loss_rows[i] = lse - w_i sum (label_weight given: every row) or
//             lse - sum / k_i - log k_i (0 for k_i = 0): kl_combine_kernel's expressions (ce_loss.hip)
//   FOLD_BCE  loss_rows[i] = sum_g rec - sum over the labels of (score + offset)
// A label outside [0, m) is not scored: loss_rows[i] = NaN.
template <int SCORER, int NORM, int FOLD>
__global__ __launch_bounds__(256) void ml_dist_finish_kernel(Operand A, Operand R, Operand TG, int dir, int d, int dr,
                                                             long long n, long long m, float lp,
                                                             const float* __restrict__ rec, int groups,
                                                             const long long* __restrict__ rowptr,
                                                             const long long* __restrict__ col,
                                                             const float* __restrict__ label_weight, float offset,
                                                             float* __restrict__ loss_rows, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const long long b = rowptr[i], e = rowptr[i + 1];
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
        sc = dist_label_score<SCORER, NORM>(A, R, TG, dir, d, dr, i, j, lp);
        if (FOLD == FOLD_BCE) sc += offset;
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
  if (FOLD == FOLD_BCE) {
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

template <int SCORER, int NORM, int FOLD>
static int launch_ml_fwd(bool vec, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr,
                         long long n, long long m, float lp, const long long* rowptr, const long long* col,
                         const float* label_weight, float offset, float* loss_rows, float* lse, float* rec,
                         hipStream_t st) {
  int ct, groups;
  cd_groups(n, m, ct, groups);
  const dim3 grid((unsigned)groups, (unsigned)((n + PT_BM - 1) / PT_BM));
  const Index none{nullptr, 1, KGE_I64};  // (not read by these folds)
  if (vec)
    hipLaunchKernelGGL((ce_dist_fwd_kernel<SCORER, NORM, true, FOLD>), grid, dim3(256), 0, st, A, R, TG, dir, d, dr, n, m, lp,
                       none, ct, groups, rec, offset);
  else
    hipLaunchKernelGGL((ce_dist_fwd_kernel<SCORER, NORM, false, FOLD>), grid, dim3(256), 0, st, A, R, TG, dir, d, dr, n, m,
                       lp, none, ct, groups, rec, offset);
  hipLaunchKernelGGL((ml_dist_finish_kernel<SCORER, NORM, FOLD>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, A, R, TG,
                     dir, d, dr, n, m, lp, rec, groups, rowptr, col, label_weight, offset, loss_rows, lse);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

static inline bool cd_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the vector-load condition of pairs_kernel (score_pairs.hip: pairs_vec_ok) for float32 rows
static bool cd_vec_ok(int scorer, int d, int dr, const Operand& A, const Operand& R, const Operand& TG) {
  if (d % 8) return false;
  if (scorer == KGE_ROTATE && dr != d / 2) return false;
  if (!cd_aligned16(A.base) || !cd_aligned16(R.base) || !cd_aligned16(TG.base)) return false;
  return !((A.ld * 4) % 16 || (R.ld * 4) % 16 || (TG.ld * 4) % 16);
}

int run_ce_dist_fwd(int scorer, float lp, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr,
                    long long n, long long m, const Index& label, float* loss_rows, float* lse, void* ws,
                    long long ws_bytes, hipStream_t st) {
  if (n == 0) return KGE_OK;
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || (scorer != KGE_TRANSE && scorer != KGE_ROTATE)) return KGE_ERR_UNSUPPORTED;
  if (n > 65535LL * PT_BM) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255) || ws_bytes < ce_dist_records_bytes(n, m)) return KGE_ERR_WORKSPACE;
  const bool vec = cd_vec_ok(scorer, d, dr, A, R, TG);
  float* rec = (float*)ws;
#define KGE_CDF(SC, NM) return launch_fwd<SC, NM>(vec, A, R, TG, dir, d, dr, n, m, lp, label, loss_rows, lse, rec, st)
  if (scorer == KGE_TRANSE) {
    if (norm == NORM_L1) KGE_CDF(KGE_TRANSE, NORM_L1);
    KGE_CDF(KGE_TRANSE, NORM_L2);
  }
  if (norm == NORM_L1) KGE_CDF(KGE_ROTATE, NORM_L1);
  KGE_CDF(KGE_ROTATE, NORM_L2);
#undef KGE_CDF
}

// fold: FOLD_KL (lse written, label_weight or NULL) or FOLD_BCE (lse not touched, offset)
int run_ml_dist_fwd(int fold, int scorer, float lp, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                    int dr, long long n, long long m, const long long* rowptr, const long long* col,
                    const float* label_weight, float offset, float* loss_rows, float* lse, void* ws, long long ws_bytes,
                    hipStream_t st) {
  if (n == 0) return KGE_OK;
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || (scorer != KGE_TRANSE && scorer != KGE_ROTATE)) return KGE_ERR_UNSUPPORTED;
  if (n > 65535LL * PT_BM) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255) || ws_bytes < ce_dist_records_bytes(n, m)) return KGE_ERR_WORKSPACE;
  const bool vec = cd_vec_ok(scorer, d, dr, A, R, TG);
  float* rec = (float*)ws;
#define KGE_MLF(SC, NM)                                                                                                  \
  return fold == FOLD_KL ? launch_ml_fwd<SC, NM, FOLD_KL>(vec, A, R, TG, dir, d, dr, n, m, lp, rowptr, col, label_weight, \
                                                          offset, loss_rows, lse, rec, st)                               \
                         : launch_ml_fwd<SC, NM, FOLD_BCE>(vec, A, R, TG, dir, d, dr, n, m, lp, rowptr, col, label_weight, \
                                                           offset, loss_rows, lse, rec, st)
  if (scorer == KGE_TRANSE) {
    if (norm == NORM_L1) KGE_MLF(KGE_TRANSE, NORM_L1);
    KGE_MLF(KGE_TRANSE, NORM_L2);
  }
  if (norm == NORM_L1) KGE_MLF(KGE_ROTATE, NORM_L1);
  KGE_MLF(KGE_ROTATE, NORM_L2);
#undef KGE_MLF
}

// ---- backward -----------------------------------------------------------------------------------------------------
constexpr int CB_TR = 64, CB_TC = 32, CB_KY = 16;

// WHICH == 0: rows = queries [0, n), the reduction runs over this chunk's columns [ybeg, yend) of blockIdx.z's share;
//             the partial dQ is ADDED to dq [n, d] (zeroed by the host before the first chunk).
// WHICH == 1: rows = the chunk's targets (entity col_lo + x), the reduction runs over all n queries in order;
//             g_tgt rows col_lo .. col_lo + mc - 1 are OVERWRITTEN.
// S [n, lds]: the chunk's scores, column y = entity col_lo + y; mc valid columns.
// FOLD_KL / FOLD_BCE: `lse` as before (unused for bce), `label`, `g_rows` and `g_scalar` are not read: ml carries the rows.
template <int SCORER, int NORM, int WHICH, int FOLD>
__global__ __launch_bounds__(256) void ce_dist_bwd_kernel(Operand A, Operand R, Operand TG, int dir, int d, int dr,
                                                          long long n, long long col_lo, long long mc, float lp,
                                                          const float* __restrict__ S, long long lds,
                                                          const float* __restrict__ lse, Index label,
                                                          const float* __restrict__ g_rows, float g_scalar,
                                                          float* __restrict__ dq, float* __restrict__ g_tgt,
                                                          long long ychunk, MlArgs ml) {
  constexpr bool NEED_DIST = NORM != NORM_L1;
  __shared__ float Gs[CB_KY][CB_TR + 4];
  __shared__ float Ds[CB_KY][CB_TR + 4];
  __shared__ float V0[CB_KY][CB_TC + 1];
  __shared__ float V1[CB_KY][CB_TC + 1];

  const int tid = threadIdx.x;
  const int hh = (d + 1) / 2, lim1 = d - hh;
  const int rl0 = (SCORER == KGE_ROTATE) ? dr : hh;
  const int rl1 = (SCORER == KGE_ROTATE) ? 0 : lim1;
  const int c0 = blockIdx.x * CB_TC;
  const long long row0 = (long long)blockIdx.y * CB_TR;
  const long long X = WHICH == 0 ? n : mc, Y = WHICH == 0 ? mc : n;
  const int tx = tid & 15, ty = tid >> 4;

  auto query_pair = [&](long long i, int c, float& q0, float& q1) {
    const float* arow = (const float*)A.base + index_at(A.idx, i) * A.ld;
    const float* rrow = (const float*)R.base + index_at(R.idx, i) * R.ld;
    f32x4 a0v{ldf(arow, c, hh), 0, 0, 0}, a1v{ldf(arow + hh, c, lim1), 0, 0, 0};
    f32x4 r0v{ldf(rrow, c, rl0), 0, 0, 0}, r1v{0, 0, 0, 0};
    if (SCORER != KGE_ROTATE) r1v[0] = ldf(rrow + hh, c, rl1);
    f32x4 q0v, q1v;
    build_q4<SCORER>(dir, a0v, a1v, r0v, r1v, q0v, q1v);
    q0 = q0v[0];
    q1 = q1v[0];
  };
  auto target_pair = [&](long long j, int c, float& t0, float& t1) {  // j: column of the chunk
    const float* trow = (const float*)TG.base + index_at(TG.idx, col_lo + j) * TG.ld;
    t0 = ldf(trow, c, hh);
    t1 = ldf(trow + hh, c, lim1);
  };

  // own-side values for this thread's 4 rows x 2 coordinate pairs
  float own0[4][2], own1[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long x = row0 + ty * 4 + i;
    if (x >= X) x = X - 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + tx * 2 + j;
      if (WHICH == 0) query_pair(x, c, own0[i][j], own1[i][j]);
      else target_pair(x, c, own0[i][j], own1[i][j]);
    }
  }

  float acc0[4][2], acc1[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc0[i][j] = acc1[i][j] = 0.f;

  // the weight of (query i, chunk column y): g_i (softmax_ij - [j == label_i]) from the stored score
  auto weight = [&](long long i, long long y, float& g, float& dist) {
    const float s = S[i * lds + y];
    if (FOLD == FOLD_CE) {
      const float gi = g_rows != nullptr ? g_rows[i] : g_scalar;
      float w = expf(s - lse[i]);
      if (index_at(label, i) == col_lo + y) w -= 1.0f;
      g = gi * w;
    } else {
      // KvsAll: g_i (exp(S_ij - lse_i) - w_i [j in labels_i]) or g_i (sigmoid(S_ij + offset) - [j in labels_i])
      const bool in = (ml.mask[i * ml.maskw + (y >> 5)] >> (y & 31)) & 1u;
      float w = FOLD == FOLD_KL ? expf(s - lse[i]) : 1.0f / (1.0f + expf(-(s + ml.offset)));
      if (in) w -= FOLD == FOLD_KL ? ml.wrow[i] : 1.0f;
      g = ml.grow[i] * w;
    }
    dist = -s;
  };

  const long long ybeg = WHICH == 0 ? (long long)blockIdx.z * ychunk : 0;
  const long long yend = WHICH == 0 ? (ybeg + ychunk < Y ? ybeg + ychunk : Y) : Y;
  for (long long y0 = ybeg; y0 < yend; y0 += CB_KY) {
    // ---- stage the weights (and distances) of this step
    if (WHICH == 0) {
      const int x = tid >> 2, yq = (tid & 3) * 4;
      const long long gx = row0 + x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long gy = y0 + yq + k;
        float g = 0.f, dist = 0.f;
        if (gx < X && gy < yend) weight(gx, gy, g, dist);
        Gs[yq + k][x] = g;
        if (NEED_DIST) Ds[yq + k][x] = dist;
      }
    } else {
      const int y = tid >> 4, xq = (tid & 15) * 4;
      const long long gy = y0 + y;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long gx = row0 + xq + k;
        float g = 0.f, dist = 0.f;
        if (gx < X && gy < yend) weight(gy, gx, g, dist);
        Gs[y][xq + k] = g;
        if (NEED_DIST) Ds[y][xq + k] = dist;
      }
    }
    // ---- stage the other side's vectors: 16 rows x 32 coordinate pairs x 2 halves
    {
      const int y = tid >> 4, cq = (tid & 15) * 2;
      long long gy = y0 + y;
      const bool ok = gy < yend;
      if (!ok) gy = Y - 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = c0 + cq + j;
        float v0, v1;
        if (WHICH == 0) target_pair(gy, c, v0, v1);
        else query_pair(gy, c, v0, v1);
        V0[y][cq + j] = ok ? v0 : 0.f;
        V1[y][cq + j] = ok ? v1 : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int y = 0; y < CB_KY; ++y) {
      float v0[2], v1[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        v0[j] = V0[y][tx * 2 + j];
        v1[j] = V1[y][tx * 2 + j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float g = Gs[y][ty * 4 + i];
        const float dist = NEED_DIST ? Ds[y][ty * 4 + i] : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // e = q - t ; dscore/dq = -w(e), dscore/dt = +w(e)
          const float e0 = WHICH == 0 ? own0[i][j] - v0[j] : v0[j] - own0[i][j];
          const float e1 = WHICH == 0 ? own1[i][j] - v1[j] : v1[j] - own1[i][j];
          const float sg = WHICH == 0 ? -g : g;
          if (SCORER == KGE_TRANSE) {
            acc0[i][j] = __builtin_fmaf(sg, transe_w<NORM>(e0, dist, lp), acc0[i][j]);
            acc1[i][j] = __builtin_fmaf(sg, transe_w<NORM>(e1, dist, lp), acc1[i][j]);
          } else {
            float wre, wim;
            rotate_w<NORM>(e0, e1, dist, lp, wre, wim);
            acc0[i][j] = __builtin_fmaf(sg, wre, acc0[i][j]);
            acc1[i][j] = __builtin_fmaf(sg, wim, acc1[i][j]);
          }
        }
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long x = row0 + ty * 4 + i;
    if (x >= X) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + tx * 2 + j;
      if (c >= hh) continue;
      const bool has1 = c < lim1;
      if (WHICH == 1) {
        float* o = g_tgt + (col_lo + x) * d;
        o[c] = acc0[i][j];
        if (has1) o[hh + c] = acc1[i][j];
      } else {
        unsafeAtomicAdd(dq + x * d + c, acc0[i][j]);
        if (has1) unsafeAtomicAdd(dq + x * d + hh + c, acc1[i][j]);
      }
    }
  }
}

// dQ [n, d] -> the gradients of the gathered entity row (g_a [n, d]) and relation row (g_p [n, dr]) of every query:
// the epilogue of bwd_pairs_kernel (bwd.hip), once, after the last chunk.  One thread per (row, coordinate pair).
template <int SCORER>
__global__ __launch_bounds__(256) void ce_dist_chain_kernel(Operand A, Operand R, int dir, int d, int dr, long long n,
                                                            const float* __restrict__ dq, float* __restrict__ g_a,
                                                            float* __restrict__ g_p) {
  const int hh = (d + 1) / 2, lim1 = d - hh;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * hh) return;
  const long long x = idx / hh;
  const int c = (int)(idx - x * hh);
  const bool has1 = c < lim1;
  const float dq0 = dq[x * d + c], dq1 = has1 ? dq[x * d + hh + c] : 0.f;
  float da0, da1, dr0, dr1 = 0.f;
  if (SCORER == KGE_TRANSE) {
    da0 = dq0; da1 = dq1;
    dr0 = dir == KGE_SP_ ? dq0 : -dq0;
    dr1 = dir == KGE_SP_ ? dq1 : -dq1;
  } else {  // ROTATE: the relation row holds phases
    const float* arow = (const float*)A.base + index_at(A.idx, x) * A.ld;
    const float* rrow = (const float*)R.base + index_at(R.idx, x) * R.ld;
    const f32x4 a0v{arow[c], 0, 0, 0}, a1v{arow[hh + c], 0, 0, 0}, r0v{rrow[c], 0, 0, 0};
    f32x4 q0v, q1v;
    build_q4<KGE_ROTATE>(dir, a0v, a1v, r0v, r0v, q0v, q1v);
    const float q0 = q0v[0], q1 = q1v[0];
    float sn, cs;
    sincos_canon(r0v[0], sn, cs);
    if (dir == KGE_SP_) {
      da0 = dq0 * cs + dq1 * sn; da1 = dq1 * cs - dq0 * sn;
      dr0 = dq1 * q0 - dq0 * q1;
    } else {
      da0 = dq0 * cs - dq1 * sn; da1 = dq0 * sn + dq1 * cs;
      dr0 = dq0 * q1 - dq1 * q0;
    }
  }
  g_a[x * d + c] = da0;
  if (has1) g_a[x * d + hh + c] = da1;
  g_p[x * dr + c] = dr0;
  if (SCORER != KGE_ROTATE && has1) g_p[x * dr + hh + c] = dr1;
}

template <int SCORER, int NORM, int FOLD>
static int launch_bwd_chunk(const Operand& A, const Operand& R, const Operand& TGall, int dir, int d, int dr, long long n,
                            long long col_lo, long long mc, float lp, const float* S, long long lds, const float* lse,
                            const Index& label, const float* g_rows, float g_scalar, float* dq, float* g_tgt,
                            hipStream_t st, const MlArgs& ml) {
  const int hh = (d + 1) / 2;
  const unsigned gc = (unsigned)((hh + CB_TC - 1) / CB_TC);
  const unsigned gr = (unsigned)((n + CB_TR - 1) / CB_TR);
  // query side: the chunk's columns split over blockIdx.z until ~1024 workgroups exist
  long long ys = 1024 / ((long long)gc * gr);
  if (ys > 64) ys = 64;
  if (ys < 1) ys = 1;
  long long ychunk = ((mc + ys - 1) / ys + CB_KY - 1) / CB_KY * CB_KY;
  ys = (mc + ychunk - 1) / ychunk;
  hipLaunchKernelGGL((ce_dist_bwd_kernel<SCORER, NORM, 0, FOLD>), dim3(gc, gr, (unsigned)ys), dim3(256), 0, st, A, R, TGall,
                     dir, d, dr, n, col_lo, mc, lp, S, lds, lse, label, g_rows, g_scalar, dq, g_tgt, ychunk, ml);
  hipLaunchKernelGGL((ce_dist_bwd_kernel<SCORER, NORM, 1, FOLD>), dim3(gc, (unsigned)((mc + CB_TR - 1) / CB_TR)), dim3(256),
                     0, st, A, R, TGall, dir, d, dr, n, col_lo, mc, lp, S, lds, lse, label, g_rows, g_scalar, dq, g_tgt,
                     (long long)n, ml);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// ---- KvsAll: the rows' g_i / w_i and the chunk's label bits -----------------------------------------------------------
// grow[i] = the upstream gradient of row i (0 for a row without labels under the unweighted kl loss: its loss is the
// constant 0), wrow[i] = label_weight[i] or 1 / k_i (kl only).
__global__ __launch_bounds__(256) void ml_rows_kernel(long long n, const long long* __restrict__ rowptr,
                                                      const float* __restrict__ label_weight, int fold,
                                                      const float* __restrict__ g_rows, float g_scalar,
                                                      float* __restrict__ grow, float* __restrict__ wrow) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float gi = g_rows != nullptr ? g_rows[i] : g_scalar;
  float w = 1.0f;
  if (fold == FOLD_KL) {
    const long long k = rowptr[i + 1] - rowptr[i];
    if (label_weight != nullptr) w = label_weight[i];
    else if (k > 0) w = 1.0f / (float)k;
    else gi = 0.0f;
  }
  grow[i] = gi;
  wrow[i] = w;
}

// One wave per row: bit (i, j - col_lo) of the mask for every CSR entry (i, j) with col_lo <= j < col_lo + mc.  Labels
// outside the chunk -- outside [0, m) among them -- set nothing.
__global__ __launch_bounds__(256) void ml_mask_kernel(long long n, const long long* __restrict__ rowptr,
                                                      const long long* __restrict__ col, long long col_lo, long long mc,
                                                      unsigned int* __restrict__ mask, long long maskw) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long long e = rowptr[i + 1];
  for (long long x = rowptr[i] + lane; x < e; x += 64) {
    const long long y = col[x] - col_lo;
    if (y < 0 || y >= mc) continue;
    atomicOr(mask + i * maskw + (y >> 5), 1u << (y & 31));
  }
}

// The chunk loop of both losses.  fold == FOLD_CE: label / g_rows / g_scalar; else the CSR, label_weight and offset.
// TG: ALL rows of the entity table (identity index)
static int run_dist_bwd(int fold, int scorer, float lp, const Operand& A, const Operand& R, const Operand& TG, int dir,
                        int d, int dr, long long n, long long m, const Index& label, const long long* rowptr,
                        const long long* col, const float* label_weight, float offset, const float* lse,
                        const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt, void* ws,
                        long long ws_bytes, hipStream_t st) {
  if (n == 0) {  // no query: the entity rows get a zero gradient
    return fill_words_async(g_tgt, 0, (size_t)m * d * sizeof(float), st) ? KGE_OK : KGE_ERR_LAUNCH;
  }
  const int norm = norm_mode(lp);
  if (norm == NORM_LP || (scorer != KGE_TRANSE && scorer != KGE_ROTATE)) return KGE_ERR_UNSUPPORTED;
  if (n > 65535LL * CB_TR) return KGE_ERR_UNSUPPORTED;
  if (!ws || ((uintptr_t)ws & 255)) return KGE_ERR_WORKSPACE;
  const long long C = fold == FOLD_CE ? ce_dist_chunk_cols(n, m, d, ws_bytes) : ml_dist_chunk_cols(n, m, d, ws_bytes);
  if (C < 64) return KGE_ERR_WORKSPACE;
  if (C > 65535LL * CB_TR) return KGE_ERR_UNSUPPORTED;
  float* dq = (float*)((char*)ws + ce_dist_records_bytes(n, m));
  float* S = (float*)((char*)dq + ce_dist_dq_bytes(n, d));
  MlArgs ml{};
  unsigned int* mask = nullptr;
  const size_t mask_bytes = (size_t)(n * C / 8);
  if (fold != FOLD_CE) {
    mask = (unsigned int*)((char*)S + cd_align(4 * n * C));
    float* rows = (float*)ws;  // (where the forward's records were)
    ml = MlArgs{mask, C / 32, rows, rows + n, offset};
    hipLaunchKernelGGL(ml_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr, label_weight, fold,
                       g_rows, g_scalar, rows, rows + n);
  }
  if (!fill_words_async(dq, 0, (size_t)n * d * sizeof(float), st)) return KGE_ERR_LAUNCH;
  for (long long lo = 0; lo < m; lo += C) {
    const long long mc = m - lo < C ? m - lo : C;
    const Operand TGc{(const char*)TG.base + lo * TG.ld * (long long)sizeof(float), TG.ld, Index{nullptr, 1, KGE_I64}};
    int rc = run_pairs_exact(scorer, KGE_F32, false, A, R, TGc, dir, d, dr, n, mc, lp, S, C, st, true);
    if (rc != KGE_OK) return rc;
    if (fold != FOLD_CE) {
      if (!fill_words_async(mask, 0, mask_bytes, st)) return KGE_ERR_LAUNCH;
      hipLaunchKernelGGL(ml_mask_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, rowptr, col, lo, mc, mask,
                         C / 32);
    }
#define KGE_CDB(SC, NM)                                                                                                   \
  rc = fold == FOLD_CE   ? launch_bwd_chunk<SC, NM, FOLD_CE>(A, R, TG, dir, d, dr, n, lo, mc, lp, S, C, lse, label, g_rows, \
                                                             g_scalar, dq, g_tgt, st, ml)                                 \
       : fold == FOLD_KL ? launch_bwd_chunk<SC, NM, FOLD_KL>(A, R, TG, dir, d, dr, n, lo, mc, lp, S, C, lse, label, g_rows, \
                                                             g_scalar, dq, g_tgt, st, ml)                                 \
                         : launch_bwd_chunk<SC, NM, FOLD_BCE>(A, R, TG, dir, d, dr, n, lo, mc, lp, S, C, lse, label, g_rows, \
                                                              g_scalar, dq, g_tgt, st, ml)
    if (scorer == KGE_TRANSE) {
      if (norm == NORM_L1) KGE_CDB(KGE_TRANSE, NORM_L1);
      else KGE_CDB(KGE_TRANSE, NORM_L2);
    } else {
      if (norm == NORM_L1) KGE_CDB(KGE_ROTATE, NORM_L1);
      else KGE_CDB(KGE_ROTATE, NORM_L2);
    }
#undef KGE_CDB
    if (rc != KGE_OK) return rc;
  }
  // (the mask is left all-zero: a workspace handed on holds no label of this call)
  if (fold != FOLD_CE && !fill_words_async(mask, 0, mask_bytes, st)) return KGE_ERR_LAUNCH;
  const long long cells = n * ((d + 1) / 2);
  const dim3 cgrid((unsigned)((cells + 255) / 256));
  if (scorer == KGE_TRANSE)
    hipLaunchKernelGGL((ce_dist_chain_kernel<KGE_TRANSE>), cgrid, dim3(256), 0, st, A, R, dir, d, dr, n, dq, g_a, g_p);
  else
    hipLaunchKernelGGL((ce_dist_chain_kernel<KGE_ROTATE>), cgrid, dim3(256), 0, st, A, R, dir, d, dr, n, dq, g_a, g_p);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

int run_ce_dist_bwd(int scorer, float lp, const Operand& A, const Operand& R, const Operand& TG, int dir, int d, int dr,
                    long long n, long long m, const Index& label, const float* lse, const float* g_rows, float g_scalar,
                    float* g_a, float* g_p, float* g_tgt, void* ws, long long ws_bytes, hipStream_t st) {
  return run_dist_bwd(FOLD_CE, scorer, lp, A, R, TG, dir, d, dr, n, m, label, nullptr, nullptr, nullptr, 0.0f, lse, g_rows,
                      g_scalar, g_a, g_p, g_tgt, ws, ws_bytes, st);
}

// fold: FOLD_KL (lse, label_weight or NULL) or FOLD_BCE (offset)
int run_ml_dist_bwd(int fold, int scorer, float lp, const Operand& A, const Operand& R, const Operand& TG, int dir, int d,
                    int dr, long long n, long long m, const long long* rowptr, const long long* col,
                    const float* label_weight, float offset, const float* lse, const float* g_rows, float g_scalar,
                    float* g_a, float* g_p, float* g_tgt, void* ws, long long ws_bytes, hipStream_t st) {
  return run_dist_bwd(fold, scorer, lp, A, R, TG, dir, d, dr, n, m, Index{nullptr, 1, KGE_I64}, rowptr, col, label_weight,
                      offset, lse, g_rows, g_scalar, g_a, g_p, g_tgt, ws, ws_bytes, st);
}

}  // namespace kge
