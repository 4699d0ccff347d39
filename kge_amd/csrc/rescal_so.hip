// rescal_so.hip -- relation prediction for RESCAL: KgeModel.score_so (kge_model.py:727-747) on the float32 matrix
// pipe, gfx950.  Reached through kge_score_so / kge_score_so_bwd_accum by tables that carry KGE_FLAG_RESCAL_GROUPED.
//
//   score[i, j] = s_i^T M_{r_j} o_i = < vec(s_i o_i^T), vec(M_{r_j}) >
//
// a GEMM C[n, m] = A[n, d^2] B[m, d^2]^T whose left operand is never stored: row i of A is the outer product of two
// entity rows, formed in registers in the lane layout of v_mfma_f32_16x16x4_f32 as fl(s_i[a] * o_i[b]) -- one multiply,
// one rounding.  B is the relation table as it lies in memory.  The reference composes the call from three repeats to
// [n m, .] rows (kge_model.py:202-209): the relation operand alone is n m d^2 floats.
//
// NOT bit-equal to kge_score_spo, which computes (M^T s) . o: the same real number in another association.  What holds
// is the float64 bound of tests/_rescal_so_ref.py.
//
// Forward (rso_fwd_kernel).  A workgroup owns 64 pairs x 32 relations x one K split of 32 slices; slice a = row a of
// every M_r, d contiguous floats.  Wave w owns pairs [16 w, 16 w + 16) and both 16-relation sub-tiles (two accumulators:
// one A fragment feeds two MFMAs).  The tile's o rows (all of them) and s rows (the split's 32 coordinates) are gathered
// once into LDS.  Per slice the 32 relation rows go global -> registers -> LDS in 16-byte pieces (an element path where
// rows are not 16-byte aligned or d % 4 != 0), the loads of slice a + 1 in flight under the MFMAs of slice a.
// K ORDER of one score: splits z = 0, 1, .. of 32 slices each; inside a split acc = +0, slices a ascending; inside a
// slice groups of 16 columns ascending; inside a group four MFMAs c = 0..3, MFMA c contracting b = 16 g + 4 q + c for
// q = 0..3 (lane quarter q reads ONE 16-byte piece of o and of each relation row per group); columns behind d are zero
// on both sides.  The splits' partial sums go to the workspace and rso_reduce_kernel adds them in ascending z.  No
// atomics: a score depends on its three rows, d and this order -- not on n, m, the tile position, index form or pitch.
//
// Backward (kge_score_so_bwd_accum), g = gout [n, m]:
//   rso_relgrad_kernel  g_M[r_j] += sum_i g[i, j] s_i o_i^T = g^T [m, n] A [n, d^2], A formed on the fly as above.  A
//     workgroup owns 16 relations x 4 slices (one per wave) x 64 columns and walks ALL pairs in ascending order, four
//     per MFMA: every output has one owner.  rels == NULL: grad_rel = grad_rel + acc, plain; a listed rels may repeat a
//     relation: atomic adds.
//   rso_entgrad_kernel  W_i = sum_j g[i, j] M_{r_j} over a tile of 32 relations, one slice W_i[a, :] at a time in the
//     accumulators of the wave that owns a (a = wave, wave + 4, ..), contracted there: g_s[i][a] = W_i[a, :] . o_i
//     (lane products, a 16-lane butterfly), g_o[i][:] += s_i[a] W_i[a, :] (registers).  W never leaves the registers.
//     The waves' g_o are added in LDS in wave order; one atomic row add of g_s and of g_o per (pair, tile).
#include "common.hpp"

namespace kge {

constexpr int RSO_TN = 64;      // forward: pairs per workgroup
constexpr int RSO_TM = 32;      // forward: relations per workgroup
constexpr int RSO_KA = 32;      // forward: slices per K split
constexpr int RSO_PIECES = 8;   // 16-byte pieces of a staged slice per thread: 32 rows x 64 pieces / 256 threads
constexpr int RSO_BP = 64;      // relation gradient: pairs staged per round
constexpr int RSO_TI = 16;      // entity gradient: pairs per workgroup
constexpr int RSO_TJ = 32;      // entity gradient: relations per workgroup

static_assert(KGE_RESCAL_MAX_DIM <= 256, "RSO_PIECES and the four column blocks of rso_entgrad_kernel assume d <= 256");

struct RsoFwd {
  Operand S, R, O;
  int d;
  long long n, m;
  float* out;              // the scores, or the first split's partial sums
  long long ldo;
  long long split_stride;  // floats between the partial sums of two splits
};

__device__ __forceinline__ f32x4 rso_zero4() { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

template <bool VEC>
__global__ __launch_bounds__(256) void rso_fwd_kernel(RsoFwd p) {
  extern __shared__ __attribute__((aligned(16))) float rso_smem[];
  __shared__ long long sRow[RSO_TM], sSid[RSO_TN], sOid[RSO_TN];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int d = p.d, dp = (d + 15) & ~15, pitch = dp + 4, ppr = dp >> 2;
  float* sO = rso_smem;                 // [RSO_TN][pitch], zero behind d and behind the last pair
  float* sB = sO + RSO_TN * pitch;      // [RSO_TM][pitch]: the slice of the tile's relations
  float* sS = sB + RSO_TM * pitch;      // [RSO_TN][RSO_KA + 1]: the split's coordinates of the s rows
  const long long j0 = (long long)blockIdx.x * RSO_TM, i0 = (long long)blockIdx.y * RSO_TN;
  const int a0 = blockIdx.z * RSO_KA;
  const int a1 = a0 + RSO_KA < d ? a0 + RSO_KA : d;
  const int ncol = (int)(p.m - j0 < RSO_TM ? p.m - j0 : RSO_TM);
  const int nrow = (int)(p.n - i0 < RSO_TN ? p.n - i0 : RSO_TN);
  const float* ent = (const float*)p.S.base;  // S.base == O.base: the entity table
  const float* rel = (const float*)p.R.base;

  if (tid < RSO_TM) sRow[tid] = tid < ncol ? index_at(p.R.idx, j0 + tid) : -1;
  if (tid >= 64 && tid < 64 + RSO_TN) {
    const int r = tid - 64;
    sSid[r] = r < nrow ? index_at(p.S.idx, i0 + r) : -1;
    sOid[r] = r < nrow ? index_at(p.O.idx, i0 + r) : -1;
  }
  __syncthreads();
  for (int e = tid; e < RSO_TN * pitch; e += 256) {
    const int r = e / pitch, c = e - r * pitch;
    sO[e] = (sOid[r] >= 0 && c < d) ? ent[sOid[r] * p.O.ld + c] : 0.0f;
  }
  for (int e = tid; e < RSO_TN * RSO_KA; e += 256) {
    const int r = e / RSO_KA, c = e - r * RSO_KA;
    sS[r * (RSO_KA + 1) + c] = (sSid[r] >= 0 && a0 + c < d) ? ent[sSid[r] * p.S.ld + a0 + c] : 0.0f;
  }

  // slice a of the tile's relation rows, piece tid + 256 k = (row, 16-byte piece of the row): zero behind d and m
  f32x4 buf[RSO_PIECES];
  auto load_slice = [&](int a) {
#pragma unroll
    for (int k = 0; k < RSO_PIECES; ++k) {
      const int idx = tid + 256 * k;
      f32x4 v = rso_zero4();
      if (idx < RSO_TM * ppr) {
        const int r = idx / ppr, q = idx - r * ppr;
        const long long row = sRow[r];
        if (row >= 0 && 4 * q < d) {
          const float* src = rel + row * p.R.ld + (long long)a * d + 4 * q;
          if (VEC) {
            v = *reinterpret_cast<const f32x4*>(src);
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (4 * q + c < d) v[c] = src[c];
          }
        }
      }
      buf[k] = v;
    }
  };
  load_slice(a0);

  const bool live = wave * 16 < nrow;  // (wave-uniform) a wave behind the last pair issues no MFMA
  const bool two = ncol > 16;          // (workgroup-uniform) the second relation sub-tile holds a column
  const float* myO = sO + (wave * 16 + lr) * pitch + 4 * lq;
  const float* myS = sS + (wave * 16 + lr) * (RSO_KA + 1);
  const float* myB = sB + lr * pitch + 4 * lq;
  f32x4 acc0 = rso_zero4(), acc1 = rso_zero4();
  for (int a = a0; a < a1; ++a) {
    __syncthreads();  // the gathers are complete; the previous slice is consumed
#pragma unroll
    for (int k = 0; k < RSO_PIECES; ++k) {
      const int idx = tid + 256 * k;
      if (idx < RSO_TM * ppr) {
        const int r = idx / ppr, q = idx - r * ppr;
        *reinterpret_cast<f32x4*>(sB + r * pitch + 4 * q) = buf[k];
      }
    }
    __syncthreads();
    if (a + 1 < a1) load_slice(a + 1);
    if (live) {
      const float sv = myS[a - a0];
      for (int g = 0; g < dp; g += 16) {
        const f32x4 o4 = *reinterpret_cast<const f32x4*>(myO + g);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(myB + g);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(sv * o4[c], b0[c], acc0, 0, 0, 0);
        if (two) {
          const f32x4 b1 = *reinterpret_cast<const f32x4*>(myB + 16 * pitch + g);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(sv * o4[c], b1[c], acc1, 0, 0, 0);
        }
      }
    }
  }
  // acc[jj] = C[pair = 4 lq + jj][relation = lr]
  float* dst = p.out + (long long)blockIdx.z * p.split_stride;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int r = wave * 16 + 4 * lq + jj;
    if (r < nrow) {
      if (lr < ncol) dst[(i0 + r) * p.ldo + j0 + lr] = acc0[jj];
      if (16 + lr < ncol) dst[(i0 + r) * p.ldo + j0 + 16 + lr] = acc1[jj];
    }
  }
}

// out[i, j] = ((ws[0] + ws[1]) + ws[2]) + ..: the K splits' partial sums ([ks][n][m]) in ascending order
__global__ __launch_bounds__(256) void rso_reduce_kernel(const float* __restrict__ ws, int ks, long long n, long long m,
                                                         float* __restrict__ out, long long ldo) {
  const long long total = n * m, stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    float v = ws[e];
    for (int z = 1; z < ks; ++z) v = v + ws[z * total + e];
    out[(e / m) * ldo + e % m] = v;
  }
}

static int rso_splits(int d) { return (d + RSO_KA - 1) / RSO_KA; }

// kge_score_so_workspace_bytes for a RESCAL table: the partial sums of the K splits (d <= 32: one split, none)
long long rescal_so_workspace_bytes(int d, long long n, long long m) {
  const int ks = rso_splits(d);
  return ks > 1 ? (long long)ks * n * m * (long long)sizeof(float) : 0;
}

// the shapes both directions take (KGE_ERR_UNSUPPORTED before any launch otherwise)
bool rescal_so_shape_ok(long long n, long long m) {
  return n <= 65535LL * RSO_TN && m <= 65535LL * RSO_TJ;
}

// kge_score_so, n > 0 and m > 0; ws: rescal_so_workspace_bytes
int run_rescal_so(const Operand& S, const Operand& R, const Operand& O, int d, long long n, long long m, float* out,
                  long long ldo, void* ws, hipStream_t st) {
  if (!rescal_so_shape_ok(n, m)) return KGE_ERR_UNSUPPORTED;
  const int ks = rso_splits(d), dp = (d + 15) & ~15;
  const bool vec = d % 4 == 0 && R.ld % 4 == 0 && ((uintptr_t)R.base & 15) == 0;
  const size_t lds_bytes = ((size_t)(RSO_TN + RSO_TM) * (dp + 4) + RSO_TN * (RSO_KA + 1)) * sizeof(float);
  auto kern = vec ? rso_fwd_kernel<true> : rso_fwd_kernel<false>;
  if (lds_bytes > 48 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return KGE_ERR_UNSUPPORTED;
    }
  }
  RsoFwd p = {S, R, O, d, n, m, ks > 1 ? (float*)ws : out, ks > 1 ? m : ldo, n * m};
  const dim3 grid((unsigned)((m + RSO_TM - 1) / RSO_TM), (unsigned)((n + RSO_TN - 1) / RSO_TN), (unsigned)ks);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, st, p);
  if (ks > 1) {
    long long blocks = (n * m + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rso_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)ws, ks, n, m, out, ldo);
  }
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// ---- backward -------------------------------------------------------------------------------------------------------
struct RsoBwd {
  Operand S, R, O;
  int d;
  long long n, m;
  const float* gout;
  long long ldg;
  float* ge;
  long long ge_ld;
  float* gr;
  long long gr_ld;
};

// grid.x = tile of 16 relations, grid.y = (group of 4 slices, block of 64 columns).  Wave w owns slice 4 ag + w.
// One chain per element: acc = +0, one MFMA per four pairs in ascending pair order (zero rows behind n).
template <bool ATOMIC>
__global__ __launch_bounds__(256) void rso_relgrad_kernel(RsoBwd p) {
  __shared__ float sG[RSO_BP][17];  // g[pair][relation]
  __shared__ float sO[RSO_BP][65];  // the block's columns of the o rows
  __shared__ float sS[RSO_BP][4];   // the group's coordinates of the s rows
  __shared__ long long sRow[16], sSid[RSO_BP], sOid[RSO_BP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int d = p.d, nb = (d + 63) / 64;
  const long long j0 = (long long)blockIdx.x * 16;
  const int ag = blockIdx.y / nb, b0 = (blockIdx.y % nb) * 64;
  const int a = 4 * ag + wave;
  const int ncol = (int)(p.m - j0 < 16 ? p.m - j0 : 16);
  const float* ent = (const float*)p.S.base;
  if (tid < 16) sRow[tid] = tid < ncol ? index_at(p.R.idx, j0 + tid) : -1;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = rso_zero4();
  for (long long i0 = 0; i0 < p.n; i0 += RSO_BP) {
    const int here = (int)(p.n - i0 < RSO_BP ? p.n - i0 : RSO_BP);
    __syncthreads();  // the previous round is consumed
    if (tid < RSO_BP) {
      sSid[tid] = tid < here ? index_at(p.S.idx, i0 + tid) : -1;
      sOid[tid] = tid < here ? index_at(p.O.idx, i0 + tid) : -1;
    }
    __syncthreads();
    for (int e = tid; e < RSO_BP * 16; e += 256) {
      const int r = e >> 4, c = e & 15;
      sG[r][c] = (r < here && c < ncol) ? p.gout[(i0 + r) * p.ldg + j0 + c] : 0.0f;
    }
    for (int e = tid; e < RSO_BP * 64; e += 256) {
      const int r = e >> 6, c = e & 63;
      sO[r][c] = (r < here && b0 + c < d) ? ent[sOid[r] * p.O.ld + b0 + c] : 0.0f;
    }
    {
      const int r = tid >> 2, c = tid & 3;
      sS[r][c] = (r < here && 4 * ag + c < d) ? ent[sSid[r] * p.S.ld + 4 * ag + c] : 0.0f;
    }
    __syncthreads();
    if (a < d) {  // (wave-uniform)
      for (int kk = 0; kk < here; kk += 4) {
        const float av = sG[kk + lq][lr];  // A[relation lr][pair kk + lq]
        const float sv = sS[kk + lq][wave];
#pragma unroll
        for (int t = 0; t < 4; ++t)  // B[pair kk + lq][column 16 t + lr] = fl(s_a o_b)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sv * sO[kk + lq][16 * t + lr], acc[t], 0, 0, 0);
      }
    }
  }
  // acc[t][jj] = C[relation 4 lq + jj][column 16 t + lr]
  if (a >= d) return;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int r = 4 * lq + jj;
    if (r >= ncol) continue;
    float* dst = p.gr + sRow[r] * p.gr_ld + (long long)a * d;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int b = b0 + 16 * t + lr;
      if (b < d) {
        if (ATOMIC) unsafeAtomicAdd(dst + b, acc[t][jj]);
        else dst[b] = dst[b] + acc[t][jj];
      }
    }
  }
}

// grid.x = tile of 16 pairs, grid.y = tile of 32 relations.  NBB = blocks of 64 columns of a slice.
template <int NBB>
__global__ __launch_bounds__(256) void rso_entgrad_kernel(RsoBwd p) {
  extern __shared__ __attribute__((aligned(16))) float rso_smem[];
  __shared__ float sG[RSO_TI][RSO_TJ + 1];  // g[pair][relation]
  __shared__ long long sRow[RSO_TJ], sSid[RSO_TI], sOid[RSO_TI];
  constexpr int PO = NBB * 64 + 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int d = p.d;
  float* sO = rso_smem;              // [RSO_TI][PO], zero behind d
  float* sS = sO + RSO_TI * PO;      // [RSO_TI][d]
  float* sGS = sS + RSO_TI * d;      // [RSO_TI][d]: g_s of the tile
  float* sGO = sGS + RSO_TI * d;     // [RSO_TI][d]: g_o of the tile
  const long long i0 = (long long)blockIdx.x * RSO_TI, j0 = (long long)blockIdx.y * RSO_TJ;
  const int nrow = (int)(p.n - i0 < RSO_TI ? p.n - i0 : RSO_TI);
  const int ncol = (int)(p.m - j0 < RSO_TJ ? p.m - j0 : RSO_TJ);
  const float* ent = (const float*)p.S.base;
  const float* rel = (const float*)p.R.base;
  if (tid < RSO_TJ) sRow[tid] = tid < ncol ? index_at(p.R.idx, j0 + tid) : -1;
  if (tid >= 64 && tid < 64 + RSO_TI) {
    const int r = tid - 64;
    sSid[r] = r < nrow ? index_at(p.S.idx, i0 + r) : -1;
    sOid[r] = r < nrow ? index_at(p.O.idx, i0 + r) : -1;
  }
  __syncthreads();
  for (int e = tid; e < RSO_TI * RSO_TJ; e += 256) {
    const int r = e / RSO_TJ, c = e - r * RSO_TJ;
    sG[r][c] = (r < nrow && c < ncol) ? p.gout[(i0 + r) * p.ldg + j0 + c] : 0.0f;
  }
  for (int e = tid; e < RSO_TI * PO; e += 256) {
    const int r = e / PO, c = e - r * PO;
    sO[e] = (r < nrow && c < d) ? ent[sOid[r] * p.O.ld + c] : 0.0f;
  }
  for (int e = tid; e < RSO_TI * d; e += 256) {
    const int r = e / d, c = e - r * d;
    sS[e] = r < nrow ? ent[sSid[r] * p.S.ld + c] : 0.0f;
  }
  __syncthreads();

  f32x4 go[NBB][4];  // go[bb][t][jj]: g_o[pair 4 lq + jj][column 64 bb + 16 t + lr] over this wave's slices
#pragma unroll
  for (int bb = 0; bb < NBB; ++bb)
#pragma unroll
    for (int t = 0; t < 4; ++t) go[bb][t] = rso_zero4();
  for (int a = wave; a < d; a += 4) {
    float gs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sv[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) sv[jj] = sS[(4 * lq + jj) * d + a];
#pragma unroll
    for (int bb = 0; bb < NBB; ++bb) {
      f32x4 acc[4];  // W[pair 4 lq + jj][a, column 64 bb + 16 t + lr]
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = rso_zero4();
#pragma unroll
      for (int kk = 0; kk < RSO_TJ; kk += 4) {  // (all 32 loads of a block in flight: zero rows behind the last relation)
        const float av = sG[lr][kk + lq];  // A[pair lr][relation kk + lq]
        const long long row = sRow[kk + lq];
        const float* src = rel + (row < 0 ? 0 : row) * p.R.ld + (long long)a * d;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int b = bb * 64 + 16 * t + lr;
          const float bv = (row >= 0 && b < d) ? src[b] : 0.0f;  // B[relation kk + lq][column b]
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int b = bb * 64 + 16 * t + lr;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          gs[jj] = __builtin_fmaf(acc[t][jj], sO[(4 * lq + jj) * PO + b], gs[jj]);
          go[bb][t][jj] = __builtin_fmaf(sv[jj], acc[t][jj], go[bb][t][jj]);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) gs[jj] = gs[jj] + __shfl_xor(gs[jj], off, 64);
      if (lr == 0) sGS[(4 * lq + jj) * d + a] = gs[jj];
    }
  }
  // the waves' g_o, added in wave order
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int bb = 0; bb < NBB; ++bb)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int b = bb * 64 + 16 * t + lr;
          if (b < d) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              float* q = sGO + (4 * lq + jj) * d + b;
              *q = w == 0 ? go[bb][t][jj] : *q + go[bb][t][jj];
            }
          }
        }
    }
    __syncthreads();
  }
  // one atomic row add of each gradient per (pair, tile)
  for (int e = tid; e < nrow * d; e += 256) {
    const int r = e / d, c = e - r * d;
    unsafeAtomicAdd(p.ge + sSid[r] * p.ge_ld + c, sGS[e]);
    unsafeAtomicAdd(p.ge + sOid[r] * p.ge_ld + c, sGO[e]);
  }
}

template <int NBB>
static int rso_launch_entgrad(const RsoBwd& p, hipStream_t st) {
  const size_t lds_bytes = ((size_t)RSO_TI * (NBB * 64 + 1) + 3 * (size_t)RSO_TI * p.d) * sizeof(float);
  auto kern = rso_entgrad_kernel<NBB>;
  if (lds_bytes > 48 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return KGE_ERR_UNSUPPORTED;
    }
  }
  const dim3 grid((unsigned)((p.n + RSO_TI - 1) / RSO_TI), (unsigned)((p.m + RSO_TJ - 1) / RSO_TJ));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, st, p);
  return KGE_OK;
}

// kge_score_so_bwd_accum, n > 0 and m > 0
int run_rescal_so_bwd_accum(const Operand& S, const Operand& R, const Operand& O, int d, long long n, long long m,
                            const float* gout, long long ldg, float* ge, long long ge_ld, float* gr, long long gr_ld,
                            hipStream_t st) {
  if (!rescal_so_shape_ok(n, m) || d > 256) return KGE_ERR_UNSUPPORTED;
  const RsoBwd p = {S, R, O, d, n, m, gout, ldg, ge, ge_ld, gr, gr_ld};
  const int nb = (d + 63) / 64;
  const dim3 grid((unsigned)((m + 15) / 16), (unsigned)(((d + 3) / 4) * nb));
  if (R.idx.ptr) hipLaunchKernelGGL(rso_relgrad_kernel<true>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(rso_relgrad_kernel<false>, grid, dim3(256), 0, st, p);
  int rc = KGE_OK;
  switch (nb) {
    case 1: rc = rso_launch_entgrad<1>(p, st); break;
    case 2: rc = rso_launch_entgrad<2>(p, st); break;
    case 3: rc = rso_launch_entgrad<3>(p, st); break;
    default: rc = rso_launch_entgrad<4>(p, st); break;
  }
  if (rc != KGE_OK) return rc;
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
