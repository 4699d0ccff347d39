// tucker3.hip -- the relation projection of relational_tucker3 (kge/model/embedder/tucker3_relation_embedder.py) on
// gfx950: M_p = (B[p] @ W^T).view(d, d), float32 (tucker3_device.hpp).  The projected rows are a
// KGE_RESCAL relation table: everything behind the projection is rescal.hip.
//
//   tucker3_project_kernel  kge_tucker3_project: out[n, d^2] = B[idx] * W^T, an NT product (both operands K-contiguous,
//                           K = d_r small and ragged, N = d^2 large).  VALU, not the matrix cores: one WRITTEN fma chain
//                           per element is the canonical arithmetic (the same bits from any tile, lane and load path),
//                           which the rounding inside an MFMA is not.  Measured: 0.75 - 1.24 TB/s of
//                           stores at the FB15k-237 shape -- bound by VALU issue and LDS reads, not by writing `out`.
//                           64 x 128 tile per 256-thread workgroup, 8 x 4 outputs per thread, K chunks of 32 transposed
//                           into LDS as [k][row] (the next chunk's global loads in flight while this one is multiplied).
//   tucker3_gather_kernel   B[idx] -> [n, d_r] dense rows in the workspace, in front of the g_W product.
//   kge_tucker3_project_bwd g_Brows = g_out * W and g_W = g_out^T * B[idx]: the two float32 gradient products of
//                           bwd_gemm32.hip (run_gemm32), not copied here.  Plain stores, no float atomics.
#include "tucker3_device.hpp"

namespace kge {

// bwd_gemm32.hip: C[M, N] = A * B on the f32 matrix cores
bool run_gemm32(bool a_kcont, int in16, long long M, long long N, long long K, const void* A, long long lda,
                const void* B, long long ldb, float* C, long long ldc, float* scratch, size_t scratch_bytes,
                hipStream_t st, int* parts = nullptr);

static bool t3_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grid.x = row tile, grid.y = column tile.  `Bm` already points at the first row of a range index (idx.ptr == NULL).
__global__ __launch_bounds__(T3_THREADS) void tucker3_project_kernel(const float* __restrict__ Bm, long long ldb, Index idx,
                                                                     const float* __restrict__ W, long long ldw, int K,
                                                                     long long N, long long n, float* __restrict__ out,
                                                                     long long ldo, int vec_b, int vec_w, int vec_o) {
  __shared__ __attribute__((aligned(16))) float sA[T3_KC * T3_LDA];
  __shared__ __attribute__((aligned(16))) float sW[T3_KC * T3_LDW];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * T3_BM, col0 = (long long)blockIdx.y * T3_BN;

  // loads: B chunk 64 rows x 32 k -- thread t takes tile row t >> 2 and k = 4 (t & 3) + 16 j .. + 3, j < 2;
  //        W chunk 128 rows x 32 k -- tile column t >> 1 and k = 4 (t & 1) + 8 j .. + 3, j < 4
  const int ar = tid >> 2, ak = (tid & 3) * 4;
  const int wr = tid >> 1, wk = (tid & 1) * 4;
  const float* arow = nullptr;
  if (row0 + ar < n) arow = Bm + index_at(idx, row0 + ar) * ldb;
  const float* wrow = col0 + wr < N ? W + (col0 + wr) * ldw : nullptr;
  f32x4 ra[2], rw[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + ak + 16 * j;
      ra[j] = (arow != nullptr && k < K) ? t3_load4(arow + k, K - k, vec_b != 0) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + wk + 8 * j;
      rw[j] = (wrow != nullptr && k < K) ? t3_load4(wrow + k, K - k, vec_w != 0) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) sA[(ak + 16 * j + e) * T3_LDA + ar] = ra[j][e];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) sW[(wk + 8 * j + e) * T3_LDW + wr] = rw[j][e];
  };

  const int tx = tid & 31, ty = tid >> 5;  // columns 4 tx .. + 3, rows 8 ty .. + 7 of the tile
  float acc[T3_TR][T3_TC];
#pragma unroll
  for (int r = 0; r < T3_TR; ++r)
#pragma unroll
    for (int c = 0; c < T3_TC; ++c) acc[r][c] = 0.0f;
  auto kstep = [&](int k) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(sA + k * T3_LDA + T3_TR * ty);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(sA + k * T3_LDA + T3_TR * ty + 4);
    const f32x4 w = *reinterpret_cast<const f32x4*>(sW + k * T3_LDW + T3_TC * tx);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < T3_TC; ++c) {
        acc[r][c] = t3_step(acc[r][c], a0[r], w[c]);
        acc[4 + r][c] = t3_step(acc[4 + r][c], a1[r], w[c]);
      }
  };

  gload(0);
  for (int k0 = 0; k0 < K; k0 += T3_KC) {
    sstore();
    __syncthreads();
    if (k0 + T3_KC < K) gload(k0 + T3_KC);
    if (k0 + T3_KC <= K) {
#pragma unroll
      for (int k = 0; k < T3_KC; ++k) kstep(k);
    } else {  // the ragged last chunk: the chain ends at K (tucker3_device.hpp)
      const int kn = K - k0;
      for (int k = 0; k < kn; ++k) kstep(k);
    }
    __syncthreads();
  }

  const long long ocol = col0 + T3_TC * tx;
  if (ocol >= N) return;
#pragma unroll
  for (int r = 0; r < T3_TR; ++r) {
    const long long orow = row0 + T3_TR * ty + r;
    if (orow >= n) break;
    float* dst = out + orow * ldo + ocol;
    if (vec_o != 0 && ocol + T3_TC <= N) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
    } else {
#pragma unroll
      for (int c = 0; c < T3_TC; ++c)
        if (ocol + c < N) dst[c] = acc[r][c];
    }
  }
}

// `Bm`: the base table, moved to the first row of a range index by the caller.
int run_tucker3_project(const float* Bm, long long ldb, const Index& idx, const float* W, long long ldw, int d, int dr,
                        long long n, float* out, long long ldo, hipStream_t st) {
  if (n == 0) return KGE_OK;
  const long long N = (long long)d * d;
  const long long tm = (n + T3_BM - 1) / T3_BM, tn = (N + T3_BN - 1) / T3_BN;
  if (tm > 0x7fffffffLL || tn > 65535) return KGE_ERR_UNSUPPORTED;
  const int vec_b = t3_aligned16(Bm) && ldb % 4 == 0, vec_w = t3_aligned16(W) && ldw % 4 == 0;
  const int vec_o = t3_aligned16(out) && ldo % 4 == 0;
  hipLaunchKernelGGL(tucker3_project_kernel, dim3((unsigned)tm, (unsigned)tn), dim3(T3_THREADS), 0, st, Bm, ldb, idx, W,
                     ldw, dr, N, n, out, ldo, vec_b, vec_w, vec_o);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// ---- backward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tucker3_gather_kernel(const float* __restrict__ Bm, long long ldb, Index idx, int dr,
                                                             long long n, float* __restrict__ dst, long long ldd) {
  const long long total = n * dr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long i = e / dr;
    const int k = (int)(e - i * dr);
    dst[i * ldd + k] = Bm[index_at(idx, i) * ldb + k];
  }
}

// The split-K partials run_gemm32 would like for an [M, N] output over K terms (its own rule: one workgroup per compute
// unit): the scratch handed to it is a function of the SHAPE, never of the caller's workspace size, so the split -- and
// with it every bit of the result -- is too.  The split needs a DENSE, 16-byte aligned output (ld == d_r: the reduction
// writes 16-byte units): with a pitched or misaligned g_brows / g_w that product runs unsplit -- inside the same bound,
// other bits.  So the bits are a function of the shape and of (dense and aligned) per output, nothing else.
static long long t3_split_bytes(long long M, long long N, long long K) {
  if (M <= 0 || N <= 0 || (M * N) % 4) return 0;
  const long long BM = M > 128 ? 256 : 128;
  const long long tiles = ((M + BM - 1) / BM) * ((N + 127) / 128);
  if (K <= 128 || tiles >= 128) return 0;
  long long P = 256 / tiles;
  if (P > K / 64) P = K / 64;
  return P < 2 ? 0 : P * M * N * 4;
}
static long long t3_gather_ld(int dr) { return (dr + 3) & ~3LL; }
static long long t3_gather_bytes(int dr, long long n) { return n * t3_gather_ld(dr) * 4; }

long long tucker3_bwd_workspace_bytes(int d, int dr, long long n) {
  const long long N = (long long)d * d;
  const long long s1 = t3_split_bytes(n, dr, N), s2 = t3_split_bytes(N, dr, n);
  return t3_gather_bytes(dr, n) + (s1 > s2 ? s1 : s2);
}

int run_tucker3_project_bwd(const float* Bm, long long ldb, const Index& idx, const float* W, long long ldw, int d, int dr,
                            long long n, const float* gout, long long ldg, float* g_brows, long long g_brows_ld,
                            float* g_w, long long g_w_ld, void* ws, long long ws_bytes, hipStream_t st) {
  if (n == 0) return KGE_OK;
  if (ws == nullptr || ws_bytes < tucker3_bwd_workspace_bytes(d, dr, n)) return KGE_ERR_WORKSPACE;
  const long long N = (long long)d * d;
  float* const rows = (float*)ws;
  float* const scratch = rows + n * t3_gather_ld(dr);
  if (g_brows != nullptr) {  // [n, d_r] = g_out [n, K = d^2] * W [K, d_r]
    const long long sb = (g_brows_ld == dr && t3_aligned16(g_brows)) ? t3_split_bytes(n, dr, N) : 0;
    if (!run_gemm32(true, 0, n, dr, N, gout, ldg, W, ldw, g_brows, g_brows_ld, sb ? scratch : nullptr, (size_t)sb, st))
      return KGE_ERR_UNSUPPORTED;
  }
  if (g_w != nullptr) {  // [d^2, d_r] = g_out^T (given as [K = n, M = d^2]) * B[idx] [K = n, d_r]
    long long blocks = (n * dr + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(tucker3_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, Bm, ldb, idx, dr, n, rows,
                       t3_gather_ld(dr));
    if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
    const long long sb = (g_w_ld == dr && t3_aligned16(g_w)) ? t3_split_bytes(N, dr, n) : 0;
    if (!run_gemm32(false, 0, N, dr, n, gout, ldg, rows, t3_gather_ld(dr), g_w, g_w_ld, sb ? scratch : nullptr, (size_t)sb,
                    st))
      return KGE_ERR_UNSUPPORTED;
  }
  return KGE_OK;
}

}  // namespace kge
