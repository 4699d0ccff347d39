// touched.hip -- the Adagrad step over ONLY the entity rows a negative-sampling batch touched (SURVEY.md 8f, N3:
// "dense-grad avoidance").
//
// TrainingJob.run_epoch's step (kge/job/train.py:452-474: zero_grad, backward, optimizer.step) on the fused
// negative-sampling path costs three passes over the whole [E, d] entity table however few rows the batch touched: the
// backward nodes' zeros_like(ent) fill, the float atomics into it, and kge_adagrad_step_multi's sweep (parameter,
// gradient, accumulator in; parameter, accumulator, bf16 copy out).  A batch touches at most n (2 + K_s + K_o) rows.
//
// Dense Adagrad with weight_decay == 0 leaves a row whose gradient is zero bit for bit as it was (sum + 0 * 0 = sum,
// p + (minus_clr * 0) / (sqrt(sum) + eps) = p, signed zeros included), so a step over the rows that HAVE a gradient is
// the same optimizer.  Which rows those are is kept in a bitmap: bit r % 32 of word r / 32 = row r has a gradient.
//   touched_mark_kernel   sets the bits of an [n, k] block of ids (global atomic OR from vector lanes, duplicates fine)
//   adagrad_touched_kernel<VEC, GROUP>  for every set bit the arithmetic of adagrad_multi_kernel on that row, then
//                         zeros over the row's gradient and over the bitmap word
// The gradient buffer is PERSISTENT: zero outside the marked rows on entry, all zero on exit, so no fill of the table's
// size is ever issued again.  (lookup_embedder.yaml:78-81 `sparse: True` reaches the same end through a coalesced
// torch sparse gradient and kge_adagrad_step_rows; the fused backward kernels never produce one.)
#include "common.hpp"

namespace kge {

template <typename T>
__global__ __launch_bounds__(256) void touched_mark_kernel(const T* __restrict__ ids, long long stride, long long n,
                                                           long long k, long long ld, long long num_rows,
                                                           unsigned int* __restrict__ bitmap) {
  const long long total = n * k;
  const long long step = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
    const long long i = e / k, j = e - i * k;
    const long long id = (long long)ids[(i * ld + j) * stride];
    if (id >= 0 && id < num_rows) atomicOr(bitmap + (id >> 5), 1u << (id & 31));
  }
}

int run_touched_mark(const Index& ids, long long n, long long k, long long ld, long long num_rows, unsigned int* bitmap,
                     hipStream_t st) {
  const long long total = n * k;
  if (total == 0) return KGE_OK;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;  // (grid-stride beyond: 16 waves per CU are enough to keep the atomics in flight)
  if (ids.itype)
    hipLaunchKernelGGL(touched_mark_kernel<long long>, dim3((unsigned)blocks), dim3(256), 0, st,
                       (const long long*)ids.ptr, ids.stride, n, k, ld, num_rows, bitmap);
  else
    hipLaunchKernelGGL(touched_mark_kernel<int>, dim3((unsigned)blocks), dim3(256), 0, st, (const int*)ids.ptr,
                       ids.stride, n, k, ld, num_rows, bitmap);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// A workgroup of 256 threads owns TOUCHED_WORDS bitmap words = 256 rows: thread t < 8 reads (and, at the end, clears)
// word blockIdx.x * 8 + t, so every word has exactly one owner and the clearing store needs no atomic.  An untouched
// chunk costs its 32 bytes of bitmap and nothing else.  (A chunk of 2048 rows per workgroup was the first shape: at
// E = 14,541 that is 8 workgroups for the whole table, each wave walking hundreds of rows one dependent load-store
// round trip after the other; 256 rows per workgroup are 57 workgroups there and 17,947 at E = 4.6 M, where a
// workgroup finds ~14 marked rows.)
//
// The marked rows of the chunk are listed in LDS (thread t looks at bit t: its slot is the number of set bits below it)
// and dealt to groups of GROUP lanes -- 16, 32 or 64, the smallest that covers a row in one trip (VEC: four floats per
// lane; scalar otherwise) -- ROWS_IN_FLIGHT rows per group and trip: the loads of all of them are issued before the
// first is used.  One row per WAVE (adagrad_rows_kernel's shape) leaves half a wave idle at d = 128 and, a table most
// of whose rows are marked, a latency chain of one row at a time.
//
// Arithmetic: adagrad_multi_kernel's with weight_decay == 0, operation for operation (-ffp-contract=off):
//   s = s + g * g;   p = p + (minus_clr * g) / (__builtin_sqrtf(s) + eps);   copy = bf16_pack(p)
constexpr int TOUCHED_WORDS = 8;
constexpr int TOUCHED_ROWS = TOUCHED_WORDS * 32;  // = the workgroup's 256 threads
constexpr int ROWS_IN_FLIGHT = 4;

template <bool VEC, int GROUP>
__global__ __launch_bounds__(256) void adagrad_touched_kernel(float* __restrict__ param, long long param_ld,
                                                              float* __restrict__ grad, long long grad_ld,
                                                              float* __restrict__ sum, long long sum_ld,
                                                              unsigned int* __restrict__ bitmap, long long num_rows,
                                                              long long num_words, int dim, float minus_clr, float eps,
                                                              unsigned short* __restrict__ copy16, long long c_ld) {
  __shared__ unsigned int words[TOUCHED_WORDS];
  __shared__ unsigned short list[TOUCHED_ROWS];
  const int tid = threadIdx.x;
  const long long word0 = (long long)blockIdx.x * TOUCHED_WORDS;
  unsigned int raw = 0u;
  if (tid < TOUCHED_WORDS) {
    const long long wi = word0 + tid;
    if (wi < num_words) raw = bitmap[wi];
    const long long valid = num_rows - wi * 32;  // rows of this word that exist
    const unsigned int mask = valid >= 32 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << valid) - 1u));
    words[tid] = raw & mask;
  }
  __syncthreads();
  int total = 0, before = 0;
#pragma unroll
  for (int j = 0; j < TOUCHED_WORDS; ++j) {
    const int c = __builtin_popcount(words[j]);
    total += c;
    if (j < (tid >> 5)) before += c;
  }
  if (total == 0) {  // (uniform) nothing marked here; a word with bits past num_rows only is still cleared
    if (tid < TOUCHED_WORDS && raw != 0u) bitmap[word0 + tid] = 0u;
    return;
  }
  const unsigned int mine = words[tid >> 5];
  if ((mine >> (tid & 31)) & 1u)
    list[before + __builtin_popcount(mine & ((1u << (tid & 31)) - 1u))] = (unsigned short)tid;
  __syncthreads();

  constexpr int GROUPS = 256 / GROUP;
  const int gid = tid / GROUP, gl = tid % GROUP;
  const long long row0 = word0 * 32;
  const int units = VEC ? dim / 4 : dim;  // what a lane handles per trip: four floats or one
  for (int base = gid; base < total; base += GROUPS * ROWS_IN_FLIGHT) {
    long long row[ROWS_IN_FLIGHT];
    bool on[ROWS_IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
      const int at = base + u * GROUPS;
      on[u] = at < total;
      row[u] = row0 + list[on[u] ? at : base];
    }
    for (int c = gl; c < units; c += GROUP) {
      if (VEC) {
        f32x4 p[ROWS_IN_FLIGHT], g[ROWS_IN_FLIGHT], s[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            p[u] = *reinterpret_cast<const f32x4*>(param + row[u] * param_ld + 4 * c);
            g[u] = *reinterpret_cast<const f32x4*>(grad + row[u] * grad_ld + 4 * c);
            s[u] = *reinterpret_cast<const f32x4*>(sum + row[u] * sum_ld + 4 * c);
          }
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            f32x4 pe = p[u], se = s[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float ge = g[u][e];
              se[e] = se[e] + ge * ge;
              pe[e] = pe[e] + (minus_clr * ge) / (__builtin_sqrtf(se[e]) + eps);
            }
            *reinterpret_cast<f32x4*>(param + row[u] * param_ld + 4 * c) = pe;
            *reinterpret_cast<f32x4*>(sum + row[u] * sum_ld + 4 * c) = se;
            const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(grad + row[u] * grad_ld + 4 * c) = zero;
            if (copy16 != nullptr) {
              u32x2 cp = {bf16_pack(pe[0], pe[1]), bf16_pack(pe[2], pe[3])};
              *reinterpret_cast<u32x2*>(copy16 + row[u] * c_ld + 4 * c) = cp;
            }
          }
        }
      } else {
        float p[ROWS_IN_FLIGHT], g[ROWS_IN_FLIGHT], s[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            p[u] = param[row[u] * param_ld + c];
            g[u] = grad[row[u] * grad_ld + c];
            s[u] = sum[row[u] * sum_ld + c];
          }
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            const float ge = g[u];
            const float se = s[u] + ge * ge;
            const float pe = p[u] + (minus_clr * ge) / (__builtin_sqrtf(se) + eps);
            sum[row[u] * sum_ld + c] = se;
            param[row[u] * param_ld + c] = pe;
            grad[row[u] * grad_ld + c] = 0.0f;
            if (copy16 != nullptr) copy16[row[u] * c_ld + c] = (unsigned short)(bf16_pack(pe, 0.0f) & 0xffffu);
          }
        }
      }
    }
  }
  __syncthreads();  // every row of the chunk is done: its words' one owner clears them
  if (tid < TOUCHED_WORDS && raw != 0u) bitmap[word0 + tid] = 0u;
}

template <bool VEC>
static void launch_adagrad_touched(int group, unsigned blocks, hipStream_t st, float* param, long long param_ld,
                                   float* grad, long long grad_ld, float* sum, long long sum_ld, unsigned int* bitmap,
                                   long long num_rows, long long num_words, int dim, float minus_clr, float eps,
                                   unsigned short* copy16, long long c_ld) {
  if (group == 16)
    hipLaunchKernelGGL((adagrad_touched_kernel<VEC, 16>), dim3(blocks), dim3(256), 0, st, param, param_ld, grad, grad_ld,
                       sum, sum_ld, bitmap, num_rows, num_words, dim, minus_clr, eps, copy16, c_ld);
  else if (group == 32)
    hipLaunchKernelGGL((adagrad_touched_kernel<VEC, 32>), dim3(blocks), dim3(256), 0, st, param, param_ld, grad, grad_ld,
                       sum, sum_ld, bitmap, num_rows, num_words, dim, minus_clr, eps, copy16, c_ld);
  else
    hipLaunchKernelGGL((adagrad_touched_kernel<VEC, 64>), dim3(blocks), dim3(256), 0, st, param, param_ld, grad, grad_ld,
                       sum, sum_ld, bitmap, num_rows, num_words, dim, minus_clr, eps, copy16, c_ld);
}

// Arguments are checked by the caller (api.hip: kge_adagrad_step_touched).  dim == 0: the words are still cleared.
int run_adagrad_touched(float* param, long long param_ld, float* grad, long long grad_ld, float* sum, long long sum_ld,
                        unsigned int* bitmap, long long num_rows, int dim, float minus_clr, float eps,
                        unsigned short* copy16, long long c_ld, hipStream_t st) {
  if (num_rows == 0) return KGE_OK;
  const long long num_words = (num_rows + 31) / 32;
  const long long blocks = (num_words + TOUCHED_WORDS - 1) / TOUCHED_WORDS;
  if (blocks > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  // four floats per lane where every row of every array starts on 16 bytes (the bf16 copy: 8), one float otherwise
  const bool vec = dim % 4 == 0 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)sum) & 15) == 0 &&
                   param_ld % 4 == 0 && grad_ld % 4 == 0 && sum_ld % 4 == 0 &&
                   (copy16 == nullptr || (((uintptr_t)copy16 & 7) == 0 && c_ld % 4 == 0));
  const int units = vec ? dim / 4 : dim;
  const int group = units <= 16 ? 16 : (units <= 32 ? 32 : 64);
  if (vec)
    launch_adagrad_touched<true>(group, (unsigned)blocks, st, param, param_ld, grad, grad_ld, sum, sum_ld, bitmap,
                                 num_rows, num_words, dim, minus_clr, eps, copy16, c_ld);
  else
    launch_adagrad_touched<false>(group, (unsigned)blocks, st, param, param_ld, grad, grad_ld, sum, sum_ld, bitmap,
                                  num_rows, num_words, dim, minus_clr, eps, copy16, c_ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
