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

// ---- SparseAdam over the rows a batch touched (kge_sparse_adam_step_touched) --------------------
// torch.optim.SparseAdam (train.optimizer.default.type: SparseAdam with lookup_embedder.yaml:78-81 `sparse: True`) is
// defined row-wise: moments and parameters change on the rows present in the coalesced sparse gradient, the step count
// is per parameter.  Its row set is what the bitmap holds, so the step is adagrad_touched_kernel's walk (the same chunk
// of 256 rows per workgroup, the same list in LDS, the same groups of lanes and rows in flight) around torch's
// functional sparse_adam, operation for operation (-ffp-contract=off; include/kge_amd.h restates it):
//   u1 = (g - m) * omb1;  m = m + u1;  u2 = (g * g - v) * omb2;  v = v + u2
//   p = p + (-step_size) * (m / (__builtin_sqrtf(v) + eps));  copy = bf16_pack(p)
// step_size comes from the parameter's kge_adam_clock record, which sparse_adam_clock_kernel advances in front of the
// update: the record of kge_adam_step_multi with SparseAdam's step size in its first float.
__global__ __launch_bounds__(64) void sparse_adam_clock_kernel(kge_adam_clock* k, double lr, double beta1,
                                                               double beta2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double b1 = k->beta1_pow * beta1;
  const double b2 = k->beta2_pow * beta2;
  const double root = __builtin_sqrt(1.0 - b2);
  k->t = k->t + 1;
  k->beta1_pow = b1;
  k->beta2_pow = b2;
  k->step_size = (float)((lr * root) / (1.0 - b1));
  k->bias_correction2_sqrt = (float)root;
}

// sparse_adam_clock_kernel on its own: the clock launch of kge_sparse_adam_step_touched_wpenalty (wpenalty.hip)
int run_sparse_adam_clock(kge_adam_clock* clock, double lr, double beta1, double beta2, hipStream_t st) {
  hipLaunchKernelGGL(sparse_adam_clock_kernel, dim3(1), dim3(64), 0, st, clock, lr, beta1, beta2);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <bool VEC, int GROUP>
__global__ __launch_bounds__(256) void sparse_adam_touched_kernel(
    float* __restrict__ param, long long param_ld, float* __restrict__ grad, long long grad_ld, float* __restrict__ m1,
    long long m1_ld, float* __restrict__ m2, long long m2_ld, unsigned int* __restrict__ bitmap, long long num_rows,
    long long num_words, int dim, const kge_adam_clock* __restrict__ clock, float omb1, float omb2, float eps,
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

  const float neg_step = -clock->step_size;
  auto one = [&](float p, float g, float& a, float& b) {
    const float u1 = (g - a) * omb1;
    a = a + u1;
    const float u2 = (g * g - b) * omb2;
    b = b + u2;
    return p + neg_step * (a / (__builtin_sqrtf(b) + eps));
  };
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
        f32x4 p[ROWS_IN_FLIGHT], g[ROWS_IN_FLIGHT], a[ROWS_IN_FLIGHT], b[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            p[u] = *reinterpret_cast<const f32x4*>(param + row[u] * param_ld + 4 * c);
            g[u] = *reinterpret_cast<const f32x4*>(grad + row[u] * grad_ld + 4 * c);
            a[u] = *reinterpret_cast<const f32x4*>(m1 + row[u] * m1_ld + 4 * c);
            b[u] = *reinterpret_cast<const f32x4*>(m2 + row[u] * m2_ld + 4 * c);
          }
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            f32x4 pe = p[u], ae = a[u], be = b[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float x = ae[e], y = be[e];
              pe[e] = one(pe[e], g[u][e], x, y);
              ae[e] = x;
              be[e] = y;
            }
            *reinterpret_cast<f32x4*>(param + row[u] * param_ld + 4 * c) = pe;
            *reinterpret_cast<f32x4*>(m1 + row[u] * m1_ld + 4 * c) = ae;
            *reinterpret_cast<f32x4*>(m2 + row[u] * m2_ld + 4 * c) = be;
            const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<f32x4*>(grad + row[u] * grad_ld + 4 * c) = zero;
            if (copy16 != nullptr) {
              u32x2 cp = {bf16_pack(pe[0], pe[1]), bf16_pack(pe[2], pe[3])};
              *reinterpret_cast<u32x2*>(copy16 + row[u] * c_ld + 4 * c) = cp;
            }
          }
        }
      } else {
        float p[ROWS_IN_FLIGHT], g[ROWS_IN_FLIGHT], a[ROWS_IN_FLIGHT], b[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            p[u] = param[row[u] * param_ld + c];
            g[u] = grad[row[u] * grad_ld + c];
            a[u] = m1[row[u] * m1_ld + c];
            b[u] = m2[row[u] * m2_ld + c];
          }
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
          if (on[u]) {
            float ae = a[u], be = b[u];
            const float pe = one(p[u], g[u], ae, be);
            m1[row[u] * m1_ld + c] = ae;
            m2[row[u] * m2_ld + c] = be;
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

template <bool VEC, int GROUP>
static void launch_sparse_adam_touched(unsigned blocks, hipStream_t st, float* param, long long param_ld, float* grad,
                                       long long grad_ld, float* m1, long long m1_ld, float* m2, long long m2_ld,
                                       unsigned int* bitmap, long long num_rows, long long num_words, int dim,
                                       const kge_adam_clock* clock, float omb1, float omb2, float eps,
                                       unsigned short* copy16, long long c_ld) {
  hipLaunchKernelGGL((sparse_adam_touched_kernel<VEC, GROUP>), dim3(blocks), dim3(256), 0, st, param, param_ld, grad,
                     grad_ld, m1, m1_ld, m2, m2_ld, bitmap, num_rows, num_words, dim, clock, omb1, omb2, eps, copy16,
                     c_ld);
}

// Arguments are checked by the caller (api.hip: kge_sparse_adam_step_touched).  The clock advances once per call,
// whatever the bitmap holds and also for num_rows == 0 (torch counts a step for every step() that sees a gradient);
// the grid is checked before it, so a declined call leaves the record alone.  dim == 0: the words are still cleared.
int run_sparse_adam_touched(float* param, long long param_ld, float* grad, long long grad_ld, float* m1, long long m1_ld,
                            float* m2, long long m2_ld, unsigned int* bitmap, long long num_rows, int dim,
                            kge_adam_clock* clock, double lr, double beta1, double beta2, float eps,
                            unsigned short* copy16, long long c_ld, hipStream_t st) {
  const long long num_words = (num_rows + 31) / 32;
  const long long blocks = (num_words + TOUCHED_WORDS - 1) / TOUCHED_WORDS;
  if (blocks > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sparse_adam_clock_kernel, dim3(1), dim3(64), 0, st, clock, lr, beta1, beta2);
  if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
  if (num_rows == 0) return KGE_OK;
  // 1 - beta in double, then rounded: the weights torch derives from the Python floats
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  // four floats per lane where every row of every array starts on 16 bytes (the bf16 copy: 8), one float otherwise
  const bool vec = dim % 4 == 0 &&
                   (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m1 | (uintptr_t)m2) & 15) == 0 &&
                   param_ld % 4 == 0 && grad_ld % 4 == 0 && m1_ld % 4 == 0 && m2_ld % 4 == 0 &&
                   (copy16 == nullptr || (((uintptr_t)copy16 & 7) == 0 && c_ld % 4 == 0));
  const int units = vec ? dim / 4 : dim;
  const int group = units <= 16 ? 16 : (units <= 32 ? 32 : 64);
#define KGE_SPARSE_ADAM_LAUNCH(V, G)                                                                                 \
  launch_sparse_adam_touched<V, G>((unsigned)blocks, st, param, param_ld, grad, grad_ld, m1, m1_ld, m2, m2_ld, bitmap, \
                                   num_rows, num_words, dim, clock, omb1, omb2, eps, copy16, c_ld)
  if (vec) {
    if (group == 16) KGE_SPARSE_ADAM_LAUNCH(true, 16);
    else if (group == 32) KGE_SPARSE_ADAM_LAUNCH(true, 32);
    else KGE_SPARSE_ADAM_LAUNCH(true, 64);
  } else {
    if (group == 16) KGE_SPARSE_ADAM_LAUNCH(false, 16);
    else if (group == 32) KGE_SPARSE_ADAM_LAUNCH(false, 32);
    else KGE_SPARSE_ADAM_LAUNCH(false, 64);
  }
#undef KGE_SPARSE_ADAM_LAUNCH
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
