// wpenalty.hip -- the embedders' FREQUENCY-WEIGHTED penalty terms inside the optimizer's pass.
//
// LookupEmbedder.penalty with regularize_args.weighted: true (kge/model/embedder/lookup_embedder.py:148-173) is, with
// m = len(indexes) and c_r = the occurrences of row r among the batch's indexes,
//   value = weight / p / m * sum_r c_r * sum_j |x_rj|^p          (n3, complex: |z|^3, |z| = sqrt(re^2 + im^2 + 1e-14))
//   d value / d x_rj = (weight * c_r / m) * sign(x) |x|^(p-1)    (n3: (weight * c_r / m) * |z| * re, ... * im)
// -- the gradient is a function of the element and of ITS ROW'S COUNT.  The reference gets c_r from torch.unique (a sort
// and a host wait) and the gradient through an embedding gather and autograd's scatter into a fresh [E, d] tensor.  Here:
//   penalty_count_kernel  counts[id] += 1 per occurrence (integer atomics: exact, order-free), optionally marking the
//                         row in the touched-row bitmap; duplicates inside a wave are merged before they leave it
//   multi_wpen_kernel     adagrad_multi_pen_kernel's / adam_multi_kernel<PEN>'s arithmetic per element with w replaced by
//                         the row factor f_r = weight * ((float)c_r / (float)m)  (one IEEE division, then one product)
//   touched_wpen_kernel   adagrad_touched_kernel's / sparse_adam_touched_kernel's row updates with g + f_r * ... in registers
// Every count word has ONE owner workgroup, which reads it once and stores zero over it: after the step the count buffer
// is all zero again (the discipline of the touched-row bitmap), no fill of the table's height is ever issued.
// A row whose count is 0 gets NO penalty gradient (nothing is added, not even a signed zero) and adds nothing to the value.
// *value receives sum_r c_r * sum_j |x_rj|^p of the pre-step parameters: |x|^p per element in float32, the product with
// the count and every sum in double; one double atomic per workgroup.
#include "common.hpp"

namespace kge {

// ---- the count -------------------------------------------------------------------------------------------------------
// MERGE: the lanes of a wave that hold the same id send ONE atomic with their number.  A leader (the first live lane)
// broadcasts its id, the lanes that hold it are ballotted off; after COUNT_MERGE_ROUNDS leaders the lanes still live add
// their own 1.  One id repeated over the whole input (a batch of one relation) is then one atomic per wave instead of
// 64 on one word; all-distinct ids pay the rounds for nothing -- which is why the rounds are few.
constexpr int COUNT_MERGE_ROUNDS = 4;

template <typename T, bool MERGE>
__global__ __launch_bounds__(256) void penalty_count_kernel(const T* __restrict__ ids, long long stride, long long n,
                                                            long long k, long long ld, long long num_rows,
                                                            unsigned int* __restrict__ counts,
                                                            unsigned int* __restrict__ bitmap) {
  const long long total = n * k;
  const long long step = (long long)gridDim.x * 256;
  const int lane = threadIdx.x & 63;
  // the trip count is uniform over a WAVE (its first element decides): the ballots below see all 64 lanes
  for (long long e0 = (long long)blockIdx.x * 256 + (threadIdx.x - lane); e0 < total; e0 += step) {
    const long long e = e0 + lane;
    long long id = -1;
    if (e < total) {
      const long long i = e / k, j = e - i * k;
      id = (long long)ids[(i * ld + j) * stride];
      if (id < 0 || id >= num_rows) id = -1;
    }
    if (!MERGE) {
      if (id >= 0) {
        atomicAdd(counts + id, 1u);
        if (bitmap != nullptr) atomicOr(bitmap + (id >> 5), 1u << (id & 31));
      }
      continue;
    }
    unsigned long long live = __ballot(id >= 0);
    for (int round = 0; live != 0ull; ++round) {  // (uniform)
      if (round == COUNT_MERGE_ROUNDS) {
        if ((live >> lane) & 1ull) {
          atomicAdd(counts + id, 1u);
          if (bitmap != nullptr) atomicOr(bitmap + (id >> 5), 1u << (id & 31));
        }
        break;
      }
      const int lead = __builtin_ctzll(live);
      const long long lid = __shfl(id, lead, 64);
      const unsigned long long same = __ballot(id == lid) & live;
      if (lane == lead) {
        atomicAdd(counts + lid, (unsigned int)__builtin_popcountll(same));
        if (bitmap != nullptr) atomicOr(bitmap + (lid >> 5), 1u << (lid & 31));
      }
      live &= ~same;
    }
  }
}

// Arguments are checked by the caller (api.hip: kge_penalty_count).  merge: the in-wave duplicate merge (the product
// path) or one atomic per lane (switch PENALTY_COUNT_PLAIN: tools/wpenalty_probe.py times both).
int run_penalty_count(const Index& ids, long long n, long long k, long long ld, long long num_rows, unsigned int* counts,
                      unsigned int* bitmap, bool merge, hipStream_t st) {
  const long long total = n * k;
  if (total == 0) return KGE_OK;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;  // (grid-stride beyond, as touched_mark_kernel)
#define KGE_COUNT_LAUNCH(T, M)                                                                                       \
  hipLaunchKernelGGL((penalty_count_kernel<T, M>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)ids.ptr, \
                     ids.stride, n, k, ld, num_rows, counts, bitmap)
  if (ids.itype) {
    if (merge) KGE_COUNT_LAUNCH(long long, true);
    else KGE_COUNT_LAUNCH(long long, false);
  } else {
    if (merge) KGE_COUNT_LAUNCH(int, true);
    else KGE_COUNT_LAUNCH(int, false);
  }
#undef KGE_COUNT_LAUNCH
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// ---- what the four updates share -------------------------------------------------------------------------------------
// One element of an optimizer, operation for operation (-ffp-contract=off) the arithmetic of
//   OPT 0  adagrad_multi_kernel (optim.hip)            a = state_sum              c0 = minus_clr
//   OPT 1  adam_kernel / adam_multi_kernel (optim.hip) a, b = the moments         c0 = 1 - beta1, c1 = beta2, c2 = 1 - beta2
//   OPT 2  sparse_adam_touched_kernel (touched.hip)    a, b = the moments         c0 = 1 - beta1, c1 = 1 - beta2
// (adagrad_touched_kernel is OPT 0 with weight_decay == 0.)
struct StepArith {
  float c0, c1, c2, weight_decay, eps;
  float step_size, bc2_sqrt;  // the clock record's two floats (OPT 1, 2)
};

template <int OPT>
__device__ __forceinline__ float step_one(const StepArith& s, float p, float g, float& a, float& b) {
  if (OPT == 0) {
    if (s.weight_decay != 0.0f) g = g + s.weight_decay * p;
    a = a + g * g;
    return p + (s.c0 * g) / (__builtin_sqrtf(a) + s.eps);
  } else if (OPT == 1) {
    if (s.weight_decay != 0.0f) g = g + s.weight_decay * p;
    a = a + (g - a) * s.c0;
    b = b * s.c1 + (s.c2 * g) * g;
    const float denom = __builtin_sqrtf(b) / s.bc2_sqrt + s.eps;
    return p + (-s.step_size) * (a / denom);
  } else {
    const float u1 = (g - a) * s.c0;
    a = a + u1;
    const float u2 = (g * g - b) * s.c1;
    b = b + u2;
    return p + (-s.step_size) * (a / (__builtin_sqrtf(b) + s.eps));
  }
}

// The lp term's gradient of one element under the row factor f -- pen_grad_lp's expressions (optim.hip) -- and the
// element's part of the value: c * |x|^p, |x|^p in float32, the product (exact: 24 x 24 bits) and the sum in double.
__device__ __forceinline__ float wpen_lp(float x, int p, float f, unsigned int c, double& vd) {
  const float a = __builtin_fabsf(x);
  float t, g;
  if (p == 2) {
    t = x * x;
    g = f * x;
  } else if (p == 1) {
    t = a;
    g = x > 0.0f ? f : (x < 0.0f ? -f : 0.0f);
  } else {  // p == 3
    t = a * a * a;
    g = f * (x * a);
  }
  vd += (double)c * (double)t;
  return g;
}

// the n3 term of one complex coordinate (adagrad_multi_pen_kernel's expressions)
__device__ __forceinline__ void wpen_n3(float re, float im, float f, unsigned int c, float& g_re, float& g_im,
                                        double& vd) {
  const float z = __builtin_sqrtf(re * re + im * im + 1e-14f);
  vd += (double)c * (double)(z * z * z);
  g_re = f * (z * re);
  g_im = f * (z * im);
}

template <int W>
__device__ __forceinline__ void load_w(float (&v)[W], const float* p) {
  if constexpr (W == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = t[e];
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void store_w(float* p, const float (&v)[W]) {
  if constexpr (W == 4) {
    const f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}

template <int W>
__device__ __forceinline__ void store_bf16_w(unsigned short* p, const float (&v)[W]) {
  if constexpr (W == 4) {
    const u32x2 c = {bf16_pack(v[0], v[1]), bf16_pack(v[2], v[3])};
    *reinterpret_cast<u32x2*>(p) = c;
  } else {
    *p = (unsigned short)(bf16_pack(v[0], 0.0f) & 0xffffu);
  }
}

// W elements from offset `at` of the four arrays: x = the parameters (already loaded: the term was formed from them),
// pg = the term's gradient, add[e] = whether element e takes it (its row's count is not 0).  zero_grad: the touched-row
// contract (zeros over the gradient that was read).
template <int OPT, int W, bool ZERO_GRAD>
__device__ __forceinline__ void step_w(const StepArith& s, float* param, float* grad, float* s1, float* s2,
                                       unsigned short* copy16, long long at, long long at_grad, long long at_s1,
                                       long long at_s2, long long at_copy, const float (&x)[W], const float (&pg)[W],
                                       const bool (&add)[W]) {
  float g[W], a[W], b[W], p[W];
  load_w<W>(g, grad + at_grad);
  load_w<W>(a, s1 + at_s1);
  if (OPT != 0) load_w<W>(b, s2 + at_s2);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    float be = OPT != 0 ? b[e] : 0.0f;
    p[e] = step_one<OPT>(s, x[e], add[e] ? g[e] + pg[e] : g[e], a[e], be);
    if (OPT != 0) b[e] = be;
  }
  store_w<W>(param + at, p);
  store_w<W>(s1 + at_s1, a);
  if (OPT != 0) store_w<W>(s2 + at_s2, b);
  if (ZERO_GRAD) {
    float zero[W];
#pragma unroll
    for (int e = 0; e < W; ++e) zero[e] = 0.0f;
    store_w<W>(grad + at_grad, zero);
  }
  if (copy16 != nullptr) store_bf16_w<W>(copy16 + at_copy, p);
}

// one workgroup's double partial into *value (every thread of the workgroup calls)
__device__ __forceinline__ void wpen_value_add(double vd, double* value, double (&part)[4]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vd += __shfl_down(vd, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = vd;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = part[0] + part[1] + part[2] + part[3];
    if (sum != 0.0) atomicAdd(value, sum);  // (all terms are >= 0: a zero sum has nothing to add)
  }
}

// ---- the dense route (kge_adagrad_step_multi_wpenalty, kge_adam_step_multi_wpenalty) ---------------------------------
// adagrad_multi_pen_kernel walks a table as a flat array, 1024 elements per workgroup.  The count of a row would then be
// read by several workgroups and nobody could clear it.  Here a workgroup owns WHOLE ROWS: rows_per_block of them
// (a multiple of 4, so every workgroup's first element keeps the arrays' 16-byte alignment; about 1024 elements), whose
// counts and factors it keeps in LDS.  The elements are still taken four at a time regardless of the row width: with
// row_dim % 4 != 0 the four elements of a quad carry the factors of different rows.  A segment of kind 0 is the plain
// update in chunks of 1024 elements.
constexpr int WPEN_MAX_SEGS = 8;
constexpr int WPEN_MAX_ROWS = 1024;  // rows a workgroup owns at row_dim == 1
static_assert(KGE_ADAGRAD_MAX_SEGS <= WPEN_MAX_SEGS && KGE_ADAM_MAX_SEGS <= WPEN_MAX_SEGS, "segment arrays");

struct WPenSegs {
  float* param[WPEN_MAX_SEGS];
  float* grad[WPEN_MAX_SEGS];
  float* s1[WPEN_MAX_SEGS];
  float* s2[WPEN_MAX_SEGS];
  unsigned short* copy16[WPEN_MAX_SEGS];
  const kge_adam_clock* clock[WPEN_MAX_SEGS];
  unsigned int* counts[WPEN_MAX_SEGS];
  double* value[WPEN_MAX_SEGS];
  long long count[WPEN_MAX_SEGS];
  unsigned int first_block[WPEN_MAX_SEGS + 1];
  float c0[WPEN_MAX_SEGS], c1[WPEN_MAX_SEGS], c2[WPEN_MAX_SEGS], weight_decay[WPEN_MAX_SEGS], eps[WPEN_MAX_SEGS];
  float weight[WPEN_MAX_SEGS], fm[WPEN_MAX_SEGS];
  int kind[WPEN_MAX_SEGS], p[WPEN_MAX_SEGS], row_dim[WPEN_MAX_SEGS], rows_per_block[WPEN_MAX_SEGS];
  int num;
};

template <int OPT>
__global__ __launch_bounds__(256) void multi_wpen_kernel(WPenSegs a) {
  __shared__ double part[4];
  __shared__ unsigned int cnt[WPEN_MAX_ROWS];
  __shared__ float fac[WPEN_MAX_ROWS];
  int k = 0;
#pragma unroll
  for (int j = 1; j < WPEN_MAX_SEGS; ++j)
    if (j < a.num && blockIdx.x >= a.first_block[j]) k = j;
  float* __restrict__ param = a.param[k];
  float* __restrict__ grad = a.grad[k];
  float* __restrict__ s1 = a.s1[k];
  float* __restrict__ s2 = a.s2[k];
  unsigned short* __restrict__ copy16 = a.copy16[k];
  const long long count = a.count[k];
  StepArith s;
  s.c0 = a.c0[k], s.c1 = a.c1[k], s.c2 = a.c2[k], s.weight_decay = a.weight_decay[k], s.eps = a.eps[k];
  s.step_size = 0.0f, s.bc2_sqrt = 1.0f;
  if (OPT == 1) s.step_size = a.clock[k]->step_size, s.bc2_sqrt = a.clock[k]->bias_correction2_sqrt;
  const int kind = a.kind[k], pp = a.p[k], rd = a.row_dim[k];
  const int tid = threadIdx.x;
  const long long b = (long long)(blockIdx.x - a.first_block[k]);
  double vd = 0.0;

  if (kind == 0) {  // (uniform) the plain update of 1024 elements
    const long long c0 = b * 1024, c1 = c0 + 1024 < count ? c0 + 1024 : count;
    const long long i = c0 + 4 * tid;
    const float nopg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool noadd[4] = {false, false, false, false};
    if (i + 4 <= c1) {
      float x[4];
      load_w<4>(x, param + i);
      step_w<OPT, 4, false>(s, param, grad, s1, s2, copy16, i, i, i, i, i, x, nopg, noadd);
    } else {
      for (long long j = i; j < c1; ++j) {
        const float x[1] = {param[j]}, pg1[1] = {0.0f};
        const bool add1[1] = {false};
        step_w<OPT, 1, false>(s, param, grad, s1, s2, copy16, j, j, j, j, j, x, pg1, add1);
      }
    }
    return;
  }

  const int rpb = a.rows_per_block[k];
  const long long r0 = b * rpb;
  const long long left = count / rd - r0;
  const int rows = left < rpb ? (int)left : rpb;
  unsigned int mine = 0u;
  {
    unsigned int* __restrict__ counts = a.counts[k];
    const float w = a.weight[k], fm = a.fm[k];
    for (int r = tid; r < rows; r += 256) {  // this workgroup is the one reader of these words: it clears them
      const unsigned int c = counts[r0 + r];
      if (c != 0u) counts[r0 + r] = 0u;
      cnt[r] = c;
      fac[r] = w * ((float)c / fm);
      mine |= c;
    }
  }
  // (the barrier the LDS words need, and the workgroup's answer to "does any of my rows take the term": at a table of
  // millions of rows a batch counts a few hundred, and every other workgroup runs the plain update -- no float64
  // arithmetic, no reduction, no atomic on the one value word)
  const bool any = __syncthreads_or(mine != 0u) != 0;
  const long long e0 = r0 * rd;        // the chunk's first element: a multiple of 4 (rpb % 4 == 0)
  const int len = rows * rd;           // (< 2^31: checked by the launcher)
  if (kind == 2) {  // one (re, im) pair of quads per thread and trip; rd % 8 == 0
    const int h = rd / 2;
    for (int o = 4 * tid; o < rows * h; o += 1024) {
      const int r = o / h;
      const long long i_re = e0 + (long long)r * rd + (o - r * h), i_im = i_re + h;
      const unsigned int c = cnt[r];
      const float f = fac[r];
      float re[4], im[4], g_re[4] = {}, g_im[4] = {};
      load_w<4>(re, param + i_re);
      load_w<4>(im, param + i_im);
      if (c != 0u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) wpen_n3(re[e], im[e], f, c, g_re[e], g_im[e], vd);
      }
      const bool add[4] = {c != 0u, c != 0u, c != 0u, c != 0u};
      step_w<OPT, 4, false>(s, param, grad, s1, s2, copy16, i_re, i_re, i_re, i_re, i_re, re, g_re, add);
      step_w<OPT, 4, false>(s, param, grad, s1, s2, copy16, i_im, i_im, i_im, i_im, i_im, im, g_im, add);
    }
  } else {
    for (int o = 4 * tid; o < len; o += 1024) {
      const long long i = e0 + o;
      if (o + 4 <= len) {
        float x[4], pg[4];
        bool add[4];
        load_w<4>(x, param + i);
        const int r_first = o / rd;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = (rd & 3) == 0 ? r_first : (o + e) / rd;
          const unsigned int c = cnt[r];
          add[e] = c != 0u;
          pg[e] = c != 0u ? wpen_lp(x[e], pp, fac[r], c, vd) : 0.0f;
        }
        step_w<OPT, 4, false>(s, param, grad, s1, s2, copy16, i, i, i, i, i, x, pg, add);
      } else {  // the table's last elements (count % 4 != 0)
        for (int oo = o; oo < len; ++oo) {
          const long long j = e0 + oo;
          const int r = oo / rd;
          const unsigned int c = cnt[r];
          const float x[1] = {param[j]};
          const float pg1[1] = {c != 0u ? wpen_lp(x[0], pp, fac[r], c, vd) : 0.0f};
          const bool add1[1] = {c != 0u};
          step_w<OPT, 1, false>(s, param, grad, s1, s2, copy16, j, j, j, j, j, x, pg1, add1);
        }
      }
    }
  }
  if (any) wpen_value_add(vd, a.value[k], part);  // (uniform)
}

// rows a workgroup owns: a multiple of 4, about 1024 elements, at most WPEN_MAX_ROWS
static int wpen_rows_per_block(long long row_dim) {
  long long q = 256 / row_dim;
  if (q < 1) q = 1;
  return (int)(4 * q);
}

// Fills the segment record's penalty part and returns the workgroups the segment takes, or -1: unsupported.
static long long wpen_plan(WPenSegs& a, int k, long long count, const kge_wpenalty_seg& q) {
  a.kind[k] = q.kind;
  if (q.kind == 0) return (count + 1023) / 1024;
  if (q.row_dim > (1LL << 28)) return -1;  // 4 rows of a workgroup's chunk in a 32-bit offset
  a.p[k] = q.p;
  a.weight[k] = q.weight;
  a.fm[k] = (float)q.m;  // exact: m < 2^24
  a.row_dim[k] = (int)q.row_dim;
  a.rows_per_block[k] = wpen_rows_per_block(q.row_dim);
  a.counts[k] = (unsigned int*)q.counts;
  a.value[k] = q.value;
  const long long rows = count / q.row_dim;
  return (rows + a.rows_per_block[k] - 1) / a.rows_per_block[k];
}

// Arguments are checked by the caller (api.hip: kge_adagrad_step_multi_wpenalty).
int run_adagrad_multi_wpen(const kge_adagrad_seg* segs, const kge_wpenalty_seg* pens, int num, hipStream_t st) {
  WPenSegs a{};
  long long blocks = 0;
  int k = 0;
  for (int j = 0; j < num; ++j) {
    if (segs[j].count == 0) continue;
    a.param[k] = segs[j].param;
    a.grad[k] = const_cast<float*>(segs[j].grad);  // (read only: the dense route does not clear the gradient)
    a.s1[k] = segs[j].state_sum;
    a.copy16[k] = (unsigned short*)segs[j].bf16_copy;
    a.count[k] = segs[j].count;
    a.c0[k] = segs[j].minus_clr;
    a.weight_decay[k] = segs[j].weight_decay;
    a.eps[k] = segs[j].eps;
    a.first_block[k] = (unsigned int)blocks;
    const long long nb = wpen_plan(a, k, segs[j].count, pens[j]);
    if (nb < 0) return KGE_ERR_UNSUPPORTED;
    blocks += nb;
    if (blocks > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
    ++k;
  }
  if (k == 0) return KGE_OK;
  a.first_block[k] = (unsigned int)blocks;
  a.num = k;
  hipLaunchKernelGGL(multi_wpen_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// the clock kernel of kge_adam_step_multi (optim.hip), for the records of this call's non-empty segments
int run_adam_clocks(kge_adam_clock* const* clocks, const double* lr, const double* beta1, const double* beta2, int num,
                    hipStream_t st);

// Arguments are checked by the caller (api.hip: kge_adam_step_multi_wpenalty).  Empty segments take no workgroup and
// their clocks are not advanced; nothing non-empty: no launch at all -- as run_adam_multi.
int run_adam_multi_wpen(const kge_adam_seg* segs, const kge_wpenalty_seg* pens, int num, hipStream_t st) {
  WPenSegs a{};
  kge_adam_clock* clocks[WPEN_MAX_SEGS];
  double lr[WPEN_MAX_SEGS], b1[WPEN_MAX_SEGS], b2[WPEN_MAX_SEGS];
  long long blocks = 0;
  int k = 0;
  for (int j = 0; j < num; ++j) {
    if (segs[j].count == 0) continue;
    a.param[k] = segs[j].param;
    a.grad[k] = const_cast<float*>(segs[j].grad);
    a.s1[k] = segs[j].exp_avg;
    a.s2[k] = segs[j].exp_avg_sq;
    a.copy16[k] = (unsigned short*)segs[j].bf16_copy;
    a.clock[k] = segs[j].clock;
    a.count[k] = segs[j].count;
    // 1 - beta in double, then rounded: as kge_adam_step
    a.c0[k] = (float)(1.0 - segs[j].beta1);
    a.c1[k] = (float)segs[j].beta2;
    a.c2[k] = (float)(1.0 - segs[j].beta2);
    a.weight_decay[k] = segs[j].weight_decay;
    a.eps[k] = segs[j].eps;
    clocks[k] = segs[j].clock;
    lr[k] = segs[j].lr;
    b1[k] = segs[j].beta1;
    b2[k] = segs[j].beta2;
    a.first_block[k] = (unsigned int)blocks;
    const long long nb = wpen_plan(a, k, segs[j].count, pens[j]);
    if (nb < 0) return KGE_ERR_UNSUPPORTED;
    blocks += nb;
    if (blocks > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
    ++k;
  }
  if (k == 0) return KGE_OK;
  a.first_block[k] = (unsigned int)blocks;
  a.num = k;
  const int rc = run_adam_clocks(clocks, lr, b1, b2, k, st);
  if (rc != KGE_OK) return rc;
  hipLaunchKernelGGL(multi_wpen_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// ---- the touched-row route (kge_adagrad_step_touched_wpenalty, kge_sparse_adam_step_touched_wpenalty) -----------------
// adagrad_touched_kernel's walk (touched.hip): a workgroup owns 8 bitmap words = 256 rows, lists the marked ones in LDS
// and deals them to groups of GROUP lanes.  The thread that finds its row marked is also the one reader of that row's
// count word: it reads it, stores zero over it and leaves count and factor next to the row in the list.  The count
// buffer must be zero outside the marked rows on entry (kge_penalty_count with the bitmap marks what it counts), as the
// gradient buffer must: an unmarked row's count is neither read nor cleared.
constexpr int WT_WORDS = 8;
constexpr int WT_ROWS = WT_WORDS * 32;  // = the workgroup's 256 threads

struct WPenRow {
  int kind, p;
  float weight, fm;
  unsigned int* counts;
  double* value;
};

template <bool VEC, int GROUP, int OPT>
__global__ __launch_bounds__(256) void touched_wpen_kernel(float* __restrict__ param, long long param_ld,
                                                           float* __restrict__ grad, long long grad_ld,
                                                           float* __restrict__ s1, long long s1_ld,
                                                           float* __restrict__ s2, long long s2_ld,
                                                           unsigned int* __restrict__ bitmap, long long num_rows,
                                                           long long num_words, int dim, StepArith s,
                                                           const kge_adam_clock* __restrict__ clock,
                                                           unsigned short* __restrict__ copy16, long long c_ld,
                                                           WPenRow q) {
  __shared__ unsigned int words[WT_WORDS];
  __shared__ unsigned short list[WT_ROWS];
  __shared__ unsigned int cnt[WT_ROWS];
  __shared__ float fac[WT_ROWS];
  __shared__ double part[4];
  const int tid = threadIdx.x;
  const long long word0 = (long long)blockIdx.x * WT_WORDS;
  unsigned int raw = 0u;
  if (tid < WT_WORDS) {
    const long long wi = word0 + tid;
    if (wi < num_words) raw = bitmap[wi];
    const long long valid = num_rows - wi * 32;  // rows of this word that exist
    const unsigned int mask = valid >= 32 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << valid) - 1u));
    words[tid] = raw & mask;
  }
  __syncthreads();
  int total = 0, before = 0;
#pragma unroll
  for (int j = 0; j < WT_WORDS; ++j) {
    const int c = __builtin_popcount(words[j]);
    total += c;
    if (j < (tid >> 5)) before += c;
  }
  if (total == 0) {  // (uniform) nothing marked here; a word with bits past num_rows only is still cleared
    if (tid < WT_WORDS && raw != 0u) bitmap[word0 + tid] = 0u;
    return;
  }
  const long long row0 = word0 * 32;
  const unsigned int mine = words[tid >> 5];
  if ((mine >> (tid & 31)) & 1u) {
    const int slot = before + __builtin_popcount(mine & ((1u << (tid & 31)) - 1u));
    list[slot] = (unsigned short)tid;
    unsigned int c = 0u;
    if (q.kind != 0) {
      c = q.counts[row0 + tid];
      if (c != 0u) q.counts[row0 + tid] = 0u;
    }
    cnt[slot] = c;
    fac[slot] = q.kind != 0 ? q.weight * ((float)c / q.fm) : 0.0f;
  }
  __syncthreads();

  if (OPT == 2) s.step_size = clock->step_size;
  constexpr int W = VEC ? 4 : 1;
  constexpr int GROUPS = 256 / GROUP;
  const int gid = tid / GROUP, gl = tid % GROUP;
  const int units = dim / W;  // what a lane handles per trip: four floats or one
  double vd = 0.0;
  for (int at = gid; at < total; at += GROUPS) {
    const long long row = row0 + list[at];
    const unsigned int c = cnt[at];
    const float f = fac[at];
    const long long op = row * param_ld, og = row * grad_ld, o1 = row * s1_ld, o2 = row * s2_ld, oc = row * c_ld;
    bool add[W];
#pragma unroll
    for (int e = 0; e < W; ++e) add[e] = c != 0u;
    if (q.kind == 2) {  // lane u: the real parts of unit u and their imaginary parts half a row on; dim % 8 == 0
      const int hu = units / 2, h = dim / 2;
      for (int u = gl; u < hu; u += GROUP) {
        const int col = W * u;
        float re[W], im[W], g_re[W] = {}, g_im[W] = {};
        load_w<W>(re, param + op + col);
        load_w<W>(im, param + op + col + h);
        if (c != 0u) {  // (a row the backward marked and no index of the batch names: the plain update)
#pragma unroll
          for (int e = 0; e < W; ++e) wpen_n3(re[e], im[e], f, c, g_re[e], g_im[e], vd);
        }
        step_w<OPT, W, true>(s, param, grad, s1, s2, copy16, op + col, og + col, o1 + col, o2 + col, oc + col, re, g_re,
                             add);
        step_w<OPT, W, true>(s, param, grad, s1, s2, copy16, op + col + h, og + col + h, o1 + col + h, o2 + col + h,
                             oc + col + h, im, g_im, add);
      }
    } else {
      for (int u = gl; u < units; u += GROUP) {
        const int col = W * u;
        float x[W], pg[W];
        load_w<W>(x, param + op + col);
#pragma unroll
        for (int e = 0; e < W; ++e) pg[e] = c != 0u ? wpen_lp(x[e], q.p, f, c, vd) : 0.0f;
        step_w<OPT, W, true>(s, param, grad, s1, s2, copy16, op + col, og + col, o1 + col, o2 + col, oc + col, x, pg, add);
      }
    }
  }
  if (q.kind != 0) wpen_value_add(vd, q.value, part);  // (its barrier is also the one before the words are cleared)
  else __syncthreads();
  if (tid < WT_WORDS && raw != 0u) bitmap[word0 + tid] = 0u;
}

template <int OPT>
static int launch_touched_wpen(float* param, long long param_ld, float* grad, long long grad_ld, float* s1,
                               long long s1_ld, float* s2, long long s2_ld, unsigned int* bitmap, long long num_rows,
                               int dim, const StepArith& s, const kge_adam_clock* clock, unsigned short* copy16,
                               long long c_ld, const WPenRow& q, hipStream_t st) {
  const long long num_words = (num_rows + 31) / 32;
  const long long blocks = (num_words + WT_WORDS - 1) / WT_WORDS;
  // four floats per lane where every row of every array starts on 16 bytes (the bf16 copy: 8), one float otherwise
  const bool vec = dim % 4 == 0 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)s1 | (uintptr_t)s2) & 15) == 0 &&
                   param_ld % 4 == 0 && grad_ld % 4 == 0 && s1_ld % 4 == 0 && (s2 == nullptr || s2_ld % 4 == 0) &&
                   (copy16 == nullptr || (((uintptr_t)copy16 & 7) == 0 && c_ld % 4 == 0));
  const int units = vec ? dim / 4 : dim;
  const int group = units <= 16 ? 16 : (units <= 32 ? 32 : 64);
#define KGE_TW_LAUNCH(V, G)                                                                                          \
  hipLaunchKernelGGL((touched_wpen_kernel<V, G, OPT>), dim3((unsigned)blocks), dim3(256), 0, st, param, param_ld, grad, \
                     grad_ld, s1, s1_ld, s2, s2_ld, bitmap, num_rows, num_words, dim, s, clock, copy16, c_ld, q)
  if (vec) {
    if (group == 16) KGE_TW_LAUNCH(true, 16);
    else if (group == 32) KGE_TW_LAUNCH(true, 32);
    else KGE_TW_LAUNCH(true, 64);
  } else {
    if (group == 16) KGE_TW_LAUNCH(false, 16);
    else if (group == 32) KGE_TW_LAUNCH(false, 32);
    else KGE_TW_LAUNCH(false, 64);
  }
#undef KGE_TW_LAUNCH
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

static WPenRow wpen_row(const kge_wpenalty_seg& pen) {
  WPenRow q{};
  q.kind = pen.kind;
  if (pen.kind != 0) {
    q.p = pen.p;
    q.weight = pen.weight;
    q.fm = (float)pen.m;  // exact: m < 2^24
    q.counts = (unsigned int*)pen.counts;
    q.value = pen.value;
  }
  return q;
}

// Arguments are checked by the caller (api.hip: kge_adagrad_step_touched_wpenalty).
int run_adagrad_touched_wpen(float* param, long long param_ld, float* grad, long long grad_ld, float* sum,
                             long long sum_ld, unsigned int* bitmap, long long num_rows, int dim, float minus_clr,
                             float eps, unsigned short* copy16, long long c_ld, const kge_wpenalty_seg& pen,
                             hipStream_t st) {
  if (num_rows == 0) return KGE_OK;
  if (((num_rows + 31) / 32 + WT_WORDS - 1) / WT_WORDS > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  StepArith s{};
  s.c0 = minus_clr;
  s.eps = eps;
  return launch_touched_wpen<0>(param, param_ld, grad, grad_ld, sum, sum_ld, nullptr, 0, bitmap, num_rows, dim, s,
                                nullptr, copy16, c_ld, wpen_row(pen), st);
}

// the clock kernel of kge_sparse_adam_step_touched (touched.hip)
int run_sparse_adam_clock(kge_adam_clock* clock, double lr, double beta1, double beta2, hipStream_t st);

// Arguments are checked by the caller (api.hip: kge_sparse_adam_step_touched_wpenalty).  The clock: as
// run_sparse_adam_touched -- once per call, also for num_rows == 0; the grid is checked before it.
int run_sparse_adam_touched_wpen(float* param, long long param_ld, float* grad, long long grad_ld, float* m1,
                                 long long m1_ld, float* m2, long long m2_ld, unsigned int* bitmap, long long num_rows,
                                 int dim, kge_adam_clock* clock, double lr, double beta1, double beta2, float eps,
                                 unsigned short* copy16, long long c_ld, const kge_wpenalty_seg& pen, hipStream_t st) {
  if (((num_rows + 31) / 32 + WT_WORDS - 1) / WT_WORDS > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  const int rc = run_sparse_adam_clock(clock, lr, beta1, beta2, st);
  if (rc != KGE_OK) return rc;
  if (num_rows == 0) return KGE_OK;
  StepArith s{};
  // 1 - beta in double, then rounded: the weights torch derives from the Python floats
  s.c0 = (float)(1.0 - beta1);
  s.c1 = (float)(1.0 - beta2);
  s.eps = eps;
  return launch_touched_wpen<2>(param, param_ld, grad, grad_ld, m1, m1_ld, m2, m2_ld, bitmap, num_rows, dim, s, clock,
                                copy16, c_ld, wpen_row(pen), st);
}

}  // namespace kge
