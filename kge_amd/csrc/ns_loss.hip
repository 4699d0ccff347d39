// ns_loss.hip -- BCEWithLogitsKgeLoss over the [n, 1 + K] score block of a negative-sampling slot
// (kge/util/loss.py:136-189 on the scores TrainingJobNegativeSampling._process_subbatch assembles,
// train_negative_sampling.py:120-151: column 0 = the positive, columns 1.. = its negatives), forward and gradient
// in ONE pass over the block:
//   kind 0  "bce"                   sum_j l(x_j, y_j)                                      (reduction "sum")
//   kind 1  "bce_mean"              ( l(x_0, 1) + sum_{j>=1} l(x_j, 0) / K ) / 2           (loss.py:160-168)
//   kind 2  "bce_self_adversarial"  ( l(x_0, 1) + sum_{j>=1} w_j l(x_j, 0) ) / 2,  w = softmax_j(T x_j), detached
//                                                                                          (loss.py:169-186)
// with x = score + offset (train.loss_arg, loss.py:153-154) and l = torch's BCEWithLogitsLoss element:
// (1 - y) x + m + log(exp(-m) + exp(-x - m)), m = max(-x, 0).  The reference spends ~15 launches per slot on this, and
// the self-adversarial form two torch.nonzero calls = two device -> host waits per slot and step.
// One wave per row; HBM-bound on a 2 MB block (n = 512, K = 1000): read once, gradient written once.
//
// ns_loss_kernel below: the same row structure for ALL of LibKGE's negative-sampling losses, on the positive and the
// negatives as TWO pieces (pos with an element stride, neg [n, K] with a leading dimension; the gradient goes out the
// same way), so that a caller holding the positives' vector and a slot's [n, K] block needs no concatenation:
//   kinds 0-2  the bce family above, the same arithmetic in the same order (arg = offset)
//   kind 3  "kl"              lse_j(x_j) - x_0                   KLDivWithSoftmaxKgeLoss on the label matrix "column 0
//                                                                is 1" (loss.py:211-213; 0 log 0 = 0)
//           d / d x_j = softmax(x)_j - [j = 0];  two passes over the row (max, then sum) like kind 2's weights
//   kind 4  "margin_ranking"  sum_{j>=1} max(-(x_0 - x_j) + margin, 0)       MarginRankingKgeLoss (loss.py:236-252),
//           evaluated in torch's order in float32: t = x_0 - x_j, v = -t + margin, clamp_min(v, 0); arg = margin.
//           d / d x_j = [v_j >= 0] (torch's clamp_min subgradient: ACTIVE at the exact tie v = 0),
//           d / d x_0 = -#{j : v_j >= 0} (a count: exact in float32 below 2^24 negatives)
//   kind 5  "soft_margin"     sum_j log(1 + exp(z_j)), z_j = -t_j x_j, t_0 = 1, t_j = -1   SoftMarginKgeLoss
//           (loss.py:221-224) in the overflow-safe form max(z, 0) + log1p(exp(-|z|)): the reference's log(1 + exp(z))
//           is inf from z ~ 89 in float32 (and its gradient inf / inf).  d / d x_j = -t_j sigmoid(z_j)
//   kind 6  "se"              sum_j (x_j - y_j)^2, y_0 = 1, y_j = 0          SEKgeLoss (loss.py:272-274)
//           d / d x_j = 2 (x_j - y_j)
// The new kinds use the accurate expf / logf / log1pf (the block is read once either way).  No atomics: a row is one
// wave's, the reduction a fixed butterfly -- two runs give the same bits.
#include "common.hpp"

namespace kge {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float bce_elem(float x, float y) {
  const float m = __builtin_fmaxf(-x, 0.0f);
  return (1.0f - y) * x + m + __logf(__expf(-m) + __expf(-x - m));
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + __expf(-x)); }

template <int KIND>
__global__ __launch_bounds__(256) void ns_bce_kernel(const float* __restrict__ sc, long long ld, long long n, long long c,
                                                     float offset, float temp, float* __restrict__ loss_rows,
                                                     float* __restrict__ grad, long long ldg) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* x = sc + row * ld;
  float* g = grad ? grad + row * ldg : nullptr;
  const float K = (float)(c - 1);
  float wmax = -__builtin_inff(), wsum = 0.0f;
  if (KIND == 2) {  // softmax statistics of the negatives' T (x + offset)
    for (long long j = 1 + lane; j < c; j += 64) wmax = __builtin_fmaxf(wmax, temp * (x[j] + offset));
    wmax = wave_max(wmax);
    for (long long j = 1 + lane; j < c; j += 64) wsum += __expf(temp * (x[j] + offset) - wmax);
    wsum = wave_sum(wsum);
  }
  float acc = 0.0f;
  for (long long j = lane; j < c; j += 64) {
    const float v = x[j] + offset;
    const float y = j == 0 ? 1.0f : 0.0f;
    const float l = bce_elem(v, y);
    const float d = sigmoidf(v) - y;  // d l / d x
    float w;
    if (KIND == 0) w = 1.0f;
    else if (KIND == 1) w = j == 0 ? 0.5f : 0.5f / K;
    else w = j == 0 ? 0.5f : 0.5f * __expf(temp * v - wmax) / wsum;
    acc += w * l;
    if (g) g[j] = w * d;
  }
  acc = wave_sum(acc);
  if (lane == 0) loss_rows[row] = acc;
}

int run_ns_bce(int kind, const float* scores, long long ld, long long n, long long c, float offset, float temp,
               float* loss_rows, float* grad, long long ldg, hipStream_t st) {
  if (n == 0) return KGE_OK;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  if (kind == 0) hipLaunchKernelGGL(ns_bce_kernel<0>, grid, block, 0, st, scores, ld, n, c, offset, temp, loss_rows, grad, ldg);
  else if (kind == 1) hipLaunchKernelGGL(ns_bce_kernel<1>, grid, block, 0, st, scores, ld, n, c, offset, temp, loss_rows, grad, ldg);
  else hipLaunchKernelGGL(ns_bce_kernel<2>, grid, block, 0, st, scores, ld, n, c, offset, temp, loss_rows, grad, ldg);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

template <int KIND>
__global__ __launch_bounds__(256) void ns_loss_kernel(const float* __restrict__ pos, long long pos_stride,
                                                      const float* __restrict__ neg, long long neg_ld, long long n,
                                                      long long c, float arg, float temp, float* __restrict__ loss_rows,
                                                      float* __restrict__ g_pos, long long g_pos_stride,
                                                      float* __restrict__ g_neg, long long g_neg_ld) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float x0 = pos[row * pos_stride];
  const float* xn = neg + row * neg_ld;  // xn[j - 1] = x_j, j >= 1
  float* gn = g_neg ? g_neg + row * g_neg_ld : nullptr;
  const auto at = [&](long long j) { return j == 0 ? x0 : xn[j - 1]; };
  const auto put = [&](long long j, float v) {
    if (j == 0) g_pos[row * g_pos_stride] = v;
    else gn[j - 1] = v;
  };
  float acc = 0.0f;
  if (KIND <= 2) {  // ns_bce_kernel's arithmetic, operation for operation
    const float offset = arg;
    const float K = (float)(c - 1);
    float wmax = -__builtin_inff(), wsum = 0.0f;
    if (KIND == 2) {
      for (long long j = 1 + lane; j < c; j += 64) wmax = __builtin_fmaxf(wmax, temp * (xn[j - 1] + offset));
      wmax = wave_max(wmax);
      for (long long j = 1 + lane; j < c; j += 64) wsum += __expf(temp * (xn[j - 1] + offset) - wmax);
      wsum = wave_sum(wsum);
    }
    for (long long j = lane; j < c; j += 64) {
      const float v = at(j) + offset;
      const float y = j == 0 ? 1.0f : 0.0f;
      const float l = bce_elem(v, y);
      const float d = sigmoidf(v) - y;
      float w;
      if (KIND == 0) w = 1.0f;
      else if (KIND == 1) w = j == 0 ? 0.5f : 0.5f / K;
      else w = j == 0 ? 0.5f : 0.5f * __expf(temp * v - wmax) / wsum;
      acc += w * l;
      if (gn) put(j, w * d);
    }
    acc = wave_sum(acc);
  } else if (KIND == 3) {  // kl: lse(x) - x_0
    float mx = -__builtin_inff(), sum = 0.0f;
    for (long long j = lane; j < c; j += 64) mx = __builtin_fmaxf(mx, at(j));
    mx = wave_max(mx);
    for (long long j = lane; j < c; j += 64) sum += expf(at(j) - mx);
    sum = wave_sum(sum);
    acc = (mx - x0) + logf(sum);  // (mx - x_0 is the large part and exact-ish; log(sum) in [0, log c])
    if (gn) {
      const float inv = 1.0f / sum;
      for (long long j = lane; j < c; j += 64) put(j, expf(at(j) - mx) * inv - (j == 0 ? 1.0f : 0.0f));
    }
  } else if (KIND == 4) {  // margin ranking: torch's order t = x_0 - x_j, v = -t + margin, clamp_min(v, 0)
    float cnt = 0.0f;
    for (long long j = 1 + lane; j < c; j += 64) {
      const float t = x0 - xn[j - 1];
      const float v = -t + arg;
      const bool active = v >= 0.0f;  // torch's clamp_min backward: grad * (v >= min) -- the tie is active
      acc += active ? v : 0.0f;
      cnt += active ? 1.0f : 0.0f;
      if (gn) gn[j - 1] = active ? 1.0f : 0.0f;
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);  // whole numbers: exact
    if (gn && lane == 0) g_pos[row * g_pos_stride] = -cnt;
  } else if (KIND == 5) {  // soft margin, overflow-safe
    for (long long j = lane; j < c; j += 64) {
      const float t = j == 0 ? 1.0f : -1.0f;
      const float z = -t * at(j);
      const float e = expf(-__builtin_fabsf(z));  // in (0, 1]
      acc += __builtin_fmaxf(z, 0.0f) + log1pf(e);
      if (gn) put(j, -t * ((z >= 0.0f ? 1.0f : e) / (1.0f + e)));  // sigmoid(z) without an overflow
    }
    acc = wave_sum(acc);
  } else {  // se
    for (long long j = lane; j < c; j += 64) {
      const float d = at(j) - (j == 0 ? 1.0f : 0.0f);
      acc += d * d;
      if (gn) put(j, 2.0f * d);
    }
    acc = wave_sum(acc);
  }
  if (lane == 0) loss_rows[row] = acc;
}

int run_ns_loss(int kind, const float* pos, long long pos_stride, const float* neg, long long neg_ld, long long n,
                long long K, float arg, float temp, float* loss_rows, float* g_pos, long long g_pos_stride, float* g_neg,
                long long g_neg_ld, hipStream_t st) {
  if (n == 0) return KGE_OK;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
#define KGE_NS_LOSS_LAUNCH(KIND)                                                                                       \
  hipLaunchKernelGGL(ns_loss_kernel<KIND>, grid, block, 0, st, pos, pos_stride, neg, neg_ld, n, K + 1, arg, temp,     \
                     loss_rows, g_pos, g_pos_stride, g_neg, g_neg_ld)
  switch (kind) {
    case 0: KGE_NS_LOSS_LAUNCH(0); break;
    case 1: KGE_NS_LOSS_LAUNCH(1); break;
    case 2: KGE_NS_LOSS_LAUNCH(2); break;
    case 3: KGE_NS_LOSS_LAUNCH(3); break;
    case 4: KGE_NS_LOSS_LAUNCH(4); break;
    case 5: KGE_NS_LOSS_LAUNCH(5); break;
    case 6: KGE_NS_LOSS_LAUNCH(6); break;
    default: return KGE_ERR_INVALID_ARG;
  }
#undef KGE_NS_LOSS_LAUNCH
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
