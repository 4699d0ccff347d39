// conve_train.hip -- the TRAINING-mode network of ConvE (kge/model/conve.py:81-93 under Module.train(): batch-norm on batch
// statistics, Dropout2d on the feature map, Dropout on the projection) and its backward on gfx950: kge_conve_train_fwd /
// kge_conve_train_bwd (include/kge_amd.h "ConvE, training").  float32, no float atomics, no library
// call; the arithmetic of conve_device.hpp ((v - mean) * rsq, cv_rsq, the MFMA chain, the channel order), so that with
// both probabilities 0 the forward's x carries the bits kge_conve_queries returns under the batch statistics.
//
// forward (the feature map [n, 32 Ho Wo] never goes to memory)
//   ct_stats_kernel        grid (row tiles of 32, 32 channels): the channel's convolution slice in LDS -> (count, mean, M2)
//   ct_stats_merge_kernel  the tiles in ascending order (Chan et al.) -> bn1_mean, bn1_var (biased)
//   ct_partial_kernel      conve_partial_kernel on dense rows under the batch (mean, rsq), the Dropout2d factor of
//                          (row, channel) applied as the slice is written; partials ws[(c * n + row) * d + j]
//   ct_finish_kernel       the 32 partials in channel order + proj_b, times the projection mask -> y[n, d] (saved)
//   ct_bn2_fwd_kernel      a workgroup per 64 columns: column statistics over the rows, x = relu((y - mean) * rsq)
// backward
//   ct_bn2_bwd_kernel      per 64 columns, two sweeps over the rows: g_u[n, d] (the gradient in front of the projection
//                          mask) and g_proj_b
//   ct_feature_bwd_kernel  grid (channel, block of 64 positions, blocks of 256 outputs): loops over ALL row tiles in order;
//                          per tile the activated slice a[32, 64] is rebuilt in LDS, g_a = g_u_tile . proj_w[:, block]
//                          (MFMA, K = d, proj_w[:, block] staged in LDS) and g_proj_w[:, block] += g_u_tile^T . a (MFMA,
//                          K = the 32 rows) in registers: one owner per element, one store at the end.  g_vhat[n, F] goes
//                          to the workspace -- the one feature-map-sized round trip of the step
//   ct_feature_merge_kernel  the blocks' (sum g_vhat, sum g_vhat vhat) in block order -> the channel's two means
//   ct_conv_bwd_kernel     grid over row tiles of 8: g_v = rsq (g_vhat - m1 - vhat m2), per-tile partials of g_conv_w /
//                          g_conv_b, the transposed convolution into the rows' two images -> g_s_emb, g_p_emb
//   ct_conv_merge_kernel   the tiles' partials in tile order -> g_conv_w, g_conv_b
#include "conve_device.hpp"
#include "philox.hpp"

namespace kge {

struct CtNet {
  int h, w, pad, has_bias;
  int Ho, Wo, HW, d;
  const float* conv_w;
  const float* conv_b;
  float eps1;
  const float* proj_w;
  long long proj_ld;
  const float* proj_b;
  float eps2;
};

struct CtRows {  // the dense embedded rows [n, d + 1]
  const float* s;
  long long s_ld;
  const float* p;
  long long p_ld;
  long long n;
};

constexpr unsigned CT_ROLE_FEATURE = 3, CT_ROLE_PROJ = 4;  // the `role` words of the two masks (include/kge_amd.h)
constexpr int CT_PB = 64;          // positions per workgroup of the feature backward
constexpr int CT_LDP = CT_PB + 1;  // their LDS pitch
constexpr int CT_JB = 256;         // outputs j per workgroup of the feature backward: 8 x 2 accumulator blocks, 4 a wave
constexpr int CT_RT = 8;           // rows per workgroup of the convolution backward
constexpr int CT_MAX_LDS = 156 * 1024;

// DropKey here: thr_ent / sc_ent = the feature map's Dropout2d, thr_rel / sc_rel = the projection's Dropout
__device__ __forceinline__ float ct_feature_factor(const DropKey& k, long long row, int c) {
  return drop_factor(c, RowMask{(unsigned)row, CT_ROLE_FEATURE, k.thr_ent, k.sc_ent}, k);
}
__device__ __forceinline__ float ct_proj_factor(const DropKey& k, long long row, int j) {
  return drop_factor(j, RowMask{(unsigned)row, CT_ROLE_PROJ, k.thr_rel, k.sc_rel}, k);
}

__device__ __forceinline__ float ct_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum over the 256 threads of a workgroup, the same bits in every thread: a butterfly per wave, the waves in order
__device__ __forceinline__ float ct_block_sum(float v, float* red) {
  v = ct_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <int FS>
__global__ __launch_bounds__(CV_THREADS) void ct_stats_kernel(CtNet net, CtRows R, float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float ct_smem[];  // [rows][ldf]: the convolution, before the norm
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * CV_TM;
  const int HW = net.HW, ldf = cv_ldf(HW);
  const int rows = (int)(R.n - row0 < CV_TM ? R.n - row0 : CV_TM);
  float wc[FS * FS];
#pragma unroll
  for (int i = 0; i < FS * FS; ++i) wc[i] = net.conv_w[c * FS * FS + i];
  const float bias = net.has_bias ? net.conv_b[c] : 0.0f;
  float s = 0.0f;
  for (int pos = lane; pos < HW; pos += 64) {
    const int y = pos / net.Wo, x = pos - y * net.Wo;
    for (int i = wv; i < rows; i += CV_THREADS / 64) {
      const float v = cv_conv<FS>(R.s + (row0 + i) * R.s_ld + 1, R.p + (row0 + i) * R.p_ld + 1, net.h, net.w, net.pad, y,
                                  x, wc, bias);
      ct_smem[i * ldf + pos] = v;
      s += v;
    }
  }
  const float cnt = (float)rows * (float)HW;
  const float mean = ct_block_sum(s, red) / cnt;
  float q = 0.0f;  // (a thread reads back what it wrote)
  for (int pos = lane; pos < HW; pos += 64)
    for (int i = wv; i < rows; i += CV_THREADS / 64) {
      const float dv = ct_smem[i * ldf + pos] - mean;
      q = __builtin_fmaf(dv, dv, q);
    }
  const float m2 = ct_block_sum(q, red);
  if (tid == 0) {
    float* o = stats + ((long long)blockIdx.x * CV_CHANNELS + c) * 3;
    o[0] = cnt; o[1] = mean; o[2] = m2;
  }
}

__global__ __launch_bounds__(64) void ct_stats_merge_kernel(const float* __restrict__ stats, long long tiles,
                                                            float* __restrict__ mean1, float* __restrict__ var1) {
  const int c = threadIdx.x;
  if (c >= CV_CHANNELS) return;
  float nA = stats[c * 3], mA = stats[c * 3 + 1], qA = stats[c * 3 + 2];
  for (long long t = 1; t < tiles; ++t) {
    const float* b = stats + (t * CV_CHANNELS + c) * 3;
    const float nB = b[0], delta = b[1] - mA, nAB = nA + nB;
    mA = mA + delta * (nB / nAB);
    qA = (qA + b[2]) + (delta * delta) * (nA * (nB / nAB));
    nA = nAB;
  }
  mean1[c] = mA;
  var1[c] = qA / nA;
}

template <int FS>
__global__ __launch_bounds__(CV_THREADS) void ct_partial_kernel(CtNet net, CtRows R, DropKey key,
                                                                const float* __restrict__ mean1,
                                                                const float* __restrict__ var1, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float ct_smem[];  // [CV_TM][ldf]
  __shared__ float sF[CV_TM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * CV_TM, n = R.n;
  const int HW = net.HW, ldf = cv_ldf(HW), KP = ldf - 1, d = net.d;
  if (tid < CV_TM) sF[tid] = row0 + tid < n ? ct_feature_factor(key, row0 + tid, c) : 0.0f;
  float wc[FS * FS];
#pragma unroll
  for (int i = 0; i < FS * FS; ++i) wc[i] = net.conv_w[c * FS * FS + i];
  const float bias = net.has_bias ? net.conv_b[c] : 0.0f;
  const float mean = mean1[c], rsq = cv_rsq(var1[c], net.eps1);
  __syncthreads();

  for (int pos = lane; pos < KP; pos += 64) {
    const int y = pos / net.Wo, x = pos - y * net.Wo;
    for (int i = wv; i < CV_TM; i += CV_THREADS / 64) {
      float f = 0.0f;
      if (pos < HW && row0 + i < n)
        f = cv_relu(cv_bn(cv_conv<FS>(R.s + (row0 + i) * R.s_ld + 1, R.p + (row0 + i) * R.p_ld + 1, net.h, net.w, net.pad,
                                      y, x, wc, bias), mean, rsq)) * sF[i];
      ct_smem[i * ldf + pos] = f;
    }
  }
  __syncthreads();

  // the projection: the chain of conve_partial_kernel (conve_device.hpp "projection")
  const int li = lane & 31, kh = lane >> 5;
  const float* arow = ct_smem + li * ldf + 4 * kh;
  const long long koff = (long long)c * HW + 4 * kh;
  const int nblk = (d + 31) >> 5;
  for (int b0 = 0; b0 < nblk; b0 += 8) {
    const int bA = b0 + wv, bB = b0 + wv + 4;
    if (bA >= nblk) continue;
    const int jA = bA * 32 + li, jB = bB * 32 + li;
    const bool okA = jA < d, okB = bB < nblk && jB < d;
    const float* wA = net.proj_w + (long long)(okA ? jA : 0) * net.proj_ld + koff;
    const float* wB = net.proj_w + (long long)(okB ? jB : 0) * net.proj_ld + koff;
    f32x16 accA, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) accA[r] = accB[r] = 0.0f;
    for (int k0 = 0; k0 < KP; k0 += 8) {
      const int kb = k0 + 4 * kh;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool kin = kb + t < HW;
        const float a = arow[k0 + t];
        const float vA = (okA && kin) ? wA[k0 + t] : 0.0f;
        const float vB = (okB && kin) ? wB[k0 + t] : 0.0f;
        accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a, vA, accA, 0, 0, 0);
        if (bB < nblk) accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a, vB, accB, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (row < n) {
        float* dst = ws + ((long long)c * n + row) * d;
        if (okA) dst[jA] = accA[r];
        if (okB) dst[jB] = accB[r];
      }
    }
  }
}

__global__ __launch_bounds__(256) void ct_finish_kernel(CtNet net, DropKey key, const float* __restrict__ ws, long long n,
                                                        float* __restrict__ y) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int d = net.d;
  const long long row = t / d;
  const int j = (int)(t - row * d);
  if (row >= n) return;
  y[row * d + j] = cv_finish(ws + row * d + j, n * d, net.proj_b[j]) * ct_proj_factor(key, row, j);
}

// the four row phases of a column, in order
__device__ __forceinline__ float ct_col_sum(float v, float (*red)[64], int ph, int cl) {
  __syncthreads();
  red[ph][cl] = v;
  __syncthreads();
  return ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

__global__ __launch_bounds__(256) void ct_bn2_fwd_kernel(int d, float eps2, const float* __restrict__ y, long long n,
                                                         float* __restrict__ x, long long x_ld, float* __restrict__ mean2,
                                                         float* __restrict__ var2) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const bool ok = col < d;
  float s = 0.0f;
  if (ok)
    for (long long row = ph; row < n; row += 4) s += y[row * d + col];
  const float mean = ct_col_sum(s, red, ph, cl) / (float)n;
  float q = 0.0f;
  if (ok)
    for (long long row = ph; row < n; row += 4) {
      const float dv = y[row * d + col] - mean;
      q = __builtin_fmaf(dv, dv, q);
    }
  const float var = ct_col_sum(q, red, ph, cl) / (float)n;
  if (!ok) return;
  const float rsq = cv_rsq(var, eps2);
  for (long long row = ph; row < n; row += 4) x[row * x_ld + col] = cv_relu(cv_bn(y[row * d + col], mean, rsq));
  if (ph == 0) {
    mean2[col] = mean;
    var2[col] = var;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ct_bn2_bwd_kernel(int d, float eps2, DropKey key, const float* __restrict__ y,
                                                         const float* __restrict__ g_x, long long gx_ld, long long n,
                                                         const float* __restrict__ mean2, const float* __restrict__ var2,
                                                         float* __restrict__ g_u, float* __restrict__ g_proj_b) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const bool ok = col < d;
  const float mean = ok ? mean2[col] : 0.0f, rsq = ok ? cv_rsq(var2[col], eps2) : 0.0f;
  float s1 = 0.0f, s2 = 0.0f;
  if (ok)
    for (long long row = ph; row < n; row += 4) {
      const float zh = cv_bn(y[row * d + col], mean, rsq);
      const float gz = zh > 0.0f ? g_x[row * gx_ld + col] : 0.0f;
      s1 += gz;
      s2 = __builtin_fmaf(gz, zh, s2);
    }
  const float m1 = ct_col_sum(s1, red, ph, cl) / (float)n;
  const float m2 = ct_col_sum(s2, red, ph, cl) / (float)n;
  float sb = 0.0f;
  if (ok)
    for (long long row = ph; row < n; row += 4) {
      const float zh = cv_bn(y[row * d + col], mean, rsq);
      const float gz = zh > 0.0f ? g_x[row * gx_ld + col] : 0.0f;
      const float gu = (rsq * ((gz - m1) - zh * m2)) * ct_proj_factor(key, row, col);
      g_u[row * d + col] = gu;
      sb += gu;
    }
  const float b = ct_col_sum(sb, red, ph, cl);
  if (ok && ph == 0) g_proj_b[col] = b;
}

template <int FS>
__global__ __launch_bounds__(CV_THREADS) void ct_feature_bwd_kernel(CtNet net, CtRows R, DropKey key,
                                                                    const float* __restrict__ mean1,
                                                                    const float* __restrict__ var1,
                                                                    const float* __restrict__ g_u,
                                                                    float* __restrict__ g_vhat,
                                                                    float* __restrict__ g_proj_w, long long gpw_ld,
                                                                    float* __restrict__ fsum, int w_in_lds) {
  extern __shared__ __attribute__((aligned(16))) float ct_smem[];
  __shared__ float red[4];
  __shared__ float sF[CV_TM];
  float* sa = ct_smem;                     // [32][CT_LDP] the activated slice (masked)
  float* svh = sa + CV_TM * CT_LDP;        // [32][CT_LDP] the normed slice in front of the ReLU
  float* sga = svh + CV_TM * CT_LDP;       // [2][32][CT_LDP] g_a of the two halves of K
  float* sw = sga + 2 * CV_TM * CT_LDP;    // [dpad][CT_LDP] proj_w[:, block] (w_in_lds)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, kh = lane >> 5;
  const int c = blockIdx.x, k0 = blockIdx.y * CT_PB, j0 = blockIdx.z * CT_JB;
  const bool first = blockIdx.z == 0;  // the workgroup that also forms g_vhat
  const int HW = net.HW, d = net.d, dpad = (d + 7) & ~7;
  const long long n = R.n, F = (long long)CV_CHANNELS * HW;
  const float* wcol = net.proj_w + (long long)c * HW;

  if (first && w_in_lds)
    for (int idx = tid; idx < dpad * CT_PB; idx += CV_THREADS) {
      const int j = idx >> 6, pos = idx & 63;
      sw[j * CT_LDP + pos] = (j < d && k0 + pos < HW) ? wcol[(long long)j * net.proj_ld + k0 + pos] : 0.0f;
    }
  float wc[FS * FS];
#pragma unroll
  for (int i = 0; i < FS * FS; ++i) wc[i] = net.conv_w[c * FS * FS + i];
  const float bias = net.has_bias ? net.conv_b[c] : 0.0f;
  const float mean = mean1[c], rsq = cv_rsq(var1[c], net.eps1);

  f32x16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
  float s1 = 0.0f, s2 = 0.0f;
  const int jA = j0 + wv * 64 + li, jB = jA + 32;  // the wave's two blocks of outputs
  const bool wave_on = j0 + wv * 64 < d;
  const int kpos = k0 + lane;  // (a) : a lane per position
  const int py = kpos / net.Wo, px = kpos - py * net.Wo;

  for (long long row0 = 0; row0 < n; row0 += CV_TM) {
    __syncthreads();  // the tile before is read
    if (tid < CV_TM) sF[tid] = row0 + tid < n ? ct_feature_factor(key, row0 + tid, c) : 0.0f;
    __syncthreads();
    // (a) the slice of this tile, rows behind n and positions behind HW zero
    for (int i = wv; i < CV_TM; i += CV_THREADS / 64) {
      float vh = 0.0f, a = 0.0f;
      if (kpos < HW && row0 + i < n) {
        vh = cv_bn(cv_conv<FS>(R.s + (row0 + i) * R.s_ld + 1, R.p + (row0 + i) * R.p_ld + 1, net.h, net.w, net.pad, py, px,
                               wc, bias), mean, rsq);
        a = cv_relu(vh) * sF[i];
      }
      sa[i * CT_LDP + lane] = a;
      svh[i * CT_LDP + lane] = vh;
    }
    __syncthreads();
    // (1) g_a[32 rows, 64 positions] = g_u_tile . proj_w[:, block]: wave = (position half nb, K half)
    if (first) {
      const int nb = wv & 1, half = wv >> 1;
      const int kmid = ((dpad / 8 + 1) / 2) * 8;
      const int jbeg = half ? kmid : 0, jend = half ? dpad : kmid;
      const bool rok = row0 + li < n;
      const float* gur = g_u + (rok ? row0 + li : 0) * d;
      const int pcol = nb * 32 + li;
      const bool pok = k0 + pcol < HW;
      f32x16 ga;
#pragma unroll
      for (int r = 0; r < 16; ++r) ga[r] = 0.0f;
      for (int jg = jbeg; jg < jend; jg += 8) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int j = jg + 4 * kh + t;
          const float a = (rok && j < d) ? gur[j] : 0.0f;
          float b;
          if (w_in_lds) b = sw[j * CT_LDP + pcol];
          else b = (j < d && pok) ? wcol[(long long)j * net.proj_ld + k0 + pcol] : 0.0f;
          ga = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, ga, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        sga[(half * CV_TM + (r & 3) + 8 * (r >> 2) + 4 * kh) * CT_LDP + pcol] = ga[r];
    }
    // (2) g_proj_w[j, position] += sum over the tile's rows of g_u[row][j] a[row][position]: K = the 32 rows
    if (wave_on) {
#pragma unroll 4
      for (int st = 0; st < CV_TM / 2; ++st) {
        const int k = 2 * st + kh;
        const long long row = row0 + k;
        const float a0 = (row < n && jA < d) ? g_u[row * d + jA] : 0.0f;
        const float a1 = (row < n && jB < d) ? g_u[row * d + jB] : 0.0f;
        const float b0 = sa[k * CT_LDP + li], b1 = sa[k * CT_LDP + 32 + li];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
      }
    }
    // (c) through the Dropout2d scale and the ReLU: g_vhat, and the channel's two sums
    if (first) {
      __syncthreads();
      if (kpos < HW)
        for (int i = wv; i < CV_TM; i += CV_THREADS / 64) {
          if (row0 + i >= n) break;
          const float vh = svh[i * CT_LDP + lane];
          const float ga = sga[i * CT_LDP + lane] + sga[(CV_TM + i) * CT_LDP + lane];
          const float gv = vh > 0.0f ? ga * sF[i] : 0.0f;
          g_vhat[(row0 + i) * F + (long long)c * HW + kpos] = gv;
          s1 += gv;
          s2 = __builtin_fmaf(gv, vh, s2);
        }
    }
  }

  if (wave_on) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + (q & 1) * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = (q < 2 ? jA - li : jB - li) + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (j < d && k < HW) g_proj_w[(long long)j * gpw_ld + (long long)c * HW + k] = acc[q][r];
      }
    }
  }
  if (first) {
    const float t1 = ct_block_sum(s1, red), t2 = ct_block_sum(s2, red);
    if (tid == 0) {
      float* o = fsum + ((long long)c * gridDim.y + blockIdx.y) * 2;
      o[0] = t1; o[1] = t2;
    }
  }
}

__global__ __launch_bounds__(64) void ct_feature_merge_kernel(const float* __restrict__ fsum, int nblk, float count,
                                                              float* __restrict__ m12) {
  const int c = threadIdx.x;
  if (c >= CV_CHANNELS) return;
  float s1 = 0.0f, s2 = 0.0f;
  for (int b = 0; b < nblk; ++b) {
    s1 += fsum[((long long)c * nblk + b) * 2];
    s2 += fsum[((long long)c * nblk + b) * 2 + 1];
  }
  m12[c] = s1 / count;
  m12[CV_CHANNELS + c] = s2 / count;
}

template <int FS>
__global__ __launch_bounds__(CV_THREADS) void ct_conv_bwd_kernel(CtNet net, CtRows R, const float* __restrict__ mean1,
                                                                 const float* __restrict__ var1,
                                                                 const float* __restrict__ g_vhat,
                                                                 const float* __restrict__ m12, float* __restrict__ wpart,
                                                                 float* __restrict__ g_s, long long gs_ld,
                                                                 float* __restrict__ g_p, long long gp_ld) {
  constexpr int TT = FS * FS + 1;  // the taps and the bias
  extern __shared__ __attribute__((aligned(16))) float ct_smem[];
  const int HW = net.HW, d = net.d, Wo = net.Wo, Ho = net.Ho, h = net.h, w = net.w, pad = net.pad;
  float* sgv = ct_smem;                // [CT_RT][HW] g_v of one channel
  float* simg = sgv + CT_RT * HW;      // [CT_RT][2 d] the gradient of the rows' stacked images
  float* sred = simg + CT_RT * 2 * d;  // [4][TT]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long row0 = (long long)blockIdx.x * CT_RT, n = R.n, F = (long long)CV_CHANNELS * HW;
  const int npix = CT_RT * 2 * d;

  for (int c = 0; c < CV_CHANNELS; ++c) {
    float wc[FS * FS], wa[FS * FS];
#pragma unroll
    for (int i = 0; i < FS * FS; ++i) {
      wc[i] = net.conv_w[c * FS * FS + i];
      wa[i] = 0.0f;
    }
    const float bias = net.has_bias ? net.conv_b[c] : 0.0f;
    const float mean = mean1[c], rsq = cv_rsq(var1[c], net.eps1), m1 = m12[c], m2 = m12[CV_CHANNELS + c];
    float ba = 0.0f;
    for (int e = tid; e < CT_RT * HW; e += CV_THREADS) {
      const int i = e / HW, k = e - i * HW;
      const long long row = row0 + i;
      float g = 0.0f;
      if (row < n) {
        const int y = k / Wo, x = k - y * Wo;
        const float* es = R.s + row * R.s_ld + 1;
        const float* rs = R.p + row * R.p_ld + 1;
        const float vh = cv_bn(cv_conv<FS>(es, rs, h, w, pad, y, x, wc, bias), mean, rsq);
        g = rsq * ((g_vhat[row * F + (long long)c * HW + k] - m1) - vh * m2);
        ba += g;
#pragma unroll
        for (int ky = 0; ky < FS; ++ky) {
          const int yy = y + ky - pad;
          if (yy < 0 || yy >= 2 * h) continue;
          const float* src = yy < h ? es + yy * w : rs + (yy - h) * w;
#pragma unroll
          for (int kx = 0; kx < FS; ++kx) {
            const int xx = x + kx - pad;
            if (xx >= 0 && xx < w) wa[ky * FS + kx] = __builtin_fmaf(g, src[xx], wa[ky * FS + kx]);
          }
        }
      }
      sgv[e] = g;
    }
#pragma unroll
    for (int i = 0; i < FS * FS; ++i) {
      const float v = ct_wave_sum(wa[i]);
      if (lane == 0) sred[wv * TT + i] = v;
    }
    ba = ct_wave_sum(ba);
    if (lane == 0) sred[wv * TT + FS * FS] = ba;
    __syncthreads();
    if (tid < TT)
      wpart[((long long)blockIdx.x * CV_CHANNELS + c) * TT + tid] =
          ((sred[tid] + sred[TT + tid]) + sred[2 * TT + tid]) + sred[3 * TT + tid];
    // the transposed convolution: a thread owns the pixels tid, tid + 256, ... through all channels
    for (int pix = tid; pix < npix; pix += CV_THREADS) {
      const int i = pix / (2 * d), r = pix - i * 2 * d;
      const int yy = r / w, xx = r - yy * w;
      const float* gv = sgv + i * HW;
      float a = 0.0f;
#pragma unroll
      for (int ky = 0; ky < FS; ++ky) {
        const int y = yy - ky + pad;
        if (y < 0 || y >= Ho) continue;
#pragma unroll
        for (int kx = 0; kx < FS; ++kx) {
          const int x = xx - kx + pad;
          if (x >= 0 && x < Wo) a = __builtin_fmaf(gv[y * Wo + x], wc[ky * FS + kx], a);
        }
      }
      simg[pix] = c == 0 ? a : simg[pix] + a;
    }
    __syncthreads();  // sgv and sred are free for the next channel
  }
  for (int pix = tid; pix < npix; pix += CV_THREADS) {
    const int i = pix / (2 * d), r = pix - i * 2 * d;
    const long long row = row0 + i;
    if (row >= n) continue;
    if (r < d) g_s[row * gs_ld + 1 + r] = simg[pix];
    else g_p[row * gp_ld + 1 + (r - d)] = simg[pix];
  }
  if (tid < CT_RT && row0 + tid < n) {
    g_s[(row0 + tid) * gs_ld] = 0.0f;
    g_p[(row0 + tid) * gp_ld] = 0.0f;
  }
}

__global__ __launch_bounds__(256) void ct_conv_merge_kernel(const float* __restrict__ wpart, long long tiles, int fs2,
                                                            float* __restrict__ g_conv_w, float* __restrict__ g_conv_b) {
  const int e = blockIdx.x * 256 + threadIdx.x, TT = fs2 + 1;
  if (e >= CV_CHANNELS * TT) return;
  const int c = e / TT, t = e - c * TT;
  float s = 0.0f;
  for (long long i = 0; i < tiles; ++i) s += wpart[(i * CV_CHANNELS + c) * TT + t];
  if (t < fs2) g_conv_w[c * fs2 + t] = s;
  else if (g_conv_b) g_conv_b[c] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------
static CtNet ct_net(const kge_conve_net* cn) {
  CtNet net;
  net.h = cn->h; net.w = cn->w; net.pad = cn->padding; net.has_bias = cn->has_conv_bias ? 1 : 0;
  net.Ho = 2 * cn->h - cn->filter_size + 2 * cn->padding + 1;
  net.Wo = cn->w - cn->filter_size + 2 * cn->padding + 1;
  net.HW = net.Ho * net.Wo;
  net.d = cn->h * cn->w;
  net.conv_w = cn->conv_w; net.conv_b = cn->conv_b; net.eps1 = cn->bn1_eps;
  net.proj_w = cn->proj_w; net.proj_ld = cn->proj_ld; net.proj_b = cn->proj_b; net.eps2 = cn->bn2_eps;
  return net;
}

// the workspace in floats.  forward: [partials 32 n d][tile statistics 96 tiles32]; backward: [g_u n d][g_vhat n F]
// [block sums 64 nblk][m1, m2: 64][tile partials of the convolution 32 (fs^2 + 1) tiles8]; one size serves both
struct CtLayout {
  long long tiles32, tiles8, nblk, stats, g_vhat, fsum, m12, wpart, floats;
};
static CtLayout ct_layout(int d, int hw, int fs, long long n) {
  CtLayout L;
  L.tiles32 = (n + CV_TM - 1) / CV_TM;
  L.tiles8 = (n + CT_RT - 1) / CT_RT;
  L.nblk = (hw + CT_PB - 1) / CT_PB;
  L.stats = (long long)CV_CHANNELS * n * d;
  const long long fwd = L.stats + 3 * CV_CHANNELS * L.tiles32;
  L.g_vhat = n * d;
  L.fsum = L.g_vhat + n * CV_CHANNELS * hw;
  L.m12 = L.fsum + 2 * CV_CHANNELS * L.nblk;
  L.wpart = L.m12 + 2 * CV_CHANNELS;
  const long long bwd = L.wpart + (long long)CV_CHANNELS * (fs * fs + 1) * L.tiles8;
  L.floats = fwd > bwd ? fwd : bwd;
  return L;
}

long long conve_train_workspace_bytes(int d, int hw, int fs, long long n) {
  return ct_layout(d, hw, fs, n).floats * (long long)sizeof(float);
}

template <typename K>
static bool ct_lds(K kern, size_t lds) {
  if (lds <= (size_t)CV_LDS_ASK) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          CT_MAX_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

static inline int ct_ok() { return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH; }

template <int FS>
static int ct_fwd(const CtNet& net, const CtRows& R, const DropKey& key, float* x, long long x_ld, float* y, float* mean1,
                  float* var1, float* mean2, float* var2, float* ws, hipStream_t st) {
  const long long n = R.n;
  const CtLayout L = ct_layout(net.d, net.HW, FS, n);
  const size_t lds = (size_t)CV_TM * cv_ldf(net.HW) * sizeof(float);
  if (!ct_lds(ct_stats_kernel<FS>, lds) || !ct_lds(ct_partial_kernel<FS>, lds)) return KGE_ERR_LAUNCH;
  const dim3 grid((unsigned)L.tiles32, CV_CHANNELS);
  float* stats = ws + L.stats;
  hipLaunchKernelGGL(ct_stats_kernel<FS>, grid, dim3(CV_THREADS), lds, st, net, R, stats);
  hipLaunchKernelGGL(ct_stats_merge_kernel, dim3(1), dim3(64), 0, st, stats, L.tiles32, mean1, var1);
  hipLaunchKernelGGL(ct_partial_kernel<FS>, grid, dim3(CV_THREADS), lds, st, net, R, key, mean1, var1, ws);
  hipLaunchKernelGGL(ct_finish_kernel, dim3((unsigned)((n * net.d + 255) / 256)), dim3(256), 0, st, net, key, ws, n, y);
  hipLaunchKernelGGL(ct_bn2_fwd_kernel, dim3((unsigned)((net.d + 63) / 64)), dim3(256), 0, st, net.d, net.eps2, y, n, x,
                     x_ld, mean2, var2);
  return ct_ok();
}

template <int FS>
static int ct_bwd(const CtNet& net, const CtRows& R, const DropKey& key, const float* g_x, long long gx_ld, const float* y,
                  const float* mean1, const float* var1, const float* mean2, const float* var2, float* g_s,
                  long long gs_ld, float* g_p, long long gp_ld, float* g_conv_w, float* g_conv_b, float* g_proj_w,
                  long long gpw_ld, float* g_proj_b, float* ws, hipStream_t st) {
  const long long n = R.n;
  const int d = net.d, dpad = (d + 7) & ~7;
  const CtLayout L = ct_layout(d, net.HW, FS, n);
  float* g_u = ws;
  float* g_vhat = ws + L.g_vhat;
  float* fsum = ws + L.fsum;
  float* m12 = ws + L.m12;
  float* wpart = ws + L.wpart;
  const size_t fixed = (size_t)4 * CV_TM * CT_LDP * sizeof(float), wbytes = (size_t)dpad * CT_LDP * sizeof(float);
  const int w_in_lds = fixed + wbytes <= (size_t)CT_MAX_LDS ? 1 : 0;
  const size_t lds_f = fixed + (w_in_lds ? wbytes : 0);
  const size_t lds_c = ((size_t)CT_RT * (net.HW + 2 * d) + 4 * (FS * FS + 1)) * sizeof(float);
  if (!ct_lds(ct_feature_bwd_kernel<FS>, lds_f) || !ct_lds(ct_conv_bwd_kernel<FS>, lds_c)) return KGE_ERR_LAUNCH;
  hipLaunchKernelGGL(ct_bn2_bwd_kernel, dim3((unsigned)((d + 63) / 64)), dim3(256), 0, st, d, net.eps2, key, y, g_x, gx_ld,
                     n, mean2, var2, g_u, g_proj_b);
  hipLaunchKernelGGL(ct_feature_bwd_kernel<FS>, dim3(CV_CHANNELS, (unsigned)L.nblk, (unsigned)((d + CT_JB - 1) / CT_JB)),
                     dim3(CV_THREADS), lds_f, st, net, R, key, mean1, var1, g_u, g_vhat, g_proj_w, gpw_ld, fsum, w_in_lds);
  hipLaunchKernelGGL(ct_feature_merge_kernel, dim3(1), dim3(64), 0, st, fsum, (int)L.nblk, (float)n * (float)net.HW, m12);
  hipLaunchKernelGGL(ct_conv_bwd_kernel<FS>, dim3((unsigned)L.tiles8), dim3(CV_THREADS), lds_c, st, net, R, mean1, var1,
                     g_vhat, m12, wpart, g_s, gs_ld, g_p, gp_ld);
  hipLaunchKernelGGL(ct_conv_merge_kernel, dim3((unsigned)((CV_CHANNELS * (FS * FS + 1) + 255) / 256)), dim3(256), 0, st,
                     wpart, L.tiles8, FS * FS, g_conv_w, net.has_bias ? g_conv_b : nullptr);
  return ct_ok();
}

#define CT_DISPATCH(fs, call)                                  \
  switch (fs) {                                                \
    case 1: { constexpr int FS = 1; return call; }             \
    case 2: { constexpr int FS = 2; return call; }             \
    case 3: { constexpr int FS = 3; return call; }             \
    case 4: { constexpr int FS = 4; return call; }             \
    case 5: { constexpr int FS = 5; return call; }             \
    default: return KGE_ERR_UNSUPPORTED;                       \
  }

// n >= 2, the gate passed, ws holds conve_train_workspace_bytes
int run_conve_train_fwd(const kge_conve_net* cn, const DropKey& key, const float* s_emb, long long s_ld,
                        const float* p_emb, long long p_ld, long long n, float* x, long long x_ld, float* y, float* mean1,
                        float* var1, float* mean2, float* var2, float* ws, hipStream_t st) {
  const CtNet net = ct_net(cn);
  const CtRows R{s_emb, s_ld, p_emb, p_ld, n};
  CT_DISPATCH(cn->filter_size, ct_fwd<FS>(net, R, key, x, x_ld, y, mean1, var1, mean2, var2, ws, st));
}

int run_conve_train_bwd(const kge_conve_net* cn, const DropKey& key, const float* s_emb, long long s_ld,
                        const float* p_emb, long long p_ld, long long n, const float* g_x, long long gx_ld, const float* y,
                        const float* mean1, const float* var1, const float* mean2, const float* var2, float* g_s,
                        long long gs_ld, float* g_p, long long gp_ld, float* g_conv_w, float* g_conv_b, float* g_proj_w,
                        long long gpw_ld, float* g_proj_b, float* ws, hipStream_t st) {
  const CtNet net = ct_net(cn);
  const CtRows R{s_emb, s_ld, p_emb, p_ld, n};
  CT_DISPATCH(cn->filter_size, ct_bwd<FS>(net, R, key, g_x, gx_ld, y, mean1, var1, mean2, var2, g_s, gs_ld, g_p, gp_ld,
                                          g_conv_w, g_conv_b, g_proj_w, gpw_ld, g_proj_b, ws, st));
}

}  // namespace kge
