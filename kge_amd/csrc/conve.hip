// conve.hip -- the evaluation network of ConvE (kge/model/conve.py:75-93) on gfx950 (conve_device.hpp; DESIGN.md
// section 32): kge_conve_queries.  Two kernels, no float atomics, no library call:
//
//   conve_partial_kernel   grid (row tiles of 32, 32 channels).  A workgroup builds ONE channel's slice of its rows'
//                          feature map in LDS -- gather of the two images, convolution, batch-norm 1, ReLU; the map
//                          never goes to memory -- and multiplies it by that channel's columns of proj_w on the float32
//                          matrix cores (v_mfma_f32_32x32x2_f32: M = the 32 rows, N = 32 outputs, K = the positions).
//                          A wave owns two blocks of 32 outputs per pass; a pass covers 256 outputs.  The partial
//                          [rows, d] goes to the workspace: ws[(c * n + row) * d + j].
//   conve_finish_kernel    a thread per output: the 32 partials in ascending channel order, proj_b, batch-norm 2, ReLU,
//                          q[i][1 + j]; the thread of j == 0 writes q[i][0] = 1.0f.
//
// A row's bits do not depend on n, its position, the index form, a pitch, an alignment or the launch: a row meets
// the other rows of its tile only as the M index of an MFMA, and the split (32 channels) is fixed.
#include "conve_device.hpp"

namespace kge {

struct CvNet {
  int h, w, pad, has_bias;
  int Ho, Wo, HW, d;
  const float* conv_w;
  const float* conv_b;
  const float* mean1;
  const float* var1;
  float eps1;
  const float* proj_w;
  long long proj_ld;
  const float* proj_b;
  const float* mean2;
  const float* var2;
  float eps2;
};

template <int FS>
__global__ __launch_bounds__(CV_THREADS) void conve_partial_kernel(CvNet net, const float* __restrict__ ent,
                                                                   long long ent_ld, const float* __restrict__ rel,
                                                                   long long rel_ld, Index s, Index p, long long n,
                                                                   float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float cv_smem[];  // [CV_TM][ldf]
  __shared__ const float* sE[CV_TM];
  __shared__ const float* sR[CV_TM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * CV_TM;
  const int HW = net.HW, ldf = cv_ldf(HW), KP = ldf - 1, d = net.d;

  if (tid < CV_TM) {
    const long long row = row0 + tid;
    const bool ok = row < n;
    sE[tid] = ok ? ent + index_at(s, row) * ent_ld + 1 : nullptr;
    sR[tid] = ok ? rel + index_at(p, row) * rel_ld + 1 : nullptr;
  }
  float wc[FS * FS];
#pragma unroll
  for (int i = 0; i < FS * FS; ++i) wc[i] = net.conv_w[c * FS * FS + i];
  const float bias = net.has_bias ? net.conv_b[c] : 0.0f;
  const float mean = net.mean1[c], rsq = cv_rsq(net.var1[c], net.eps1);
  __syncthreads();

  // the channel's slice: a lane per position, a wave takes the rows wv, wv + 4, ...; rows behind n and the positions
  // that pad the last group of eight are zeros
  for (int pos = lane; pos < KP; pos += 64) {
    const int y = pos / net.Wo, x = pos - y * net.Wo;
    for (int i = wv; i < CV_TM; i += CV_THREADS / 64) {
      float f = 0.0f;
      const float* es = sE[i];
      if (pos < HW && es != nullptr)
        f = cv_relu(cv_bn(cv_conv<FS>(es, sR[i], net.h, net.w, net.pad, y, x, wc, bias), mean, rsq));
      cv_smem[i * ldf + pos] = f;
    }
  }
  __syncthreads();

  // the projection: lane (i = lane & 31, kh = lane >> 5) holds A[i][k] and B[k][j = lane & 31] of position
  // k = 8 g + 4 kh + t in step t of group g
  const int li = lane & 31, kh = lane >> 5;
  const float* arow = cv_smem + li * ldf + 4 * kh;
  const long long koff = (long long)c * HW + 4 * kh;
  const int nblk = (d + 31) >> 5;
  for (int b0 = 0; b0 < nblk; b0 += 8) {
    const int bA = b0 + wv, bB = b0 + wv + 4;
    if (bA >= nblk) continue;  // (the whole wave: bA depends on the wave alone)
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
    // C: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
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

__global__ __launch_bounds__(256) void conve_finish_kernel(CvNet net, const float* __restrict__ ws, long long n,
                                                           float* __restrict__ q, long long q_ld) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int d = net.d;
  const long long row = t / d;
  const int j = (int)(t - row * d);
  if (row >= n) return;
  const float x = cv_finish(ws + row * d + j, n * d, net.proj_b[j]);
  q[row * q_ld + 1 + j] = cv_relu(cv_bn(x, net.mean2[j], cv_rsq(net.var2[j], net.eps2)));
  if (j == 0) q[row * q_ld] = 1.0f;
}

// what the gate of api.hip (check_conve) asks: does one channel's slice of 32 rows fit the LDS plan
bool conve_lds_ok(long long hw) { return hw >= 1 && ((hw + 7) & ~7LL) + 1 <= CV_MAX_LDF; }

long long conve_workspace_bytes(int d, long long n) { return (long long)CV_CHANNELS * n * d * (long long)sizeof(float); }

template <int FS>
static int cv_launch(const CvNet& net, const float* ent, long long ent_ld, const float* rel, long long rel_ld,
                     const Index& s, const Index& p, long long n, float* ws, hipStream_t st) {
  auto kern = conve_partial_kernel<FS>;
  const size_t lds = (size_t)CV_TM * cv_ldf(net.HW) * sizeof(float);
  if (lds > (size_t)CV_LDS_ASK) {
    // asked once per instantiation and device (the flags are plain bools: two host threads that launch at the same time
    // may both ask, which is harmless -- the call sets the same value; a device id of 64 or above asks on every launch).  The gate has already said the shape is supported (128 KiB + 512 B of
    // the CU's 160 KiB): a runtime that refuses is a launch error, not an unsupported shape
    static bool asked[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return KGE_ERR_LAUNCH;
    if (dev >= 64 || !asked[dev]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              CV_TM * CV_MAX_LDF * (int)sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return KGE_ERR_LAUNCH;
      }
      if (dev < 64) asked[dev] = true;
    }
  }
  const dim3 grid((unsigned)((n + CV_TM - 1) / CV_TM), CV_CHANNELS);
  hipLaunchKernelGGL(kern, grid, dim3(CV_THREADS), lds, st, net, ent, ent_ld, rel, rel_ld, s, p, n, ws);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

// n > 0, the gate passed, ws holds conve_workspace_bytes(d, n)
int run_conve_queries(const kge_conve_net* cn, const float* ent, long long ent_ld, const float* rel, long long rel_ld,
                      const Index& s, const Index& p, long long n, float* q, long long q_ld, float* ws, hipStream_t st) {
  CvNet net;
  net.h = cn->h; net.w = cn->w; net.pad = cn->padding; net.has_bias = cn->has_conv_bias ? 1 : 0;
  net.Ho = 2 * cn->h - cn->filter_size + 2 * cn->padding + 1;
  net.Wo = cn->w - cn->filter_size + 2 * cn->padding + 1;
  net.HW = net.Ho * net.Wo;
  net.d = cn->h * cn->w;
  net.conv_w = cn->conv_w; net.conv_b = cn->conv_b; net.mean1 = cn->bn1_mean; net.var1 = cn->bn1_var;
  net.eps1 = cn->bn1_eps;
  net.proj_w = cn->proj_w; net.proj_ld = cn->proj_ld; net.proj_b = cn->proj_b; net.mean2 = cn->bn2_mean;
  net.var2 = cn->bn2_var; net.eps2 = cn->bn2_eps;
  const long long tiles = (n + CV_TM - 1) / CV_TM, fblocks = (n * net.d + 255) / 256;
  if (tiles > 0x7fffffffLL || fblocks > 0x7fffffffLL) return KGE_ERR_UNSUPPORTED;
  int rc;
  switch (cn->filter_size) {
    case 1: rc = cv_launch<1>(net, ent, ent_ld, rel, rel_ld, s, p, n, ws, st); break;
    case 2: rc = cv_launch<2>(net, ent, ent_ld, rel, rel_ld, s, p, n, ws, st); break;
    case 3: rc = cv_launch<3>(net, ent, ent_ld, rel, rel_ld, s, p, n, ws, st); break;
    case 4: rc = cv_launch<4>(net, ent, ent_ld, rel, rel_ld, s, p, n, ws, st); break;
    case 5: rc = cv_launch<5>(net, ent, ent_ld, rel, rel_ld, s, p, n, ws, st); break;
    default: return KGE_ERR_UNSUPPORTED;
  }
  if (rc != KGE_OK) return rc;
  hipLaunchKernelGGL(conve_finish_kernel, dim3((unsigned)fblocks), dim3(256), 0, st, net, ws, n, q, q_ld);
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
