// kvsall_collate.hip -- a KvsAll batch built on the device: what the collate function of TrainingJobKvsAll does on the
// host per batch (kge/job/train_KvsAll.py:118-201: a Python loop over the batch's examples, two passes, per-example
// slice assignments into queries / label_coords / triples) and what the plugin then did to it (bincount, cumsum,
// nonzero per query type, repeat_interleave and a gather: the per-type CSR of the fused losses, padded for the captured
// step).  The index arrays (KvsAllIndex._keys, _values_offset, _values of every query type) live on the device; only the
// batch's example numbers cross the bus.  Integer work only, no atomics.
//
// Two launches on the caller's stream:
//   1. scan   ONE workgroup of 1024 threads (16 waves of 64) walks the batch in chunks of 1024 rows.  Per row: its
//             query type (the example number against the types' boundaries), its key and its label count.  Per chunk
//             four exclusive scans over the workgroup -- the rows of each type (three counters packed into one 64-bit
//             word, 20 bits each: a chunk holds at most 1024 rows) and the label count of each type -- as wave scans by
//             __shfl_up plus 16 wave totals in LDS (128 bytes), with running totals carried from chunk to chunk in
//             registers (125 VGPRs, no scratch: 16 waves fit one CU).  That gives every row its typed row number, its typed label start and its batch label start
//             (the sum of the three typed starts).  Written: queries, query_type, the typed ids / rowptr / weight /
//             rows, then the padding rows, counts, and the two per-row label starts in the workspace.
//   2. copy   label position j of the batch -> its row by a binary search in the workspace's batch label starts
//             ([n + 1], a few KiB, cache resident), then label_coords[j], triples[j] and the typed col entry.  A
//             workgroup of 256 threads takes a piece of 1024 positions, so a long row is spread over several
//             workgroups.  Further workgroups zero each typed col beyond its labels.
// Every store is checked against the extent the caller stated (nnz_cap, rows_cap, lab_cap): a batch that does not fit
// writes less, never elsewhere.
#include "common.hpp"

namespace kge {

struct CollateType {
  const long long* keys;     // [M, 2]
  const long long* offsets;  // [M + 1]
  const long long* values;   // [offsets[M]]
  long long first, last;     // the type's example numbers [first, last)
  int q0_col, q1_col, target_col;
};

struct CollateTyped {
  long long* ids;
  long long* rowptr;
  long long* col;
  float* weight;
  long long* rows;
  long long rows_cap, lab_cap;
  long long fill_block0;  // first workgroup of this type's zero fill in the copy launch
};

struct CollateArgs {
  CollateType type[3];
  CollateTyped typed[3];
  int num_types;
  int want_typed;
  const long long* examples;
  long long n, nnz_cap, num_examples;
  long long* queries;
  long long* query_type;
  int* label_coords;
  long long* triples;
  float weight;
  long long* counts;
  long long* ws;  // [n + 1] batch label starts | [n] typed label starts | [3] labels per type
  long long copy_blocks;
};

constexpr int kScanThreads = 1024, kCopyThreads = 256, kCopyPiece = 1024;

// exclusive scan of v over the workgroup (kScanThreads) and the workgroup's total; `tot` is 16 words of LDS
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long* tot, long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) tot[wave] = inc;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const long long x = tot[w];
    if (w < wave) before += x;
    all += x;
  }
  __syncthreads();  // (tot is reused by the next scan)
  total = all;
  return before + inc - v;
}

// the type of example number ex (clamped into [0, num_examples)): its index and everything of its descriptor
__device__ __forceinline__ int type_of(const CollateArgs& a, long long ex, CollateType& ty) {
  int t = 0;
  ty = a.type[0];
#pragma unroll
  for (int u = 1; u < 3; ++u)
    if (u < a.num_types && ex >= a.type[u].first && a.type[u].last > a.type[u].first) {  // (an empty type owns nothing)
      t = u;
      ty = a.type[u];
    }
  return t;
}

__device__ __forceinline__ long long clamp_example(const CollateArgs& a, long long ex) {
  return ex < 0 ? 0 : (ex >= a.num_examples ? a.num_examples - 1 : ex);
}

__global__ __launch_bounds__(kScanThreads) void kvsall_collate_scan_kernel(CollateArgs a) {
  __shared__ long long tot[kScanThreads / 64];
  const int tid = threadIdx.x;
  long long* gstart = a.ws;
  long long* tstart = a.ws + a.n + 1;
  long long carry_n[3] = {0, 0, 0}, carry_d[3] = {0, 0, 0};
  for (long long base = 0; base < a.n; base += kScanThreads) {
    const long long i = base + tid;
    int t = -1;
    long long deg = 0, k0 = 0, k1 = 0;
    if (i < a.n) {
      const long long ex = clamp_example(a, a.examples[i]);
      CollateType ty;
      t = type_of(a, ex, ty);
      const long long e = ex - ty.first;
      deg = ty.offsets[e + 1] - ty.offsets[e];
      k0 = ty.keys[2 * e];
      k1 = ty.keys[2 * e + 1];
    }
    long long tot_c, exc_d[3] = {0, 0, 0}, tot_d[3] = {0, 0, 0};
    const long long exc_c = block_exclusive_scan(t < 0 ? 0ll : 1ll << (20 * t), tot, tot_c);
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (u < a.num_types) exc_d[u] = block_exclusive_scan(t == u ? deg : 0ll, tot, tot_d[u]);
    if (i < a.n) {
      long long r = 0, ls = 0, g = 0;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        g += carry_d[u] + exc_d[u];
        if (t == u) {
          r = carry_n[u] + ((exc_c >> (20 * u)) & 0xFFFFF);
          ls = carry_d[u] + exc_d[u];
        }
      }
      gstart[i] = g;
      tstart[i] = ls;
      if (a.queries) {
        a.queries[2 * i] = k0;
        a.queries[2 * i + 1] = k1;
        a.query_type[i] = t;
      }
      if (a.want_typed) {
#pragma unroll
        for (int u = 0; u < 3; ++u)
          if (t == u) {
            const CollateTyped& T = a.typed[u];
            if (r <= T.rows_cap) T.rowptr[r] = ls;
            if (r < T.rows_cap) {
              T.ids[2 * r] = k0;
              T.ids[2 * r + 1] = k1;
              if (T.weight) T.weight[r] = a.weight;
              if (T.rows) T.rows[r] = i;
            }
          }
      }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      carry_n[u] += (tot_c >> (20 * u)) & 0xFFFFF;
      carry_d[u] += tot_d[u];
    }
  }
  // every thread holds the same totals: rows and labels per type
  if (tid == 0) {
    gstart[a.n] = carry_d[0] + carry_d[1] + carry_d[2];
    for (int u = 0; u < 3; ++u) a.ws[2 * a.n + 1 + u] = carry_d[u];
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (u >= a.num_types) continue;
    const long long nu = carry_n[u], zu = carry_d[u];
    long long fits = 1;
    if (a.want_typed) {
      const CollateTyped& T = a.typed[u];
      fits = nu <= T.rows_cap && zu + (T.rows_cap - nu) <= T.lab_cap;
      // padding rows: query (0, 0) with the single label 0, weight 0, batch row -1
      for (long long r = nu + tid; r <= T.rows_cap; r += kScanThreads) {
        T.rowptr[r] = zu + (r - nu);
        if (r < T.rows_cap) {
          T.ids[2 * r] = 0;
          T.ids[2 * r + 1] = 0;
          if (T.weight) T.weight[r] = 0.0f;
          if (T.rows) T.rows[r] = -1;
        }
      }
    }
    if (a.counts && tid == 0) {
      a.counts[3 * u] = nu;
      a.counts[3 * u + 1] = zu;
      a.counts[3 * u + 2] = fits;
    }
  }
}

__global__ __launch_bounds__(kCopyThreads) void kvsall_collate_copy_kernel(CollateArgs a) {
  const long long* gstart = a.ws;
  const long long* tstart = a.ws + a.n + 1;
  const long long b = blockIdx.x;
  if (b < a.copy_blocks) {
    long long nnz = gstart[a.n];
    if (nnz > a.nnz_cap) nnz = a.nnz_cap;
#pragma unroll
    for (int k = 0; k < kCopyPiece / kCopyThreads; ++k) {
      const long long j = b * kCopyPiece + k * kCopyThreads + threadIdx.x;
      if (j >= nnz) continue;
      long long lo = 0, hi = a.n;  // gstart[lo] <= j < gstart[hi]: rows without labels are stepped over
      while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (gstart[mid] <= j) lo = mid;
        else hi = mid;
      }
      const long long i = lo, within = j - gstart[i];
      const long long ex = clamp_example(a, a.examples[i]);
      CollateType ty;
      const int t = type_of(a, ex, ty);
      const long long e = ex - ty.first;
      const long long v = ty.values[ty.offsets[e] + within];
      if (a.label_coords) {
        a.label_coords[2 * j] = (int)i;
        a.label_coords[2 * j + 1] = (int)v;
        a.triples[3 * j + ty.q0_col] = ty.keys[2 * e];
        a.triples[3 * j + ty.q1_col] = ty.keys[2 * e + 1];
        a.triples[3 * j + ty.target_col] = v;
      }
      if (a.want_typed) {
        const long long p = tstart[i] + within;
#pragma unroll
        for (int u = 0; u < 3; ++u)
          if (t == u && p < a.typed[u].lab_cap) a.typed[u].col[p] = v;
      }
    }
    return;
  }
  // zero fill of a typed col beyond its labels (the labels of the padding rows included)
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (u >= a.num_types) continue;
    const CollateTyped& T = a.typed[u];
    const long long fb = b - T.fill_block0, nblk = (T.lab_cap + kCopyPiece - 1) / kCopyPiece;
    if (fb < 0 || fb >= nblk) continue;
    const long long zu = a.ws[2 * a.n + 1 + u];
#pragma unroll
    for (int k = 0; k < kCopyPiece / kCopyThreads; ++k) {
      const long long p = fb * kCopyPiece + k * kCopyThreads + threadIdx.x;
      if (p >= zu && p < T.lab_cap) T.col[p] = 0;
    }
  }
}

long long kvsall_collate_workspace_bytes(long long n) { return (2 * n + 4) * (long long)sizeof(long long); }

int run_kvsall_collate(const kge_kvsall_index* types, int num_types, const long long* examples, long long n,
                       long long nnz_cap, long long* queries, long long* query_type, int* label_coords,
                       long long* triples, const kge_kvsall_typed* typed, float weight, long long* counts, void* ws,
                       hipStream_t st) {
  CollateArgs a{};
  long long first = 0, blocks = (nnz_cap + kCopyPiece - 1) / kCopyPiece;
  a.copy_blocks = blocks;
  for (int u = 0; u < num_types; ++u) {
    CollateType& ty = a.type[u];
    ty.keys = (const long long*)types[u].keys;
    ty.offsets = (const long long*)types[u].offsets;
    ty.values = (const long long*)types[u].values;
    ty.first = first;
    ty.last = first = types[u].last;
    ty.target_col = types[u].target_col;
    ty.q0_col = ty.target_col == 0 ? 1 : 0;  // the two key columns take the remaining triple columns in S, P, O order
    ty.q1_col = ty.target_col == 2 ? 1 : 2;
    if (typed) {
      CollateTyped& T = a.typed[u];
      T.ids = (long long*)typed[u].ids;
      T.rowptr = (long long*)typed[u].rowptr;
      T.col = (long long*)typed[u].col;
      T.weight = typed[u].weight;
      T.rows = (long long*)typed[u].rows;
      T.rows_cap = typed[u].rows_cap;
      T.lab_cap = typed[u].lab_cap;
      T.fill_block0 = blocks;
      blocks += (T.lab_cap + kCopyPiece - 1) / kCopyPiece;
    }
  }
  a.num_types = num_types;
  a.want_typed = typed != nullptr;
  a.examples = examples;
  a.n = n;
  a.nnz_cap = nnz_cap;
  a.num_examples = first;
  a.queries = queries;
  a.query_type = query_type;
  a.label_coords = label_coords;
  a.triples = triples;
  a.weight = weight;
  a.counts = counts;
  a.ws = (long long*)ws;
  hipLaunchKernelGGL(kvsall_collate_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, a);
  if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
  if (blocks > 0) {
    hipLaunchKernelGGL(kvsall_collate_copy_kernel, dim3((unsigned)blocks), dim3(kCopyThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return KGE_ERR_LAUNCH;
  }
  return KGE_OK;
}

}  // namespace kge
