// rescal_grouped_device.hpp -- the workspace and the tile geometry of the relation-grouped RESCAL kernels
// (rescal_grouped.hip; include/kge_amd.h "RESCAL, relation-grouped").
//
// Tile: 16 rows of ONE relation group (the M of v_mfma_f32_16x16x4_f32) x 64 output columns, a 16-column tile per wave.
// The 16-row instruction and not 32x32x2: at the FB15k-237 shape (237 relations for 512 rows) a group holds two rows
// on average -- a 32-row tile would multiply 30 rows of zeros -- and a 16-row tile keeps the accumulator at 4 VGPRs.
// LDS of the build: 16 entity rows on the pitch 260 (16.3 KiB) + one panel of 32 k-rows x 64 columns of M_p on the
// pitch 68 (8.5 KiB).  A whole M_p at d = 256 is 256 KiB: it never sits in LDS, a workgroup streams the 64 columns it
// owns in 8 panels.  Both pitches are 4 mod 32 words: the 16 x 4 lanes of an MFMA operand read 64 distinct banks.
#pragma once
#include "rescal_device.hpp"

namespace kge {

constexpr int RG_THREADS = 256;
constexpr int RG_TM = 16;               // rows of a tile
constexpr int RG_CB = 64;               // output columns of a workgroup
constexpr int RG_KP = 32;               // k-rows of a panel of M_p
constexpr int RG_LDX = RS_MAX_DIM + 4;  // a staged row
constexpr int RG_LDP = RG_CB + 4;       // a panel row
constexpr int RG_STAGE = 1024;          // keys staged per pass of the grouping kernels
constexpr int RG_NEG_CHUNK = 256;       // samples staged per pass of rsg_neg_kernel
constexpr long long RG_MAX_N = KGE_RESCAL_GROUPED_MAX_N;
static_assert(RG_NEG_CHUNK == RG_THREADS && RG_NEG_CHUNK % 8 == 0, "a sample per thread; whole lane sets per chunk");

// The sections of the workspace, each on a 16-byte boundary; the first four are the public result of kge_rescal_group.
struct RgWs {
  int* perm;         // [n]      batch positions in ascending relation id, ascending position inside a relation
  int* group_rel;    // [n]      the first G: the relation of group g
  int* group_begin;  // [n + 1]  the first G + 1: group g is perm[group_begin[g] .. group_begin[g + 1])
  int* counts;       // [4]      G, the number of row tiles T, 0, 0
  int* tile_begin;   // [n + 1]  the first G + 1: the first row tile of group g
  int* key;          // [n]      the relation of position i (a dense int32 copy of the index)
  int* less;         // [n]      keys below key[i]
  int* cnt;          // [n]      keys equal to key[i]
  int* eqb;          // [n]      equal keys in front of position i
  float* Q;          // [n, d]   the queries of the backward
  float* GQ;         // [n, d]   their gradients
};

__host__ inline long long rg_a16(long long bytes) { return (bytes + 15) & ~15LL; }

__host__ inline long long rg_workspace_bytes(long long n, int d) {
  return 6 * rg_a16(4 * n) + 2 * rg_a16(4 * (n + 1)) + 16 + 2 * rg_a16(4 * n * d);
}

__host__ inline RgWs rg_workspace(void* ws, long long n, int d) {
  char* p = (char*)ws;
  auto take = [&p](long long bytes) {
    char* r = p;
    p += rg_a16(bytes);
    return r;
  };
  RgWs w;
  w.perm = (int*)take(4 * n);
  w.group_rel = (int*)take(4 * n);
  w.group_begin = (int*)take(4 * (n + 1));
  w.counts = (int*)take(16);
  w.tile_begin = (int*)take(4 * (n + 1));
  w.key = (int*)take(4 * n);
  w.less = (int*)take(4 * n);
  w.cnt = (int*)take(4 * n);
  w.eqb = (int*)take(4 * n);
  w.Q = (float*)take(4 * n * d);
  w.GQ = (float*)take(4 * n * d);
  return w;
}

// the most row tiles a batch can have: a tile per group and one more per 16 rows
__host__ inline long long rg_max_tiles(long long n, long long num_rel) {
  const long long g = n < num_rel ? n : num_rel;
  const long long t = g + n / RG_TM;
  return t < n ? t : n;
}

// the group of row tile t < T: the last g with tile_begin[g] <= t
__device__ __forceinline__ int rg_tile_group(const int* __restrict__ tile_begin, int G, int t) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_begin[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

}  // namespace kge
