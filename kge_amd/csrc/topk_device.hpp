// topk_device.hpp -- what the two kernel pairs of kge_topk share (topk.hip: k <= 128, one lane per row inserts into an
// LDS list; topk_wide.hip: k <= 1024, a wave merges a row's pending keys into a list in the workspace): the launch
// arguments, the 64-bit key and the host-side geometry.
#pragma once
#include "common.hpp"
#include "pairs_device.hpp"
#include "switches.hpp"

namespace kge {

struct TopkArgs {
  int nfilt;                     // <= 2
  const unsigned int* bits[2];   // the filter bits of RankArgs (common.hpp): bit (j & 31) of word [i * rs + (j >> 5) * us]
  long long bits_rs, bits_us;
  int col_tiles;                 // column tiles a workgroup walks
  int k;                         // <= KGE_TOPK_MAX
  unsigned long long* part;      // narrow: [n][groups][k] keys; wide: [n][groups][2][k] (ping-pong halves); groups = gridDim.x
};

// Key: high word = the order-preserving unsigned image of the canonical score (NaN -> -inf, -0.0 -> +0.0),
// low word = 0xFFFFFFFF - j (j = the column inside the scored slice).  A larger key is better; equal scores order by
// ascending entity id; every real column has a non-zero key (j <= 2^32 - 2) and 0 means "empty".
__device__ __forceinline__ unsigned long long topk_key(float s, unsigned int j) {
  if (s != s) s = -__builtin_inff();  // count_one's NaN rule (common.hpp)
  if (s == 0.0f) s = 0.0f;            // -0.0 -> +0.0
  const unsigned int u = __float_as_uint(s);
  const unsigned int hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)hi << 32) | (unsigned long long)(0xFFFFFFFFu - j);
}

// (value, id) of a key; 0 ("empty") -> (-inf, -1)
__device__ __forceinline__ void topk_unpack(unsigned long long key, long long col_begin, float& v, long long& id) {
  v = -__builtin_inff();
  id = -1;
  if (key != 0ull) {
    const unsigned int hi = (unsigned int)(key >> 32);
    v = __uint_as_float((hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi);
    id = col_begin + (long long)(0xFFFFFFFFu - (unsigned int)key);
  }
}

constexpr int TOPK_MAX_GROUPS = 512;  // column groups of a launch (topk_merge_kernel's head table)
constexpr int TOPK_NARROW_MAX = 128;  // largest k of topk_select_kernel: its lists are [k][64] keys of LDS, 64 KB here
// Smallest k the wide pair takes by itself (SW_TOPK_WIDE unset): the smallest probed k at which it beat the narrow pair
// at 14,541 and at 1,000,000 entities by more than the windows' spread (profiles/topk_wide_probe.txt).
constexpr int TOPK_WIDE_K0 = 64;

static inline bool topk_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// (the conditions of score_pairs.hip's vector loads)
static inline bool topk_vec_ok(int dtype, int d, int dr, int scorer, const Operand& A, const Operand& R,
                               const Operand& TG) {
  if (d % 8) return false;
  if (scorer == KGE_ROTATE && dr != d / 2) return false;
  const int es = dtype == KGE_BF16 ? 2 : 4;
  const int al = dtype == KGE_BF16 ? 8 : 16;
  if (!topk_aligned16(A.base) || !topk_aligned16(R.base) || !topk_aligned16(TG.base)) return false;
  if ((A.ld * es) % al || (R.ld * es) % al || (TG.ld * es) % al) return false;
  return true;
}

// topk.hip
long long topk_groups(long long n, long long m, int* col_tiles);
bool topk_takes_wide(int k);
long long topk_part_bytes(long long n, long long m, int k);
// topk_wide.hip
long long topk_wide_groups(long long n, long long m, int k, int* col_tiles);
long long topk_wide_part_bytes(long long n, long long m, int k);
int run_topk_wide(int scorer, int dtype, bool use_mfma, const Operand& A, const Operand& R, const Operand& TG, int dir,
                  int d, int dr, long long n, long long m, float lp, int k, int nfilt, const unsigned int* const* bits,
                  long long bits_rs, long long bits_us, unsigned long long* part, long long col_begin, float* out_val,
                  long long* out_idx, long long ld, hipStream_t st);

}  // namespace kge
