// neg_sample.hip -- the negative samples of one slot, drawn, filtered and redrawn on the device: what
// KgeSampler.sample does on the host per slot and step (kge/util/sampler.py:80-137: _sample, then
// _filter_and_resample* :163-196, 700-752, a per-row loop over a dict of positives) followed by the copy of the [n, K]
// int64 block to the GPU (train_negative_sampling.py:86-101).
//
// out[i, k] = the draw of the FIRST attempt t = 0, 1, 2, ... that is not a known answer of row i's key
// a[i] * mult + b[i] (rejection sampling: the accepted draw is distributed as the proposal -- uniform, or the alias
// table's frequencies -- conditioned on "not a positive", which is what the reference's resample loop produces).
//
// Random numbers: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), counter based, no state, no library:
//   key     = (seed low 32, seed high 32)
//   counter = (k, i, t, (uint32)call * 4 + slot)         one block r0..r3 per (row, column, attempt)
//   uniform   id = umul64hi((r0 << 32) | r1, vocab)
//   frequency bucket = umul64hi((r0 << 32) | r1, vocab), u = (r2 >> 8) * 2^-24,
//             id = u < alias_prob[bucket] ? bucket : alias_idx[bucket]      (torch._multinomial_alias_draw's arithmetic)
// A draw is a pure function of (seed, call, slot, i, k, t): no dependence on the launch geometry or on other lanes.
//
// One WAVE per row, lanes across columns.  The row's range [begin, end) in `values` comes from the 64-ary search of
// kge_filter_lookup (filter_key_pos, common.hpp), once per row; membership of a draw is a binary search in that sorted
// range, per lane; the redraw loop diverges per lane.  A lane gives up after KGE_NEG_SAMPLE_MAX_ATTEMPTS attempts and
// keeps its last draw (the reference loops forever on a key whose answers cover the vocabulary).  stats: per row the
// number of rejected attempts and the number of columns that hit the cap, wave-reduced, one plain store each.
#include "philox.hpp"

namespace kge {

template <bool ALIAS, bool FILTER>
__global__ __launch_bounds__(256) void neg_sample_kernel(long long n, long long K, unsigned long long vocab, unsigned k0,
                                                         unsigned k1, unsigned c3, const float* __restrict__ alias_prob,
                                                         const long long* __restrict__ alias_idx,
                                                         const long long* __restrict__ keys, long long num_keys,
                                                         const long long* __restrict__ starts,
                                                         const long long* __restrict__ values, Index a, Index b,
                                                         long long mult, long long* __restrict__ out, long long ld,
                                                         int* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (a whole wave)
  long long begin = 0, end = 0;
  if (FILTER && num_keys > 0) {
    const long long key = index_at(a, i) * mult + index_at(b, i);
    const long long pos = filter_key_pos(keys, num_keys, key, lane);
    if (pos < num_keys && keys[pos] == key) {
      begin = starts[pos];
      end = starts[pos + 1];
    }
  }
  int rejected = 0, capped = 0;
  for (long long k = lane; k < K; k += 64) {
    long long id = 0;
    int t = 0;
    for (;;) {
      const Philox4 r = philox4x32_10((unsigned)k, (unsigned)i, (unsigned)t, c3, k0, k1);
      id = (long long)__umul64hi(((unsigned long long)r.r0 << 32) | r.r1, vocab);
      if (ALIAS) {
        const float u = (float)(r.r2 >> 8) * 0x1p-24f;
        if (!(u < alias_prob[id])) id = alias_idx[id];
      }
      if (!FILTER) break;
      long long lo = begin, hi = end;  // the first position in [begin, end) with values[pos] >= id
      while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (values[mid] < id) lo = mid + 1;
        else hi = mid;
      }
      if (!(lo < end && values[lo] == id)) break;
      ++rejected;
      if (++t == KGE_NEG_SAMPLE_MAX_ATTEMPTS) {
        ++capped;
        break;
      }
    }
    out[i * ld + k] = id;
  }
  if (stats) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      rejected += __shfl_xor(rejected, o, 64);
      capped += __shfl_xor(capped, o, 64);
    }
    if (lane == 0) {
      stats[i * 2] = rejected;
      stats[i * 2 + 1] = capped;
    }
  }
}

int run_neg_sample(long long n, long long K, long long vocab, int slot, unsigned long long seed, unsigned long long call,
                   const float* alias_prob, const long long* alias_idx, const long long* keys, long long num_keys,
                   const long long* starts, const long long* values, const Index& a, const Index& b, long long mult,
                   long long* out, long long ld, int* stats, hipStream_t st) {
  if (n == 0 || K == 0) return KGE_OK;
  const dim3 grid((unsigned)((n + 3) / 4)), block(256);
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), c3 = (unsigned)call * 4u + (unsigned)slot;
#define KGE_NEG_SAMPLE_LAUNCH(ALIAS, FILTER)                                                                          \
  hipLaunchKernelGGL((neg_sample_kernel<ALIAS, FILTER>), grid, block, 0, st, n, K, (unsigned long long)vocab, k0, k1, \
                     c3, alias_prob, alias_idx, keys, num_keys, starts, values, a, b, mult, out, ld, stats)
  if (alias_prob) {
    if (keys) KGE_NEG_SAMPLE_LAUNCH(true, true);
    else KGE_NEG_SAMPLE_LAUNCH(true, false);
  } else {
    if (keys) KGE_NEG_SAMPLE_LAUNCH(false, true);
    else KGE_NEG_SAMPLE_LAUNCH(false, false);
  }
#undef KGE_NEG_SAMPLE_LAUNCH
  return hipGetLastError() == hipSuccess ? KGE_OK : KGE_ERR_LAUNCH;
}

}  // namespace kge
