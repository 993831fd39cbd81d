// xhist_mode.hip.h — histogram_mode: per (row, bin) the number n of non-NaN values, the number of distinct ones, the most
// frequent value (the smallest among equally frequent ones) and how often it occurs.  It works in bin_rank's sorted domain
// (xhist_rank.hip.h): `order`, the sorted bin keys, `offsets`, the head and NaN bits of every word of 64 sorted positions and the
// three scalars before / last / next of every word.  There a tie run is [s, e) between two heads, a bin's distinct values are a
// difference of two head counts and its mode is its longest run, the first of the longest ones.
//
//   mode_runs    one wave per (row, word), no gather of values.  A lane whose position is a head, in a bin (key < B) and not NaN
//                holds pack = (e - s) << 32 | (0xFFFFFFFF - s): s its own position, e the next head of the word, else `next` of
//                the word.  Both halves fit 32 bits (n_cols < 2^31), a longer run is a larger pack, and of two runs of one
//                length the one that starts first is: one unsigned compare is "longest, then smallest value".  Every other
//                lane holds 0.  The keys do not decrease along a word, so an inclusive segmented maximum over equal keys (six
//                shuffle steps) leaves each bin's best run of the word in the last lane of the bin's segment; that lane alone
//                reads slot[row, key] and issues a 64-bit atomicMax only where it improves on what it read.  At most one atomic
//                per (word, bin), and the maximum of integers does not depend on the order of arrival.
//   mode_finish  one thread per (row, bin): the bin's first NaN position by rank_bins' bisection over the NaN bits, count and
//                nunique from it, mode_count and s from the slot, and mode = float64(values[order[s]]), the call's only gather of
//                values besides rank_heads'.  An empty bin gets 0, 0, the quiet NaN of np.nan and 0.  Every output element is
//                written exactly once.
//
// The slots are the out_mode_count block itself, uint64 [n_rows, B], zeroed by the driver for every batch of rows and finished in
// place: the thread of a (row, bin) reads its slot and then writes the bin's mode_count over it.  Plain launches order the steps.
//
// Nothing here instantiates a kernel: xhist_rank.hip does.
#pragma once

#include "xhist_rank.hip.h"

namespace xhist {

// one launch over rows [r0, r0 + r.n_rows) of the call: every pointer is pre-advanced to r0.  r.n_cols == 0: a call without
// columns, where mode_finish reads nothing of r but n_rows and nb.
struct ModeParams {
  RankParams r;            // the sorted domain (div and out unused)
  uint64_t* slots;         // [n_rows, nb]: the out_mode_count block
  int64_t* out_count;      // [n_rows, nb]
  int64_t* out_nunique;    // [n_rows, nb]
  double* out_mode;        // [n_rows, nb]
  int64_t* out_mode_count;  // [n_rows, nb]
};

__device__ __forceinline__ void mode_runs_body(const ModeParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {  // (uniform in a wave)
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    const bool in = i < p.n_cols;
    const uint64_t b = in ? p.keys[row * p.n_cols + i] : ~0ull;  // (past the row: a key no bin has, and none before it equals)
    const uint64_t hw = p.headw[u];
    const bool counted = in && b < (uint64_t)p.nb;
    uint64_t pack = 0;
    if (counted && ((hw >> lane) & 1) && !((p.nanw[u] >> lane) & 1)) {
      const uint64_t after = hw & ~rank_upto(lane);
      const int64_t e = after ? w * 64 + __ffsll((unsigned long long)after) - 1 : (int64_t)p.next[u];
      pack = (uint64_t)(e - i) << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t ob = __shfl_up((unsigned long long)b, d), op = __shfl_up((unsigned long long)pack, d);
      if (lane >= d && ob == b && op > pack) pack = op;
    }
    const uint64_t bn = __shfl_down((unsigned long long)b, 1);
    if (counted && pack && (lane == 63 || bn != b)) {
      uint64_t* const slot = m.slots + row * p.nb + (int64_t)b;
      if (pack > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)pack);
    }
  }
}

__device__ __forceinline__ void mode_finish_body(const ModeParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int64_t n = p.n_rows * p.nb;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t count = 0, nunique = 0, mode_count = 0;
    uint64_t bits = kRankNaN;
    if (p.n_cols > 0) {
      const int64_t row = j / p.nb, b = j % p.nb, at = row * p.words;
      const int64_t o = p.offsets[row * (p.nb + 1) + b], e = p.offsets[row * (p.nb + 1) + b + 1];
      int64_t lo = o, hi = e;  // no position below lo holds a NaN, every position of the bin from hi on does
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((p.nanw[at + (mid >> 6)] >> (mid & 63)) & 1) hi = mid;
        else lo = mid + 1;
      }
      const uint64_t slot = m.slots[j];
      const int64_t s = (int64_t)(0xFFFFFFFFu - (uint32_t)slot);
      if (lo > o && s < p.n_cols) {  // (a bin with a value has a run, so its slot is not 0 and s is the run's first position)
        count = lo - o;
        nunique = rank_heads_upto(p, at, lo - 1) - rank_heads_upto(p, at, o) + 1;
        mode_count = (int64_t)(slot >> 32);
        const int64_t voff = row_offset(p.v.row0 + row, p.v.rs, p.v.ir, p.v.os);
        bits = __builtin_bit_cast(uint64_t, load_as<double>(p.v.ptr, p.v.dt, voff + p.order[row * p.n_cols + s] * p.v.cs));
      }
    }
    m.out_count[j] = count;
    m.out_nunique[j] = nunique;
    reinterpret_cast<uint64_t*>(m.out_mode)[j] = bits;
    m.out_mode_count[j] = mode_count;  // (over the slot this thread alone read)
  }
}

// The kernels: mode_runs takes kRankWaves waves of 64 lanes, mode_finish 256 threads.
__global__ void __launch_bounds__(64 * kRankWaves) mode_runs(const ModeParams m) { mode_runs_body(m); }
__global__ void __launch_bounds__(256) mode_finish(const ModeParams m) { mode_finish_body(m); }

}  // namespace xhist
