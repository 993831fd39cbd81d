// xhist_unique.hip.h — bin_unique: per row the distinct non-NaN values of every bin, ascending, with how often each occurs, in CSR
// form (uniques, counts, offsets), and for every sample the entry that holds its value (inverse).  It works in bin_rank's sorted
// domain (xhist_rank.hip.h): `order`, the sorted bin keys, the sort's `offsets`, the head and NaN bits of every word of 64 sorted
// positions and `before` of every word.  Inside a bin the non-NaN values precede the NaNs and a bin's first position is a head,
// so every head from the bin's start o_b up to a non-NaN position i is a distinct value, and the entry of the run that holds i is
//   u = uoff[b] + rank_heads_upto(i) - rank_heads_upto(o_b)
// with uoff the exclusive scan of the bins' distinct-value counts over the row: out_offsets itself, W the width of a row's
// uniques and counts.
//
//   unique_bins     one thread per (row, bin): the bin's first NaN position by rank_bins' bisection over the NaN bits, the
//                   distinct values as a difference of two head counts (histogram_mode's nunique), stored at
//                   out_offsets[row, b + 1]; the thread of bin 0 also stores the 0 of out_offsets[row, 0].
//   unique_scan     one workgroup per row: the inclusive scan of the row's B + 1 int64 in place, in tiles of kUniqueTile with a
//                   carry (a shuffle scan inside each wave, the waves' totals through LDS).
//   unique_runs     one wave per (row, word).  A lane whose position is a head, in a bin (key < B) and not NaN is the first
//                   sample of a distinct value: it computes u and, where u < W, gathers its one value (the call's only gather of
//                   values besides rank_heads') and stores uniques[row, u] and counts[row, u] = e - i, e the next head of the
//                   word, else `next` of the word.  Every entry below min(U, W) has exactly one such lane.
//   unique_pad      the entries [min(U, W), W) of every row, U = out_offsets[row, B]: the quiet NaN of np.nan and 0.  A workgroup
//                   per (row, chunk of kUniquePadChunk entries), and a chunk below U is skipped after one read.
//   unique_inverse  only with an inverse: one wave per (row, word), no gather of values: inverse[row, order[i]] = u of the run's
//                   head (the heads up to i are the heads up to it), -1 where the key is B or the NaN bit is set.  order is a
//                   permutation, so every element is written exactly once.
//
// Plain launches order the steps, no kernel waits for another workgroup and none issues an atomic.  Entries u >= W are stored
// nowhere; out_offsets and the inverse hold the true u all the same.
//
// Nothing here instantiates a kernel: xhist_rank.hip does.
#pragma once

#include "xhist_rank.hip.h"

namespace xhist {

constexpr int kUniquePer = 4;                      // consecutive offsets of one thread of a scan tile
constexpr int kUniqueTile = 256 * kUniquePer;      // offsets one workgroup of 256 threads scans at a time
constexpr int kUniquePadChunk = 256 * 8;           // entries of one unit of unique_pad

// one launch over rows [r0, r0 + r.n_rows) of the call: every pointer is pre-advanced to r0.  r.n_cols == 0: a call without
// columns, where unique_pad reads nothing of r but n_rows and nb.
struct UniqueParams {
  RankParams r;          // the sorted domain (div and out unused); r.offsets are the sort's, positions
  int64_t* out_offsets;  // [n_rows, nb + 1]
  double* out_uniques;   // [n_rows, width]
  int64_t* out_counts;   // [n_rows, width]
  int64_t* out_inverse;  // [n_rows, n_cols]; nullptr: none
  int64_t width;
};

__device__ __forceinline__ void unique_bins_body(const UniqueParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int64_t n = p.n_rows * p.nb;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = j / p.nb, b = j % p.nb, at = row * p.words;
    const int64_t o = p.offsets[row * (p.nb + 1) + b], e = p.offsets[row * (p.nb + 1) + b + 1];
    int64_t lo = o, hi = e;  // no position below lo holds a NaN, every position of the bin from hi on does
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((p.nanw[at + (mid >> 6)] >> (mid & 63)) & 1) hi = mid;
      else lo = mid + 1;
    }
    m.out_offsets[row * (p.nb + 1) + b + 1] = lo > o ? rank_heads_upto(p, at, lo - 1) - rank_heads_upto(p, at, o) + 1 : 0;
    if (b == 0) m.out_offsets[row * (p.nb + 1)] = 0;
  }
}

__device__ __forceinline__ void unique_scan_body(const UniqueParams& __restrict__ m) {
  __shared__ int64_t s_wave[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t nb1 = m.r.nb + 1;
  int64_t* const row = m.out_offsets + (int64_t)blockIdx.x * nb1;
  int64_t carry = 0;
  for (int64_t base = 0; base < nb1; base += kUniqueTile) {  // (uniform in the workgroup)
    const int64_t i0 = base + (int64_t)tid * kUniquePer;
    int64_t v[kUniquePer], sum = 0;
#pragma unroll
    for (int j = 0; j < kUniquePer; ++j) {
      sum += i0 + j < nb1 ? row[i0 + j] : 0;
      v[j] = sum;
    }
    int64_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t t = __shfl_up((long long)inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int64_t below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) below += s_wave[w];
      total += s_wave[w];
    }
    const int64_t excl = carry + below + inc - sum;
#pragma unroll
    for (int j = 0; j < kUniquePer; ++j)
      if (i0 + j < nb1) row[i0 + j] = excl + v[j];
    carry += total;
    __syncthreads();  // (read before the next tile overwrites them)
  }
}

__device__ __forceinline__ void unique_runs_body(const UniqueParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {  // (uniform in a wave)
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    if (i >= p.n_cols) continue;
    const int64_t r0 = row * p.n_cols, at = row * p.words;
    const uint64_t b = p.keys[r0 + i], hw = p.headw[u];
    if (b >= (uint64_t)p.nb || !((hw >> lane) & 1) || ((p.nanw[u] >> lane) & 1)) continue;
    const int64_t o = p.offsets[row * (p.nb + 1) + (int64_t)b];
    const int64_t e_at = m.out_offsets[row * (p.nb + 1) + (int64_t)b] + (int64_t)p.before[u] + __popcll(hw & rank_upto(lane)) -
                         rank_heads_upto(p, at, o);
    if (e_at >= m.width) continue;
    const uint64_t after = hw & ~rank_upto(lane);
    const int64_t e = after ? w * 64 + __ffsll((unsigned long long)after) - 1 : (int64_t)p.next[u];
    const int64_t voff = row_offset(p.v.row0 + row, p.v.rs, p.v.ir, p.v.os);
    const double v = load_as<double>(p.v.ptr, p.v.dt, voff + p.order[r0 + i] * p.v.cs);
    reinterpret_cast<uint64_t*>(m.out_uniques)[row * m.width + e_at] = __builtin_bit_cast(uint64_t, v);
    m.out_counts[row * m.width + e_at] = e - i;
  }
}

__device__ __forceinline__ void unique_pad_body(const UniqueParams& __restrict__ m) {
  const int64_t chunks = (m.width + kUniquePadChunk - 1) / kUniquePadChunk, units = m.r.n_rows * chunks, nb1 = m.r.nb + 1;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {  // (uniform in the workgroup)
    const int64_t row = u / chunks, c0 = (u % chunks) * kUniquePadChunk;
    const int64_t c1 = c0 + kUniquePadChunk < m.width ? c0 + kUniquePadChunk : m.width;
    const int64_t have = m.out_offsets[row * nb1 + m.r.nb];
    for (int64_t j = (have > c0 ? have : c0) + threadIdx.x; j < c1; j += blockDim.x) {
      reinterpret_cast<uint64_t*>(m.out_uniques)[row * m.width + j] = kRankNaN;
      m.out_counts[row * m.width + j] = 0;
    }
  }
}

__device__ __forceinline__ void unique_inverse_body(const UniqueParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    if (i >= p.n_cols) continue;
    const int64_t r0 = row * p.n_cols, at = row * p.words;
    const int64_t pos = p.order[r0 + i];
    const uint64_t b = p.keys[r0 + i], hw = p.headw[u];
    int64_t e_at = -1;
    if (b < (uint64_t)p.nb && !((p.nanw[u] >> lane) & 1)) {
      const int64_t o = p.offsets[row * (p.nb + 1) + (int64_t)b];
      e_at = m.out_offsets[row * (p.nb + 1) + (int64_t)b] + (int64_t)p.before[u] + __popcll(hw & rank_upto(lane)) -
             rank_heads_upto(p, at, o);
    }
    m.out_inverse[r0 + pos] = e_at;
  }
}

// The kernels: unique_runs / unique_inverse take kRankWaves waves of 64 lanes, the others 256 threads.
__global__ void __launch_bounds__(256) unique_bins(const UniqueParams m) { unique_bins_body(m); }
__global__ void __launch_bounds__(256) unique_scan(const UniqueParams m) { unique_scan_body(m); }
__global__ void __launch_bounds__(64 * kRankWaves) unique_runs(const UniqueParams m) { unique_runs_body(m); }
__global__ void __launch_bounds__(256) unique_pad(const UniqueParams m) { unique_pad_body(m); }
__global__ void __launch_bounds__(64 * kRankWaves) unique_inverse(const UniqueParams m) { unique_inverse_body(m); }

}  // namespace xhist
