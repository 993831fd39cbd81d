// xhist_rank.hip.h — bin_rank: the rank of every sample's value among the non-NaN values of its bin.  Everything here works on
// what bin_sort leaves, per row of n_cols positions: `order` (int64, by bin, then by value, NaN last in its bin), the sorted bin
// keys beside it (uint64 in [0, B], B: not counted) and `offsets` (int64 [B + 1]).  With i an index into order, p_i = order[i],
// b_i the sorted key and v_i = float64(values[p_i]), position i is a *head* when it starts a tie run:
//   head_i = (i == 0) || b_i != b_{i-1} || !(v_i == v_{i-1})
// so equal values on the two sides of a bin border do not tie, -0.0 and +0.0 do, and every NaN is its own head.  The tie run of i
// is [s, e): s the last head at or before i, e the first head after it (n_cols: none).  A row is cut into *words* of 64
// positions, one wave64 step each; `words` = ceil(n_cols / 64).
//
//   rank_heads   one wave per (row, word): gathers v_i (the only gather of values of the call), compares each lane with its
//                predecessor (a shuffle; lane 0 reads position i - 1 itself) and writes the word's 64 head bits and 64 NaN bits
//                from two ballots.  Bits past n_cols are 0.
//   rank_totals, rank_scan, rank_words
//                three uint32 per word: `before` (heads in the words before it), `last` (the last head at or before the word's
//                end) and `next` (the first head after the word's end, n_cols: none).  A row's words go in tiles of kRankTile,
//                as the sort's chunks go in slices: rank_totals writes each tile's heads, last head and first head, rank_scan
//                (one workgroup per row) turns them into what a tile takes over from the tiles before and after it, and
//                rank_words scans each tile's words from there.  The words are 1/64 of the samples, the tiles 1/65536; the
//                launches order the steps and no workgroup waits for another.
//   rank_bins    only for pct: one thread per (row, bin) finds the bin's first NaN position by bisection over the NaN bits (NaN
//                is last in its bin) and writes the divisor as float64: the number n of non-NaN values, for dense the number
//                D of heads among them; NaN where n == 0 (no sample reads it).
//   rank_apply   one wave per (row, word), no gather of values: s and e from the word's head bits, else from `last` of the
//                word before and `next` of this one; o = offsets[b_i]; the rank of the method, divided once by the bin's
//                divisor for pct, stored at out[row, p_i].  NaN where b_i == B or the NaN bit is set.  order is a permutation,
//                so every element of out is written exactly once.
//
// Nothing here instantiates a kernel: xhist_rank.hip does.
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

constexpr int kRankWaves = 4;                        // waves of a workgroup of rank_heads / rank_apply: one word each at a time
constexpr int kRankPer = 4;                          // consecutive words of one thread of a tile
constexpr int kRankTile = 256 * kRankPer;            // words of one tile: what one workgroup of 256 threads scans at a time
constexpr uint64_t kRankNaN = 0x7ff8000000000000ull;  // the quiet NaN of np.nan

// one launch over rows [r0, r0 + n_rows) of the call: every pointer is pre-advanced to r0 (for the values, v.row0 is r0)
struct RankParams {
  ValuesRead v;  // the values, as sort_keys reads them
  int32_t method;
  const int64_t* order;    // [n_rows, n_cols]
  const uint64_t* keys;    // [n_rows, n_cols] the sorted bin keys
  const int64_t* offsets;  // [n_rows, nb + 1]
  uint64_t* headw;         // [n_rows, words]
  uint64_t* nanw;          // [n_rows, words]
  uint32_t* before;        // [n_rows, words]
  uint32_t* last;          // [n_rows, words]
  uint32_t* next;          // [n_rows, words]
  uint32_t* part;          // [3, n_rows, tiles] per tile: heads, last head, first head; after rank_scan: what the tile takes over
  double* div;             // [n_rows, nb]; nullptr: no pct
  double* out;             // [n_rows, n_cols]
  int64_t n_rows, n_cols, words, tiles, nb;
};

// bits 0 .. lane of a word
__device__ __forceinline__ uint64_t rank_upto(int lane) { return (2ull << lane) - 1; }

// heads at positions 0 .. j of a row whose words start at `at`
__device__ __forceinline__ int64_t rank_heads_upto(const RankParams& __restrict__ p, int64_t at, int64_t j) {
  return (int64_t)p.before[at + (j >> 6)] + __popcll(p.headw[at + (j >> 6)] & rank_upto((int)(j & 63)));
}

__device__ __forceinline__ void rank_heads_body(const RankParams& __restrict__ p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {  // (uniform in a wave)
    const int64_t row = u / p.words, i = (u % p.words) * 64 + lane;
    const bool in = i < p.n_cols;
    const int64_t r0 = row * p.n_cols, voff = row_offset(p.v.row0 + row, p.v.rs, p.v.ir, p.v.os);
    uint64_t b = 0;
    double v = 0.0;
    if (in) {
      b = p.keys[r0 + i];
      v = load_as<double>(p.v.ptr, p.v.dt, voff + p.order[r0 + i] * p.v.cs);
    }
    uint64_t bp = __shfl_up((unsigned long long)b, 1);
    double vp = __shfl_up(v, 1);
    if (lane == 0 && i > 0) {  // (i <= n_cols - 1 here: a word has at least one position)
      bp = p.keys[r0 + i - 1];
      vp = load_as<double>(p.v.ptr, p.v.dt, voff + p.order[r0 + i - 1] * p.v.cs);
    }
    const bool head = in && (i == 0 || b != bp || !(v == vp));
    const uint64_t hw = __ballot(head), nw = __ballot(in && v != v);
    if (lane == 0) {
      p.headw[u] = hw;
      p.nanw[u] = nw;
    }
  }
}

// the head words of one thread of a (row, tile): kRankPer consecutive words, 0 past the row's last
struct RankOwn {
  uint64_t w[kRankPer];
  uint32_t sum, mx, mn;  // their heads, the last of them (0: none) and the first (~0u: none)
};

__device__ __forceinline__ uint32_t rank_last_bit(int64_t word, uint64_t bits) { return (uint32_t)(word * 64 + 63 - __clzll((long long)bits)); }
__device__ __forceinline__ uint32_t rank_first_bit(int64_t word, uint64_t bits) { return (uint32_t)(word * 64 + __ffsll((unsigned long long)bits) - 1); }

__device__ __forceinline__ RankOwn rank_own(const uint64_t* __restrict__ hw, int64_t w0, int64_t words) {
  RankOwn o;
  o.sum = 0, o.mx = 0, o.mn = ~0u;
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) o.w[j] = w0 + j < words ? hw[w0 + j] : 0;
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    o.sum += (uint32_t)__popcll(o.w[j]);
    if (o.w[j]) o.mx = rank_last_bit(w0 + j, o.w[j]);
  }
#pragma unroll
  for (int j = kRankPer - 1; j >= 0; --j)
    if (o.w[j]) o.mn = rank_first_bit(w0 + j, o.w[j]);
  return o;
}

// Over the 256 threads of a workgroup, inclusive: s_sum and s_max over the threads up to this one, s_min over those from it on.
__device__ __forceinline__ void rank_scan_lds(uint32_t* s_sum, uint32_t* s_max, uint32_t* s_min, uint32_t sum, uint32_t mx, uint32_t mn) {
  const int tid = threadIdx.x;
  s_sum[tid] = sum;
  s_max[tid] = mx;
  s_min[tid] = mn;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t a = tid >= d ? s_sum[tid - d] : 0, m = tid >= d ? s_max[tid - d] : 0, n = tid + d < 256 ? s_min[tid + d] : ~0u;
    __syncthreads();
    s_sum[tid] += a;
    s_max[tid] = s_max[tid] > m ? s_max[tid] : m;
    s_min[tid] = s_min[tid] < n ? s_min[tid] : n;
    __syncthreads();
  }
}

// part[row][tile] = (the heads of the tile, its last head, its first head); the workgroups walk the (row, tile) units grid-strided
__device__ __forceinline__ void rank_totals_body(const RankParams& __restrict__ p) {
  __shared__ uint32_t s_sum[256], s_max[256], s_min[256];
  const int64_t units = p.n_rows * p.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / p.tiles, tile = u % p.tiles;
    const RankOwn o = rank_own(p.headw + row * p.words, tile * kRankTile + (int64_t)threadIdx.x * kRankPer, p.words);
    rank_scan_lds(s_sum, s_max, s_min, o.sum, o.mx, o.mn);
    if (threadIdx.x == 0) {
      p.part[u] = s_sum[255];
      p.part[p.n_rows * p.tiles + u] = s_max[255];
      p.part[2 * p.n_rows * p.tiles + u] = s_min[0];
    }
    __syncthreads();  // (read before the next unit overwrites them)
  }
}

// One workgroup of 256 threads per row, a thread per run of ceil(tiles / 256) consecutive tiles: part becomes what a tile takes
// over from the others, the heads of the tiles before it, the last head in them (0: position 0 is one) and the first head in the
// tiles after it (n_cols: none).
__device__ __forceinline__ void rank_scan_body(const RankParams& __restrict__ p) {
  __shared__ uint32_t s_sum[256], s_max[256], s_min[256];
  const int tid = threadIdx.x;
  const int64_t per = (p.tiles + 255) / 256, t0 = tid * per, t1 = t0 + per < p.tiles ? t0 + per : p.tiles;
  const int64_t plane = p.n_rows * p.tiles;
  uint32_t* part = p.part + (int64_t)blockIdx.x * p.tiles;
  uint32_t sum = 0, mx = 0, mn = ~0u;
  for (int64_t t = t0; t < t1; ++t) {
    sum += part[t];
    mx = mx > part[plane + t] ? mx : part[plane + t];
    mn = mn < part[2 * plane + t] ? mn : part[2 * plane + t];
  }
  rank_scan_lds(s_sum, s_max, s_min, sum, mx, mn);
  uint32_t run_sum = s_sum[tid] - sum, run_max = tid ? s_max[tid - 1] : 0, run_min = tid < 255 ? s_min[tid + 1] : ~0u;
  if (run_min > (uint32_t)p.n_cols) run_min = (uint32_t)p.n_cols;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t a = part[t], m = part[plane + t];
    part[t] = run_sum;
    part[plane + t] = run_max;
    run_sum += a;
    run_max = run_max > m ? run_max : m;
  }
  for (int64_t t = t1 - 1; t >= t0; --t) {
    const uint32_t n = part[2 * plane + t];
    part[2 * plane + t] = run_min;
    run_min = run_min < n ? run_min : n;
  }
}

// One workgroup per (row, tile), grid-strided: the three scalars of every word of the tile, from the scan over the tile's threads
// and what rank_scan left in part.
__device__ __forceinline__ void rank_words_body(const RankParams& __restrict__ p) {
  __shared__ uint32_t s_sum[256], s_max[256], s_min[256];
  const int tid = threadIdx.x;
  const int64_t units = p.n_rows * p.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / p.tiles, tile = u % p.tiles, at = row * p.words, w0 = tile * kRankTile + (int64_t)tid * kRankPer;
    const RankOwn o = rank_own(p.headw + at, w0, p.words);
    rank_scan_lds(s_sum, s_max, s_min, o.sum, o.mx, o.mn);
    const uint32_t carry_max = p.part[units + u], carry_min = p.part[2 * units + u];
    uint32_t run_sum = p.part[u] + s_sum[tid] - o.sum;
    uint32_t run_max = tid ? s_max[tid - 1] : 0;
    uint32_t run_min = tid < 255 ? s_min[tid + 1] : ~0u;
    run_max = run_max > carry_max ? run_max : carry_max;
    run_min = run_min < carry_min ? run_min : carry_min;
#pragma unroll
    for (int j = 0; j < kRankPer; ++j)
      if (w0 + j < p.words) {
        p.before[at + w0 + j] = run_sum;
        if (o.w[j]) run_max = rank_last_bit(w0 + j, o.w[j]);
        p.last[at + w0 + j] = run_max;
        run_sum += (uint32_t)__popcll(o.w[j]);
      }
#pragma unroll
    for (int j = kRankPer - 1; j >= 0; --j)
      if (w0 + j < p.words) {
        p.next[at + w0 + j] = run_min;
        if (o.w[j]) run_min = rank_first_bit(w0 + j, o.w[j]);
      }
    __syncthreads();  // (read before the next unit overwrites them)
  }
}

__device__ __forceinline__ void rank_bins_body(const RankParams& __restrict__ p) {
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
    uint64_t bits = kRankNaN;
    if (lo > o) {
      const int64_t count = p.method == XHIST_RANK_DENSE ? rank_heads_upto(p, at, lo - 1) - rank_heads_upto(p, at, o) + 1 : lo - o;
      bits = __builtin_bit_cast(uint64_t, (double)count);
    }
    reinterpret_cast<uint64_t*>(p.div)[j] = bits;
  }
}

__device__ __forceinline__ void rank_apply_body(const RankParams& __restrict__ p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    if (i >= p.n_cols) continue;
    const int64_t r0 = row * p.n_cols, at = row * p.words;
    const int64_t pos = p.order[r0 + i];
    const uint64_t b = p.keys[r0 + i], hw = p.headw[u];
    uint64_t bits = kRankNaN;
    if (b < (uint64_t)p.nb && !((p.nanw[u] >> lane) & 1)) {
      const int64_t o = p.offsets[row * (p.nb + 1) + (int64_t)b];
      const uint64_t upto = hw & rank_upto(lane), after = hw & ~rank_upto(lane);
      // (a word without a head up to this lane is not the row's first: position 0 is a head)
      const int64_t s = upto ? w * 64 + 63 - __clzll((long long)upto) : (int64_t)p.last[u - 1];
      const int64_t e = after ? w * 64 + __ffsll((unsigned long long)after) - 1 : (int64_t)p.next[u];
      double r;
      switch (p.method) {
        case XHIST_RANK_MIN: r = (double)(s - o + 1); break;
        case XHIST_RANK_MAX: r = (double)(e - o); break;
        case XHIST_RANK_DENSE: r = (double)((int64_t)p.before[u] + __popcll(upto) - rank_heads_upto(p, at, o) + 1); break;
        case XHIST_RANK_ORDINAL: r = (double)(i - o + 1); break;
        default: r = (double)(s + e - 2 * o + 1) / 2.0; break;  // XHIST_RANK_AVERAGE (the driver admits no other code)
      }
      if (p.div) r /= p.div[row * p.nb + (int64_t)b];
      bits = __builtin_bit_cast(uint64_t, r);
    }
    reinterpret_cast<uint64_t*>(p.out)[r0 + pos] = bits;
  }
}

// The kernels: rank_heads / rank_apply take kRankWaves waves of 64 lanes, the others 256 threads.
__global__ void __launch_bounds__(64 * kRankWaves) rank_heads(const RankParams p) { rank_heads_body(p); }
__global__ void __launch_bounds__(256) rank_totals(const RankParams p) { rank_totals_body(p); }
__global__ void __launch_bounds__(256) rank_scan(const RankParams p) { rank_scan_body(p); }
__global__ void __launch_bounds__(256) rank_words(const RankParams p) { rank_words_body(p); }
__global__ void __launch_bounds__(256) rank_bins(const RankParams p) { rank_bins_body(p); }
__global__ void __launch_bounds__(64 * kRankWaves) rank_apply(const RankParams p) { rank_apply_body(p); }

}  // namespace xhist
