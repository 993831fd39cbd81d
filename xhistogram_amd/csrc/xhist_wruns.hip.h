// xhist_wruns.hip.h — the float64 sum of a weight over every tie run of bin_rank's sorted domain (xhist_rank.hip.h), for
// bin_weighted_unique (a run's sum is stored at its entry of bin_unique's CSR form) and histogram_weighted_mode (at the run's first
// sorted position, and the bin's largest sum is then found with integer atomics).  A run [s, e) lies between two heads and is
// arbitrarily long, so its sum is a segmented reduction across the words of 64 positions and the tiles of kRankTile words:
//
//   wruns_words   one wave per (row, word): the call's only gather of weights, x_i = float64(weights[order[i]]), and an inclusive
//                 segmented sum over the lanes between head bits (six shuffle steps; lane l adds lane l - d where that lane is
//                 not before the last head at or before l).  A run that starts at a head of the word and ends in it (a later
//                 head in the word, or `next` of the word at most the word's end) is complete: its head lane fetches the sum at
//                 the run's last lane and plain-stores it.  Per word two float64: `lead`, the sum of the lanes before the first
//                 head (the whole word without one), and `tail`, the sum from the last head to lane 63.
//   wruns_totals, wruns_scan, wruns_close
//                 a segmented scan of the words' elements, (tail, 1) for a word with a head and (lead, 0) for one without, under
//                 (a, fa) + (b, fb) = fb ? (b, 1) : (a + b, fa): the value before word w is the sum of the run that enters w,
//                 tail[w0] + lead[w0 + 1] + ... + lead[w - 1].  It has rank_totals / rank_scan / rank_words' three levels: a
//                 thread folds kRankPer consecutive words from the left, the 256 threads of a tile scan in LDS by doubling,
//                 wruns_totals writes each tile's element, wruns_scan (one workgroup per row) scans the tiles in groups of 256
//                 by doubling with a carry from group to group, and wruns_close scans each tile's words again from what its
//                 tile takes over and, for a word that ends an incoming run (lane 0 is no head, and the word has a head or
//                 `next` of it is at most its end), stores carry + lead at the run's slot.
//   wruns_pad     bin_weighted_unique's padding: +0.0 at the entries [min(U, W), W) of every row.
//
// The order of additions is fixed by where a run lies against the words and tiles of its row and by nothing else: not the grid,
// not the rows of a launch, not the width.  The identity of the scans is -0.0 (-0.0 + x is x for every x, -0.0 included), so a
// position past the row's end and a thread without words change no bit.  No floating-point atomic, and no kernel waits for
// another workgroup.  The slot of a run whose head is at sorted position s, in bin b: with `uoff` (bin_unique's out_offsets) the
// entry uoff[b] + heads up to s - heads up to the bin's start, stored where it is below the width; without, s itself.  Nothing is
// stored for a key of B (not counted) and for a NaN value (every NaN is its own head, so no NaN lies inside an incoming run).
//
//   wmode_max     one wave per (row, word): a head lane that is counted and not NaN reads its run's sum and holds an
//                 order-preserving 64-bit key of it (-0.0 as +0.0; any NaN the largest key; every key is above 0), the others 0.
//                 An inclusive segmented maximum over equal bin keys, and the last lane of a bin's segment issues a 64-bit
//                 atomicMax on slot[row, bin] only where it improves on what it read first (mode_runs' scheme).
//   wmode_pos     the same walk: a head whose key equals the slot holds its position, the segment's minimum goes into the second
//                 slot with an atomicMin, read first.  Among equal sums the first entry wins, the smallest value.
//   wmode_finish  one thread per (row, bin): count and nunique as mode_finish computes them; mode the value at the winning
//                 position and mode_weight the bits of that run's sum; both 0x7ff8000000000000 where the key is NaN's; an empty
//                 bin 0, 0, NaN and +0.0.  The key slots are the out_mode_weight block (zeroed by the driver), the position
//                 slots the out_mode block (bytes of all ones), both finished in place by the thread that alone read them.
//
// Nothing here instantiates a kernel: xhist_rank.hip does.
#pragma once

#include "xhist_rank.hip.h"

namespace xhist {

// one launch over rows [r0, r0 + r.n_rows) of the call: every pointer is pre-advanced to r0 (for the weights, w.row0 is r0)
struct WrunsParams {
  RankParams r;         // the sorted domain (div and out unused)
  ValuesRead w;         // the weights
  const int64_t* uoff;  // [n_rows, nb + 1] bin_unique's out_offsets; nullptr: a run's slot is its first sorted position
  double* out;          // [n_rows, width]
  int64_t width;        // (without uoff: n_cols)
  double* lead;         // [n_rows, words]
  double* tail;         // [n_rows, words]
  double* tsum;         // [n_rows, tiles] a tile's element; after wruns_scan: the sum the tile takes over
  uint64_t* tflag;      // [n_rows, tiles]
  // histogram_weighted_mode alone
  uint64_t* kslot;      // [n_rows, nb] the out_mode_weight block
  uint64_t* pslot;      // [n_rows, nb] the out_mode block
  int64_t* out_count;   // [n_rows, nb]
  int64_t* out_nunique; // [n_rows, nb]
};

constexpr double kWrunsZero = -0.0;  // the identity of IEEE addition

// the slot of the run whose head is at sorted position s of bin b (b < nb), `heads` the heads at positions 0 .. s; -1: not stored
__device__ __forceinline__ int64_t wruns_slot(const WrunsParams& __restrict__ m, int64_t row, int64_t at, uint64_t b, int64_t s, int64_t heads) {
  if (!m.uoff) return s;
  const RankParams& p = m.r;
  const int64_t o = p.offsets[row * (p.nb + 1) + (int64_t)b];
  const int64_t e_at = m.uoff[row * (p.nb + 1) + (int64_t)b] + heads - rank_heads_upto(p, at, o);
  return e_at < m.width ? e_at : -1;
}

__device__ __forceinline__ void wruns_words_body(const WrunsParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {  // (uniform in a wave)
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    const bool in = i < p.n_cols;
    const int64_t r0 = row * p.n_cols, at = row * p.words;
    const uint64_t hw = p.headw[u];
    uint64_t b = ~0ull;
    double x = kWrunsZero;
    if (in) {
      b = p.keys[r0 + i];
      x = load_as<double>(m.w.ptr, m.w.dt, row_offset(m.w.row0 + row, m.w.rs, m.w.ir, m.w.os) + p.order[r0 + i] * m.w.cs);
    }
    const uint64_t upto = hw & rank_upto(lane);
    const int seg = upto ? 63 - __clzll((long long)upto) : 0;  // the first lane of this lane's segment
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double t = __shfl_up(x, d);
      if (lane - d >= seg) x = t + x;
    }
    // lead and tail of the word (hw is uniform in the wave, so the source lanes are)
    const int first = hw ? __ffsll((unsigned long long)hw) - 1 : 64;
    const double v_lead = __shfl(x, first == 64 ? 63 : first > 0 ? first - 1 : 0), v_tail = __shfl(x, 63);
    if (lane == 0) {
      m.lead[u] = (hw & 1) ? kWrunsZero : v_lead;
      m.tail[u] = v_tail;
    }
    // the runs that start at a head of this word and end in it
    const bool head = in && ((hw >> lane) & 1);
    const uint64_t after = hw & ~rank_upto(lane);
    int64_t e = 0;
    if (head) e = after ? w * 64 + __ffsll((unsigned long long)after) - 1 : (int64_t)p.next[u];
    const bool whole = head && e <= (w + 1) * 64;
    const double sum = __shfl(x, whole ? (int)(e - w * 64 - 1) : lane);
    if (whole && b < (uint64_t)p.nb && !((p.nanw[u] >> lane) & 1)) {
      const int64_t at_out = wruns_slot(m, row, at, b, i, (int64_t)p.before[u] + __popcll(upto));
      if (at_out >= 0) m.out[row * m.width + at_out] = sum;
    }
  }
}

// one element of the segmented scan over words or tiles
struct WrunsElem {
  double v;
  uint32_t f;
};

__device__ __forceinline__ WrunsElem wruns_join(const WrunsElem a, const WrunsElem b) {
  WrunsElem c;
  c.v = b.f ? b.v : a.v + b.v;
  c.f = a.f | b.f;
  return c;
}

// the elements of one thread of a (row, tile): kRankPer consecutive words, the identity past the row's last, and their fold
struct WrunsOwn {
  uint64_t hw[kRankPer];
  double lead[kRankPer], tail[kRankPer];
  WrunsElem all;
};

__device__ __forceinline__ WrunsOwn wruns_own(const WrunsParams& __restrict__ m, int64_t at, int64_t w0) {
  WrunsOwn o;
  o.all.v = kWrunsZero, o.all.f = 0;
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    const bool have = w0 + j < m.r.words;
    o.hw[j] = have ? m.r.headw[at + w0 + j] : 0;
    o.lead[j] = have ? m.lead[at + w0 + j] : kWrunsZero;
    o.tail[j] = have ? m.tail[at + w0 + j] : kWrunsZero;
  }
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    WrunsElem e;
    e.f = o.hw[j] != 0;
    e.v = e.f ? o.tail[j] : o.lead[j];
    o.all = wruns_join(o.all, e);
  }
  return o;
}

// Over the 256 threads of a workgroup, inclusive, by doubling: s_v / s_f of a thread become the join of the elements up to it.
__device__ __forceinline__ void wruns_scan_lds(double* s_v, uint32_t* s_f, const WrunsElem e) {
  const int tid = threadIdx.x;
  s_v[tid] = e.v;
  s_f[tid] = e.f;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    WrunsElem a;
    a.v = tid >= d ? s_v[tid - d] : kWrunsZero;
    a.f = tid >= d ? s_f[tid - d] : 0;
    WrunsElem c;
    c.v = s_v[tid], c.f = s_f[tid];
    __syncthreads();
    c = wruns_join(a, c);
    s_v[tid] = c.v;
    s_f[tid] = c.f;
    __syncthreads();
  }
}

__device__ __forceinline__ void wruns_totals_body(const WrunsParams& __restrict__ m) {
  __shared__ double s_v[256];
  __shared__ uint32_t s_f[256];
  const RankParams& p = m.r;
  const int64_t units = p.n_rows * p.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / p.tiles, tile = u % p.tiles;
    const WrunsOwn o = wruns_own(m, row * p.words, tile * kRankTile + (int64_t)threadIdx.x * kRankPer);
    wruns_scan_lds(s_v, s_f, o.all);
    if (threadIdx.x == 0) {
      m.tsum[u] = s_v[255];
      m.tflag[u] = s_f[255];
    }
    __syncthreads();  // (read before the next unit overwrites them)
  }
}

// One workgroup of 256 threads per row: tsum becomes the sum a tile takes over from the tiles before it, the sum so far of the
// run that is open where the tile starts (a tile that starts on a head reads it into no result).  Groups of 256 tiles, a carry
// from group to group.
__device__ __forceinline__ void wruns_scan_body(const WrunsParams& __restrict__ m) {
  __shared__ double s_v[256];
  __shared__ uint32_t s_f[256];
  const int tid = threadIdx.x;
  const int64_t tiles = m.r.tiles;
  double* const tsum = m.tsum + (int64_t)blockIdx.x * tiles;
  const uint64_t* const tflag = m.tflag + (int64_t)blockIdx.x * tiles;
  WrunsElem carry;
  carry.v = kWrunsZero, carry.f = 0;
  for (int64_t base = 0; base < tiles; base += 256) {  // (uniform in the workgroup)
    const int64_t t = base + tid;
    WrunsElem e;
    e.v = t < tiles ? tsum[t] : kWrunsZero;
    e.f = t < tiles ? (uint32_t)tflag[t] : 0;
    wruns_scan_lds(s_v, s_f, e);
    WrunsElem before;
    before.v = tid ? s_v[tid - 1] : kWrunsZero;
    before.f = tid ? s_f[tid - 1] : 0;
    WrunsElem last;
    last.v = s_v[255], last.f = s_f[255];
    if (t < tiles) tsum[t] = wruns_join(carry, before).v;
    carry = wruns_join(carry, last);
    __syncthreads();  // (read before the next group overwrites them)
  }
}

__device__ __forceinline__ void wruns_close_body(const WrunsParams& __restrict__ m) {
  __shared__ double s_v[256];
  __shared__ uint32_t s_f[256];
  const RankParams& p = m.r;
  const int tid = threadIdx.x;
  const int64_t units = p.n_rows * p.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / p.tiles, tile = u % p.tiles, at = row * p.words, r0 = row * p.n_cols;
    const int64_t w0 = tile * kRankTile + (int64_t)tid * kRankPer;
    const WrunsOwn o = wruns_own(m, at, w0);
    wruns_scan_lds(s_v, s_f, o.all);
    WrunsElem carry, before;
    carry.v = m.tsum[u], carry.f = 0;
    before.v = tid ? s_v[tid - 1] : kWrunsZero;
    before.f = tid ? s_f[tid - 1] : 0;
    double acc = wruns_join(carry, before).v;  // the sum of the run that enters word w0
#pragma unroll
    for (int j = 0; j < kRankPer; ++j) {
      const int64_t w = w0 + j;
      if (w < p.words) {
        const uint64_t hw = o.hw[j];
        if (w > 0 && !(hw & 1)) {  // a run enters this word; (position 0 is a head, so word 0 has none)
          const int64_t e = hw ? w * 64 + __ffsll((unsigned long long)hw) - 1 : (int64_t)p.next[at + w];
          if (e <= (w + 1) * 64) {  // and ends in it
            const int64_t s = (int64_t)p.last[at + w - 1];
            const uint64_t b = p.keys[r0 + s];
            if (b < (uint64_t)p.nb) {
              const int64_t at_out = wruns_slot(m, row, at, b, s, (int64_t)p.before[at + w]);
              if (at_out >= 0) m.out[row * m.width + at_out] = acc + o.lead[j];
            }
          }
        }
        acc = hw ? o.tail[j] : acc + o.lead[j];
      }
    }
    __syncthreads();  // (read before the next unit overwrites them)
  }
}

constexpr int kWrunsPadChunk = 256 * 8;  // entries of one unit of wruns_pad

__device__ __forceinline__ void wruns_pad_body(const WrunsParams& __restrict__ m) {
  const int64_t chunks = (m.width + kWrunsPadChunk - 1) / kWrunsPadChunk, units = m.r.n_rows * chunks, nb1 = m.r.nb + 1;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {  // (uniform in the workgroup)
    const int64_t row = u / chunks, c0 = (u % chunks) * kWrunsPadChunk;
    const int64_t c1 = c0 + kWrunsPadChunk < m.width ? c0 + kWrunsPadChunk : m.width;
    const int64_t have = m.uoff[row * nb1 + m.r.nb];
    for (int64_t j = (have > c0 ? have : c0) + threadIdx.x; j < c1; j += blockDim.x) m.out[row * m.width + j] = 0.0;
  }
}

// an order-preserving key of a run's sum: -0.0 as +0.0, any NaN the largest; never 0
__device__ __forceinline__ uint64_t wmode_key(double s) {
  if (s != s) return ~0ull;
  const uint64_t bits = __builtin_bit_cast(uint64_t, s + 0.0);
  return (bits >> 63) ? ~bits : bits | (1ull << 63);
}

// MAX: the key of every counted non-NaN head's sum, the maximum per bin into kslot.  Otherwise: the position of every such head
// whose key is the slot's, the minimum per bin into pslot.
template <bool MAX>
__device__ __forceinline__ void wmode_walk_body(const WrunsParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t units = p.n_rows * p.words;
  for (int64_t u = (int64_t)blockIdx.x * kRankWaves + wave; u < units; u += (int64_t)gridDim.x * kRankWaves) {  // (uniform in a wave)
    const int64_t row = u / p.words, w = u % p.words, i = w * 64 + lane;
    const bool in = i < p.n_cols;
    const uint64_t b = in ? p.keys[row * p.n_cols + i] : ~0ull;  // (past the row: a key no bin has)
    const uint64_t hw = p.headw[u];
    const bool counted = in && b < (uint64_t)p.nb;
    uint64_t pack = MAX ? 0 : ~0ull;
    if (counted && ((hw >> lane) & 1) && !((p.nanw[u] >> lane) & 1)) {
      const uint64_t key = wmode_key(m.out[row * p.n_cols + i]);
      if (MAX) pack = key;
      else if (key == m.kslot[row * p.nb + (int64_t)b]) pack = (uint64_t)i;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t ob = __shfl_up((unsigned long long)b, d), op = __shfl_up((unsigned long long)pack, d);
      if (lane >= d && ob == b && (MAX ? op > pack : op < pack)) pack = op;
    }
    const uint64_t bn = __shfl_down((unsigned long long)b, 1);
    if (counted && pack != (MAX ? 0 : ~0ull) && (lane == 63 || bn != b)) {
      uint64_t* const slot = (MAX ? m.kslot : m.pslot) + row * p.nb + (int64_t)b;
      const uint64_t seen = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (MAX) {
        if (pack > seen) atomicMax(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)pack);
      } else {
        if (pack < seen) atomicMin(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)pack);
      }
    }
  }
}

__device__ __forceinline__ void wmode_finish_body(const WrunsParams& __restrict__ m) {
  const RankParams& p = m.r;
  const int64_t n = p.n_rows * p.nb;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t count = 0, nunique = 0;
    uint64_t bits = kRankNaN, wbits = 0;
    if (p.n_cols > 0) {
      const int64_t row = j / p.nb, b = j % p.nb, at = row * p.words;
      const int64_t o = p.offsets[row * (p.nb + 1) + b], e = p.offsets[row * (p.nb + 1) + b + 1];
      int64_t lo = o, hi = e;  // no position below lo holds a NaN, every position of the bin from hi on does
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((p.nanw[at + (mid >> 6)] >> (mid & 63)) & 1) hi = mid;
        else lo = mid + 1;
      }
      const uint64_t key = m.kslot[j], s = m.pslot[j];
      if (lo > o && s < (uint64_t)p.n_cols) {  // (a bin with a value has a run, so both slots were set)
        count = lo - o;
        nunique = rank_heads_upto(p, at, lo - 1) - rank_heads_upto(p, at, o) + 1;
        if (key == ~0ull) {
          wbits = kRankNaN;
        } else {
          const int64_t voff = row_offset(p.v.row0 + row, p.v.rs, p.v.ir, p.v.os);
          bits = __builtin_bit_cast(uint64_t, load_as<double>(p.v.ptr, p.v.dt, voff + p.order[row * p.n_cols + (int64_t)s] * p.v.cs));
          wbits = reinterpret_cast<const uint64_t*>(m.out)[row * p.n_cols + (int64_t)s];
        }
      }
    }
    m.out_count[j] = count;
    m.out_nunique[j] = nunique;
    m.pslot[j] = bits;   // (out_mode, over the slot this thread alone read)
    m.kslot[j] = wbits;  // (out_mode_weight, likewise)
  }
}

// The kernels: wruns_words and the wmode walks take kRankWaves waves of 64 lanes, the others 256 threads.
__global__ void __launch_bounds__(64 * kRankWaves) wruns_words(const WrunsParams m) { wruns_words_body(m); }
__global__ void __launch_bounds__(256) wruns_totals(const WrunsParams m) { wruns_totals_body(m); }
__global__ void __launch_bounds__(256) wruns_scan(const WrunsParams m) { wruns_scan_body(m); }
__global__ void __launch_bounds__(256) wruns_close(const WrunsParams m) { wruns_close_body(m); }
__global__ void __launch_bounds__(256) wruns_pad(const WrunsParams m) { wruns_pad_body(m); }
__global__ void __launch_bounds__(64 * kRankWaves) wmode_max(const WrunsParams m) { wmode_walk_body<true>(m); }
__global__ void __launch_bounds__(64 * kRankWaves) wmode_pos(const WrunsParams m) { wmode_walk_body<false>(m); }
__global__ void __launch_bounds__(256) wmode_finish(const WrunsParams m) { wmode_finish_body(m); }

}  // namespace xhist
