// xhist_group.hip.h — bin_order: the stable group-by of a row's samples by bin, a counting sort of keys that are bin numbers.
// Per row of n_cols positions with keys in [0, B) or -1 (bin_index's block; -1 sorts as key B) it writes
//   order    int64 [n_cols]  the positions sorted by key, positions of equal keys ascending (np.argsort(key, kind="stable"))
//   offsets  int64 [B + 1]   offsets[b] = #{p : key[p] < b}: bin b is order[offsets[b] : offsets[b + 1]], the dropped samples
//                            are order[offsets[B] :]
// in three steps over the key block:
//   group_count<W>    a row is cut into `chunks` contiguous chunks of `chunk` positions (a multiple of 64).  One wave64 owns
//                     one (row, chunk): it counts the chunk's keys into its own B + 1 uint32 counters in LDS (the last one is
//                     key -1) and writes them to cnt[row][chunk][B + 1].  Counts do not depend on the order of the additions,
//                     so plain LDS adds without a return value do.
//   group_scan        offsets[b] = the exclusive prefix over bins of the totals over chunks, and cnt[row][chunk][key] becomes
//                     offsets[key] + the counts of the earlier chunks: where the (chunk, key) run starts in the row's order.
//                     Everything of a row is below 2^31, so uint32 holds it.  A row cut into thousands of chunks is too much
//                     for the one workgroup that scans a row's bins, so the chunks go in slices of 64:
//                       group_totals  a workgroup per (row, tile of bins, slice), a thread per bin: part[row][slice][bin] = the
//                                     slice's total
//                       group_scan    one workgroup per row, the bins in tiles of the block with the running sum carried from
//                                     tile to tile: offsets, and part becomes the base of each (slice, bin)
//                       group_bases   as group_totals: from its slice's base, a thread rewrites the slice's 64 counters of its bin
//                     A row of one chunk is its own slice: group_scan runs on cnt itself and the other two are not launched.
//   group_scatter<W>  the same (row, chunk) -> wave assignment.  The wave loads its bases into its LDS counters and walks its
//                     chunk 64 consecutive positions at a step.  In a step the lanes that hold the same key find each other by
//                     one __ballot per bit of the key; a lane's rank is the number of its peers below it; every lane reads its
//                     key's counter, and then the lowest lane of each group adds the group's size to it.  Distinct groups hold
//                     distinct keys, so no two lanes write one counter, and no atomic is involved: the place of a position is
//                     base + rank, a function of the keys alone.
// One wave owns one chunk, so the loop has no workgroup barrier, and a wave's LDS operations complete in the order they were
// issued: a fence at wavefront scope (group_wave_sync) is all that separates the counter reads of a step from its writes.
//
// Nothing here instantiates a kernel: xhist_group.hip does.
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

constexpr int kGroupStep = 64;   // positions of one step of a wave; chunks are whole steps
constexpr int kGroupUnroll = 4;  // key loads a lane keeps in flight
constexpr int kGroupSlice = 64;  // chunks of one slice of the scan

// one launch over rows [r0, r0 + n_rows) of the call: every pointer is pre-advanced to r0
struct GroupParams {
  const int64_t* keys;  // [n_rows, n_cols]
  uint32_t* cnt;        // [n_rows, chunks, nb1]
  uint32_t* part;       // [n_rows, slices, nb1]; cnt itself where a row is one chunk
  int64_t* order;       // [n_rows, n_cols]
  int64_t* offsets;     // [n_rows, nb1]
  int64_t n_rows, n_cols, chunk;
  int32_t chunks, slices, nb1, bits;  // nb1 = B + 1 counters; bits: 2^bits >= nb1; slices of kGroupSlice chunks
};

// between the LDS accesses of a wave's lanes to each other's words: the hardware runs a wave's LDS operations in order, this
// keeps the compiler from moving them
__device__ __forceinline__ void group_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the counter of a key: -1 (and anything that is no bin of the plan) is the last one
__device__ __forceinline__ uint32_t group_slot(int64_t key, int32_t nb1) {
  return (uint64_t)key < (uint64_t)(nb1 - 1) ? (uint32_t)key : (uint32_t)(nb1 - 1);
}

template <int W>
__device__ __forceinline__ void group_count_body(const GroupParams& __restrict__ p) {
  const int wave = threadIdx.x / kGroupStep, lane = threadIdx.x % kGroupStep;
  const int64_t unit = (int64_t)blockIdx.x * W + wave;  // (row, chunk)
  if (unit >= p.n_rows * p.chunks) return;              // (whole waves leave: nothing below waits for another wave)
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * p.nb1;
  for (int32_t b = lane; b < p.nb1; b += kGroupStep) my[b] = 0;
  group_wave_sync();
  const int64_t row = unit / p.chunks, begin = (unit % p.chunks) * p.chunk;
  const int64_t end = begin + p.chunk < p.n_cols ? begin + p.chunk : p.n_cols;
  const int64_t* keys = p.keys + row * p.n_cols;
  for (int64_t i = begin + lane; i < end + lane; i += kGroupStep * kGroupUnroll) {  // (i - lane < end: uniform)
    int64_t k[kGroupUnroll];
#pragma unroll
    for (int u = 0; u < kGroupUnroll; ++u) k[u] = i + u * kGroupStep < end ? keys[i + u * kGroupStep] : 0;
#pragma unroll
    for (int u = 0; u < kGroupUnroll; ++u)
      if (i + u * kGroupStep < end) atomicAdd(&my[group_slot(k[u], p.nb1)], 1u);
  }
  group_wave_sync();
  uint32_t* out = p.cnt + unit * p.nb1;
  for (int32_t b = lane; b < p.nb1; b += kGroupStep) out[b] = my[b];
}

// A slice's counters of one bin, per thread; the workgroups walk the (row, tile of bins, slice) units grid-strided.
// BASES false: part = their total.  BASES true: each becomes the running sum from part, the slice's base.
template <bool BASES>
__device__ __forceinline__ void group_slices_body(const GroupParams& __restrict__ p) {
  const int64_t nt = blockDim.x, tiles = (p.nb1 + nt - 1) / nt;
  const int64_t units = p.n_rows * tiles * p.slices;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / (tiles * p.slices), b = (u / p.slices) % tiles * nt + threadIdx.x;
    const int32_t slice = (int32_t)(u % p.slices);
    if (b >= p.nb1) continue;
    const int32_t c0 = slice * kGroupSlice, c1 = c0 + kGroupSlice < p.chunks ? c0 + kGroupSlice : p.chunks;
    uint32_t* cnt = p.cnt + row * p.chunks * p.nb1 + b;
    uint32_t* part = p.part + (row * p.slices + slice) * p.nb1 + b;
    if constexpr (!BASES) {
      uint32_t total = 0;
      for (int32_t c = c0; c < c1; ++c) total += cnt[(int64_t)c * p.nb1];
      *part = total;
    } else {
      uint32_t run = *part;
      for (int32_t c = c0; c < c1; ++c) {
        const uint32_t t = cnt[(int64_t)c * p.nb1];
        cnt[(int64_t)c * p.nb1] = run;
        run += t;
      }
    }
  }
}

// One workgroup per row, a thread per bin, the bins in tiles of the block with the running sum carried from tile to tile.
__device__ __forceinline__ void group_scan_body(const GroupParams& __restrict__ p) {
  __shared__ uint32_t s[256];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row = blockIdx.x;
  uint32_t* part = p.part + row * p.slices * p.nb1;
  int64_t* off = p.offsets + row * p.nb1;
  uint32_t carry = 0;
  for (int32_t b0 = 0; b0 < p.nb1; b0 += nt) {
    const int32_t b = b0 + tid;
    uint32_t total = 0;
    if (b < p.nb1)
      for (int32_t c = 0; c < p.slices; ++c) total += part[(int64_t)c * p.nb1 + b];
    s[tid] = total;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {  // inclusive scan of the tile's totals
      const uint32_t t = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    const uint32_t incl = s[tid], tile = s[nt - 1];
    __syncthreads();
    if (b < p.nb1) {
      uint32_t run = carry + incl - total;
      off[b] = (int64_t)run;
      for (int32_t c = 0; c < p.slices; ++c) {
        const uint32_t t = part[(int64_t)c * p.nb1 + b];
        part[(int64_t)c * p.nb1 + b] = run;
        run += t;
      }
    }
    carry += tile;
  }
}

template <int W>
__device__ __forceinline__ void group_scatter_body(const GroupParams& __restrict__ p) {
  const int wave = threadIdx.x / kGroupStep, lane = threadIdx.x % kGroupStep;
  const int64_t unit = (int64_t)blockIdx.x * W + wave;
  if (unit >= p.n_rows * p.chunks) return;
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * p.nb1;
  const uint32_t* base = p.cnt + unit * p.nb1;
  for (int32_t b = lane; b < p.nb1; b += kGroupStep) my[b] = base[b];
  group_wave_sync();
  const int64_t row = unit / p.chunks, begin = (unit % p.chunks) * p.chunk;
  const int64_t end = begin + p.chunk < p.n_cols ? begin + p.chunk : p.n_cols;
  const int64_t* keys = p.keys + row * p.n_cols;
  int64_t* out = p.order + row * p.n_cols;
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t i = begin + lane; i < end + lane; i += kGroupStep * kGroupUnroll) {
    int64_t k[kGroupUnroll];
#pragma unroll
    for (int u = 0; u < kGroupUnroll; ++u) k[u] = i + u * kGroupStep < end ? keys[i + u * kGroupStep] : 0;
#pragma unroll
    for (int u = 0; u < kGroupUnroll; ++u) {
      const int64_t pos = i + u * kGroupStep;
      if (pos - lane >= end) break;  // (uniform: the step lies past the chunk)
      const bool in = pos < end;
      const uint32_t key = in ? group_slot(k[u], p.nb1) : 0u;
      uint64_t peers = __ballot(in);
      for (int bit = 0; bit < p.bits; ++bit) {
        const bool one = (key >> bit) & 1u;
        const uint64_t m = __ballot(one);
        peers &= one ? m : ~m;
      }
      const uint32_t at = my[key];  // (every lane of a group reads the same word, before its lowest lane moves it on)
      const uint32_t rank = (uint32_t)__popcll(peers & below);
      group_wave_sync();
      if (in && rank == 0) my[key] = at + (uint32_t)__popcll(peers);
      group_wave_sync();
      if (in) out[(int64_t)at + rank] = pos;
    }
  }
}

// a plan without bins: every sample is dropped, and the order is the positions themselves
__device__ __forceinline__ void group_identity_body(int64_t* order, int64_t n_cols, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) order[i] = i % n_cols;
}

// The kernels: W waves of 64 lanes per workgroup, W * nb1 * 4 bytes of dynamic LDS.
template <int W>
__global__ void __launch_bounds__(kGroupStep * W) group_count(const GroupParams p) {
  group_count_body<W>(p);
}
__global__ void __launch_bounds__(256) group_totals(const GroupParams p) { group_slices_body<false>(p); }
__global__ void __launch_bounds__(256) group_scan(const GroupParams p) { group_scan_body(p); }
__global__ void __launch_bounds__(256) group_bases(const GroupParams p) { group_slices_body<true>(p); }
template <int W>
__global__ void __launch_bounds__(kGroupStep * W) group_scatter(const GroupParams p) {
  group_scatter_body<W>(p);
}
__global__ void __launch_bounds__(256) group_identity(int64_t* order, int64_t n_cols, int64_t n) { group_identity_body(order, n_cols, n); }

}  // namespace xhist
