// xhist_sort.hip.h — bin_sort: a row's samples grouped by bin and, inside each bin, sorted by value.  Per row of n_cols
// positions it writes
//   order    int64 [n_cols]  np.lexsort((vk, key)): by bin key (bin_index's, -1 as B), then by value key, ties in ascending position
//   offsets  int64 [B + 1]   offsets[b] = #{p : key[p] < b}, as bin_order's
// where vk is the order-preserving key of the value taken as float64 (extrema_key64: -0.0 < +0.0), complemented when the call
// is descending, and 2^64 - 1 for a NaN in either direction: NaN is last in its bin both ways.
//
// The engine is a stable least-significant-digit radix sort of (uint64 key, uint32 position) records on 8-bit digits between
// ping-pong buffers.  One pass over digit `shift / 8` is bin_order's three steps with 256 counters per wave, whatever B is:
//   sort_count     a row is cut into `chunks` contiguous chunks of `chunk` positions (a multiple of 64).  One wave64 owns one
//                  (row, chunk): it counts the digits of its records into its own 256 uint32 counters in LDS and writes them to
//                  cnt[row][chunk][256].  Plain LDS adds without a return value: counts do not depend on the order of the adds.
//   sort_totals, sort_scan, sort_bases
//                  cnt[row][chunk][digit] becomes where the (chunk, digit) run starts in the row: the exclusive prefix over
//                  digits of the totals over chunks, plus the counts of the earlier chunks.  The chunks go in slices of 64, as
//                  in bin_order; a row of one chunk is its own slice and sort_scan alone runs, on cnt itself.
//   sort_scatter   the same (row, chunk) -> wave assignment.  The wave loads its 256 bases into its LDS counters and walks its
//                  chunk 64 consecutive records at a step.  The lanes that hold the same digit find each other by 8 ballots; a
//                  lane's rank is the number of its peers below it; every lane reads its digit's counter, then the lowest lane
//                  of each group moves it on by the group's size.  The place of a record is base + rank, a function of the keys
//                  alone: no atomic's return value is read, and equal digits keep their order (the sort is stable).
// One wave owns one chunk, so the streaming loops have no workgroup barrier; a fence at wavefront scope (sort_wave_sync)
// separates the counter reads of a step from its writes.
//
// A scatter writes what its non-null destinations ask for: the key and the uint32 position (a pass inside a phase), the position
// alone (the last pass of the value phase), or the int64 position into the call's order block (the last pass of the call) with
// the key beside it, from which sort_offsets reads the runs of the bins.
//
// Around the engine:
//   sort_keys      values -> (value key, position): any real dtype through load_as<double>, any strides of an xhist_array
//   sort_gather    after the value phase: the bin key of every sorted position, as the engine's uint64 key
//   sort_offsets   over the sorted bin keys of a row: offsets[b'] = i for every b' in (key[i - 1], key[i]], with key[-1] = -1 and
//                  n_cols for every b' above the last key: every element of [n_rows, B + 1] is written exactly once
//
// Nothing here instantiates a kernel: xhist_sort.hip does.
#pragma once

#include "xhist_extrema.hip.h"  // extrema_key64 (templates and inline functions only)

namespace xhist {

constexpr int kSortDigits = 256;  // counters of a wave: one per value of an 8-bit digit
constexpr int kSortWaves = 4;     // waves of a workgroup of sort_count / sort_scatter: 4 KiB of LDS
constexpr int kSortStep = 64;     // records of one step of a wave; chunks are whole steps
constexpr int kSortUnroll = 4;    // record loads a lane keeps in flight
constexpr int kSortSlice = 64;    // chunks of one slice of the scan

// one launch over rows [r0, r0 + n_rows) of the call: every pointer is pre-advanced to r0 (cnt and part belong to the launch)
struct SortParams {
  const uint64_t* kin;  // [n_rows, n_cols] keys of the records
  const uint32_t* pin;  // [n_rows, n_cols] their positions
  uint64_t* kout;       // where the scattered keys go; nullptr: nowhere
  uint32_t* pout;       // where the scattered positions go as uint32; nullptr: nowhere
  int64_t* order;       // where they go as int64 (the call's order block); nullptr: nowhere
  uint32_t* cnt;        // [n_rows, chunks, 256]
  uint32_t* part;       // [n_rows, slices, 256]; cnt itself where a row is one chunk
  int64_t n_rows, n_cols, chunk;
  int32_t chunks, slices, shift;  // the digit is (key >> shift) & 255
};

// the values of a call as sort_keys reads them (an xhist_array, advanced to no row: `row0` is the launch's first row) and
// where the records go
struct SortKeyParams {
  const void* v_ptr;
  int64_t v_rs, v_cs, v_ir, v_os, row0;
  int32_t v_dt, descending;
  uint64_t* keys;  // [n_rows, n_cols]
  uint32_t* pos;   // [n_rows, n_cols]
  int64_t n_rows, n_cols;
};

// between the LDS accesses of a wave's lanes to each other's words: the hardware runs a wave's LDS operations in order, this
// keeps the compiler from moving them (bin_order's group_wave_sync; that header defines kernels, so it is not included here)
__device__ __forceinline__ void sort_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A slice's counters of one digit, per thread of a workgroup of 256; the workgroups walk the (row, slice) units grid-strided.
// BASES false: part = their total.  BASES true: each becomes the running sum from part, the slice's base.
template <bool BASES>
__device__ __forceinline__ void sort_slices_body(const SortParams& __restrict__ p) {
  const int64_t units = p.n_rows * p.slices;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / p.slices;
    const int32_t slice = (int32_t)(u % p.slices);
    const int32_t c0 = slice * kSortSlice, c1 = c0 + kSortSlice < p.chunks ? c0 + kSortSlice : p.chunks;
    uint32_t* cnt = p.cnt + row * p.chunks * kSortDigits + threadIdx.x;
    uint32_t* part = p.part + (row * p.slices + slice) * kSortDigits + threadIdx.x;
    if constexpr (!BASES) {
      uint32_t total = 0;
      for (int32_t c = c0; c < c1; ++c) total += cnt[(int64_t)c * kSortDigits];
      *part = total;
    } else {
      uint32_t run = *part;
      for (int32_t c = c0; c < c1; ++c) {
        const uint32_t t = cnt[(int64_t)c * kSortDigits];
        cnt[(int64_t)c * kSortDigits] = run;
        run += t;
      }
    }
  }
}

// the value key of the engine: NaN is 2^64 - 1 whatever the direction
__host__ __device__ __forceinline__ uint64_t sort_value_key(double v, bool descending) {
  if (v != v) return ~0ull;
  const uint64_t k = extrema_key64(v);
  return descending ? ~k : k;
}

__device__ __forceinline__ void sort_keys_body(const SortKeyParams& __restrict__ p) {
  const int64_t n = p.n_rows * p.n_cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / p.n_cols, col = i % p.n_cols;
    const double v = load_as<double>(p.v_ptr, p.v_dt, row_offset(p.row0 + row, p.v_rs, p.v_ir, p.v_os) + col * p.v_cs);
    p.keys[i] = sort_value_key(v, p.descending != 0);
    p.pos[i] = (uint32_t)col;
  }
}

// keys[i] = the bin key of position pos[i] of its row: binkeys is bin_index's int64 block, -1 (and anything that is no bin) is nb
__device__ __forceinline__ void sort_gather_body(const int64_t* __restrict__ binkeys, const uint32_t* __restrict__ pos,
                                                 uint64_t* __restrict__ keys, int64_t n_cols, int64_t n, int64_t nb) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = binkeys[i / n_cols * n_cols + pos[i]];
    keys[i] = (uint64_t)k < (uint64_t)nb ? (uint64_t)k : (uint64_t)nb;
  }
}

__device__ __forceinline__ void sort_count_body(const SortParams& __restrict__ p) {
  const int wave = threadIdx.x / kSortStep, lane = threadIdx.x % kSortStep;
  const int64_t unit = (int64_t)blockIdx.x * kSortWaves + wave;  // (row, chunk)
  if (unit >= p.n_rows * p.chunks) return;                       // (whole waves leave: nothing below waits for another wave)
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * kSortDigits;
  for (int b = lane; b < kSortDigits; b += kSortStep) my[b] = 0;
  sort_wave_sync();
  const int64_t row = unit / p.chunks, begin = (unit % p.chunks) * p.chunk;
  const int64_t end = begin + p.chunk < p.n_cols ? begin + p.chunk : p.n_cols;
  const uint64_t* keys = p.kin + row * p.n_cols;
  for (int64_t i = begin + lane; i < end + lane; i += kSortStep * kSortUnroll) {  // (i - lane < end: uniform)
    uint64_t k[kSortUnroll];
#pragma unroll
    for (int u = 0; u < kSortUnroll; ++u) k[u] = i + u * kSortStep < end ? keys[i + u * kSortStep] : 0;
#pragma unroll
    for (int u = 0; u < kSortUnroll; ++u)
      if (i + u * kSortStep < end) atomicAdd(&my[(uint32_t)(k[u] >> p.shift) & 255u], 1u);
  }
  sort_wave_sync();
  uint32_t* out = p.cnt + unit * kSortDigits;
  for (int b = lane; b < kSortDigits; b += kSortStep) out[b] = my[b];
}

// One workgroup of 256 threads per row, a thread per digit: the exclusive prefix over digits of the totals over slices, and
// part becomes the base of each (slice, digit).
__device__ __forceinline__ void sort_scan_body(const SortParams& __restrict__ p) {
  __shared__ uint32_t s[kSortDigits];
  const int tid = threadIdx.x;
  uint32_t* part = p.part + (int64_t)blockIdx.x * p.slices * kSortDigits + tid;
  uint32_t total = 0;
  for (int32_t c = 0; c < p.slices; ++c) total += part[(int64_t)c * kSortDigits];
  s[tid] = total;
  __syncthreads();
  for (int d = 1; d < kSortDigits; d <<= 1) {  // inclusive scan of the totals
    const uint32_t t = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  uint32_t run = s[tid] - total;
  for (int32_t c = 0; c < p.slices; ++c) {
    const uint32_t t = part[(int64_t)c * kSortDigits];
    part[(int64_t)c * kSortDigits] = run;
    run += t;
  }
}

__device__ __forceinline__ void sort_scatter_body(const SortParams& __restrict__ p) {
  const int wave = threadIdx.x / kSortStep, lane = threadIdx.x % kSortStep;
  const int64_t unit = (int64_t)blockIdx.x * kSortWaves + wave;
  if (unit >= p.n_rows * p.chunks) return;
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * kSortDigits;
  const uint32_t* base = p.cnt + unit * kSortDigits;
  for (int b = lane; b < kSortDigits; b += kSortStep) my[b] = base[b];
  sort_wave_sync();
  const int64_t row = unit / p.chunks, begin = (unit % p.chunks) * p.chunk;
  const int64_t end = begin + p.chunk < p.n_cols ? begin + p.chunk : p.n_cols;
  const int64_t r0 = row * p.n_cols;
  const uint64_t* keys = p.kin + r0;
  const uint32_t* pos = p.pin + r0;
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t i = begin + lane; i < end + lane; i += kSortStep * kSortUnroll) {
    uint64_t k[kSortUnroll];
    uint32_t q[kSortUnroll];
#pragma unroll
    for (int u = 0; u < kSortUnroll; ++u) {
      const bool in = i + u * kSortStep < end;
      k[u] = in ? keys[i + u * kSortStep] : 0;
      q[u] = in ? pos[i + u * kSortStep] : 0;
    }
#pragma unroll
    for (int u = 0; u < kSortUnroll; ++u) {
      const int64_t at_in = i + u * kSortStep;
      if (at_in - lane >= end) break;  // (uniform: the step lies past the chunk)
      const bool in = at_in < end;
      const uint32_t digit = (uint32_t)(k[u] >> p.shift) & 255u;
      uint64_t peers = __ballot(in);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool one = (digit >> bit) & 1u;
        const uint64_t m = __ballot(one);
        peers &= one ? m : ~m;
      }
      const uint32_t at = my[digit];  // (every lane of a group reads the same word, before its lowest lane moves it on)
      const uint32_t rank = (uint32_t)__popcll(peers & below);
      sort_wave_sync();
      if (in && rank == 0) my[digit] = at + (uint32_t)__popcll(peers);
      sort_wave_sync();
      if (in) {
        const int64_t to = r0 + (int64_t)at + rank;
        if (p.kout) p.kout[to] = k[u];
        if (p.pout) p.pout[to] = q[u];
        if (p.order) p.order[to] = (int64_t)q[u];
      }
    }
  }
}

// over the sorted bin keys [n_rows, n_cols] (each in [0, nb]): the start of every bin's run, offsets [n_rows, nb + 1]
__device__ __forceinline__ void sort_offsets_body(const uint64_t* __restrict__ keys, int64_t* __restrict__ offsets, int64_t n_rows,
                                                  int64_t n_cols, int64_t nb) {
  const int64_t per_row = n_cols + 1, n = n_rows * per_row;  // (element n_cols of a row: the tail above its last key)
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = j / per_row, i = j % per_row;
    const uint64_t* k = keys + row * n_cols;
    const int64_t lo = i == 0 ? 0 : (int64_t)k[i - 1] + 1;
    const int64_t hi = i == n_cols ? nb : (int64_t)k[i];
    int64_t* off = offsets + row * (nb + 1);
    for (int64_t b = lo; b <= hi; ++b) off[b] = i;
  }
}

// The kernels: sort_count / sort_scatter take kSortWaves waves of 64 lanes and kSortWaves * 1024 bytes of dynamic LDS.
__global__ void __launch_bounds__(256) sort_keys(const SortKeyParams p) { sort_keys_body(p); }
__global__ void __launch_bounds__(256) sort_gather(const int64_t* binkeys, const uint32_t* pos, uint64_t* keys, int64_t n_cols, int64_t n,
                                                   int64_t nb) {
  sort_gather_body(binkeys, pos, keys, n_cols, n, nb);
}
__global__ void __launch_bounds__(kSortStep* kSortWaves) sort_count(const SortParams p) { sort_count_body(p); }
__global__ void __launch_bounds__(256) sort_totals(const SortParams p) { sort_slices_body<false>(p); }
__global__ void __launch_bounds__(256) sort_scan(const SortParams p) { sort_scan_body(p); }
__global__ void __launch_bounds__(256) sort_bases(const SortParams p) { sort_slices_body<true>(p); }
__global__ void __launch_bounds__(kSortStep* kSortWaves) sort_scatter(const SortParams p) { sort_scatter_body(p); }
__global__ void __launch_bounds__(256) sort_offsets(const uint64_t* keys, int64_t* offsets, int64_t n_rows, int64_t n_cols, int64_t nb) {
  sort_offsets_body(keys, offsets, n_rows, n_cols, nb);
}

}  // namespace xhist
