// xhist_sort.hip.h — bin_sort: a row's samples grouped by bin and, inside each bin, sorted by value.  Per row of n_cols
// positions it writes
//   order    int64 [n_cols]  np.lexsort((vk, key)): by bin key (bin_index's, -1 as B), then by value key, ties in ascending position
//   offsets  int64 [B + 1]   offsets[b] = #{p : key[p] < b}, as bin_order's
// where vk is the order-preserving key of the value taken as float64 (extrema_key64: -0.0 < +0.0), complemented when the call
// is descending, and 2^64 - 1 for a NaN in either direction: NaN is last in its bin both ways.
//
// A stable least-significant-digit radix sort of (uint64 key, uint32 position) records on 8-bit digits between ping-pong
// buffers.  One pass over digit `shift / 8` is one pass of the count / scan / scatter engine of xhist_runs.hip.h, bin_order's:
// the slot of a record is its digit, so a wave keeps 256 counters and a step takes 8 ballots, whatever B is (sort_count,
// sort_scatter; the scan's kernels are the engine's own, and nobody reads its prefix).
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
#include "xhist_runs.hip.h"

namespace xhist {

constexpr int kSortDigits = 256;  // counters of a wave: one per value of an 8-bit digit
constexpr int kSortWaves = 4;     // waves of a workgroup of sort_count / sort_scatter: 4 KiB of LDS

// The records of one pass (the policy of xhist_runs.hip.h) and the argument of its kernels: runs.width = 256, runs.offsets
// nullptr, and cnt and part belong to the launch.
struct SortParams {
  RunsParams runs;
  const uint64_t* kin;  // [n_rows, n_cols] keys of the records
  const uint32_t* pin;  // [n_rows, n_cols] their positions
  uint64_t* kout;       // where the scattered keys go; nullptr: nowhere
  uint32_t* pout;       // where the scattered positions go as uint32; nullptr: nowhere
  int64_t* order;       // where they go as int64 (the call's order block); nullptr: nowhere
  int32_t shift;        // the digit is (key >> shift) & 255

  static constexpr int kWidth = kSortDigits, kBits = 8;
  typedef uint64_t Key;
  typedef uint32_t Rest;  // the position the record came from
  __device__ __forceinline__ uint64_t key(int64_t at) const { return kin[at]; }
  __device__ __forceinline__ uint32_t rest(int64_t at) const { return pin[at]; }
  __device__ __forceinline__ uint32_t slot(uint64_t key, int32_t) const { return (uint32_t)(key >> shift) & 255u; }
  __device__ __forceinline__ void store(int64_t to, uint64_t key, uint32_t from, int64_t) const {
    if (kout) kout[to] = key;
    if (pout) pout[to] = from;
    if (order) order[to] = (int64_t)from;
  }
};

// where the records of sort_keys go
struct SortKeyParams {
  ValuesRead v;
  int32_t descending;
  uint64_t* keys;  // [n_rows, n_cols]
  uint32_t* pos;   // [n_rows, n_cols]
  int64_t n_rows, n_cols;
};

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
    const double v = load_as<double>(p.v.ptr, p.v.dt, row_offset(p.v.row0 + row, p.v.rs, p.v.ir, p.v.os) + col * p.v.cs);
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
__global__ void __launch_bounds__(kRunsStep* kSortWaves) sort_count(const SortParams p) { runs_count_body<kSortWaves>(p); }
__global__ void __launch_bounds__(kRunsStep* kSortWaves) sort_scatter(const SortParams p) { runs_scatter_body<kSortWaves>(p); }
__global__ void __launch_bounds__(256) sort_offsets(const uint64_t* keys, int64_t* offsets, int64_t n_rows, int64_t n_cols, int64_t nb) {
  sort_offsets_body(keys, offsets, n_rows, n_cols, nb);
}

}  // namespace xhist
