// xhist_group.hip.h — bin_order: the stable group-by of a row's samples by bin, a counting sort of keys that are bin numbers.
// Per row of n_cols positions with keys in [0, B) or -1 (bin_index's block; -1 sorts as key B) it writes
//   order    int64 [n_cols]  the positions sorted by key, positions of equal keys ascending (np.argsort(key, kind="stable"))
//   offsets  int64 [B + 1]   offsets[b] = #{p : key[p] < b}: bin b is order[offsets[b] : offsets[b + 1]], the dropped samples
//                            are order[offsets[B] :]
// by one pass of the count / scan / scatter engine of xhist_runs.hip.h over the key block: a record is a key, its slot the key
// itself (B for -1), a wave keeps B + 1 counters, and a placed record stores its position.  The scan's prefix is the offsets.
//
// Nothing here instantiates a kernel: xhist_group.hip does.
#pragma once

#include "xhist_runs.hip.h"

namespace xhist {

// the counter of a key: -1 (and anything that is no bin of the plan) is the last one
__device__ __forceinline__ uint32_t group_slot(int64_t key, int32_t nb1) {
  return (uint64_t)key < (uint64_t)(nb1 - 1) ? (uint32_t)key : (uint32_t)(nb1 - 1);
}

// bin_order's records (the policy of xhist_runs.hip.h) and the argument of its kernels: runs.width = B + 1, runs.offsets the
// call's offsets block
struct GroupParams {
  RunsParams runs;
  const int64_t* keys;  // [n_rows, n_cols]
  int64_t* order;       // [n_rows, n_cols]
  int32_t bits;         // 2^bits >= B + 1

  static constexpr int kWidth = 0, kBits = 0;
  typedef int64_t Key;
  struct Rest {};
  __device__ __forceinline__ int64_t key(int64_t at) const { return keys[at]; }
  __device__ __forceinline__ Rest rest(int64_t) const { return Rest{}; }
  __device__ __forceinline__ uint32_t slot(int64_t key, int32_t width) const { return group_slot(key, width); }
  __device__ __forceinline__ void store(int64_t to, int64_t, Rest, int64_t pos) const { order[to] = pos; }
};

// a plan without bins: every sample is dropped, and the order is the positions themselves
__device__ __forceinline__ void group_identity_body(int64_t* order, int64_t n_cols, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) order[i] = i % n_cols;
}

// The kernels: W waves of 64 lanes per workgroup, W * (B + 1) * 4 bytes of dynamic LDS.
template <int W>
__global__ void __launch_bounds__(kRunsStep * W) group_count(const GroupParams p) {
  runs_count_body<W>(p);
}
template <int W>
__global__ void __launch_bounds__(kRunsStep * W) group_scatter(const GroupParams p) {
  runs_scatter_body<W>(p);
}
__global__ void __launch_bounds__(256) group_identity(int64_t* order, int64_t n_cols, int64_t n) { group_identity_body(order, n_cols, n); }

}  // namespace xhist
