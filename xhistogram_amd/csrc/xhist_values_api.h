// xhist_values_api.h — what the C ABI unit (xhist_capi.hip) and the units of the per-bin statistics of a value array share on
// the host: the view of a plan, the record of one call, and the drivers' prototypes.  Declarations only, no device code: the
// C ABI unit includes this header, each statistic's unit reaches it through xhist_values.hip.h.
#pragma once

#include "../../include/xhist_amd.h"

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>

namespace xhist {
struct DimTable;
struct RunsParams;
}

// What the units need of a plan (filled by xhist_capi.hip's values_plan()): the compare domain, the native (start, cnt)
// tables, the uint16 tables of the linear scan in the float64 and the float32-threshold domain (blob == nullptr: not built),
// and whether every dimension has arithmetic edges.
struct ValuesTables {
  const xhist::DimTable* dim;
  const uint64_t* blob;
  int32_t words;
  int max_cnt;
};
struct ValuesPlan {
  int n_dims, cmp;
  int64_t n_bins;
  int cus;
  size_t lds_max;
  bool arith;
  ValuesTables native, fine64, fine32;
};

// scratch of `bytes` bytes from the library's allocator, freed by the C ABI unit after the call; nullptr: out of memory
typedef void* (*xhist_values_alloc_fn)(void* ctx, size_t bytes);

// What stays the same through one call (built once by xhist_capi.hip's execute_values, which owns everything it points to):
// the plan; the input streams (`values`: nullptr for the maps that read the samples alone; `third`: the weights, or the second value array of the covariances; `fourth`: the weights of
// the weighted covariance; nullptr where a statistic has none); the shape; the stream; where an error message and the line
// about the launches go (the latter becomes the plan's describe()); the scratch allocator.
struct ValuesCall {
  ValuesPlan pl;
  const xhist_array *samples, *values, *third, *fourth;
  int64_t n_rows, n_cols;
  hipStream_t stream;
  char* err;
  size_t err_cap;
  char* desc;
  size_t desc_cap;
  xhist_values_alloc_fn alloc;
  void* alloc_ctx;

  void* scratch(size_t bytes) const { return alloc(alloc_ctx, bytes); }
  // the message into `err`; returns `code`
  __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) const {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, err_cap, fmt, ap);
    va_end(ap);
    return code;
  }
  __attribute__((format(printf, 2, 3))) void describe(const char* fmt, ...) const {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(desc, desc_cap, fmt, ap);
    va_end(ap);
  }
};

// The drivers: the launches of one statistic on k.stream, for DEVICE arrays the caller has validated, the plan's device current.
// Each returns XHIST_OK, or an error status with a message in k.err, and writes a line about its launches to k.desc.  They are
// reached through execute_values alone, under one of two contracts:
//   planes  outputs are [n_rows, n_bins] planes of 8-byte elements, or blocks [planes, n_rows, n_bins] of them: n_rows * n_bins > 0,
//           n_cols >= 0
//   dense   outputs are dense [n_rows, n_cols] or CSR blocks (xhist_map_run, xhist_group_run, xhist_sort_run, xhist_rank_run,
//           xhist_unique_run, xhist_unique_w_run): n_rows > 0, n_cols >= 0 and n_bins >= 0.  A call without columns and a plan without bins are the
//           driver's own branches: it writes every element the outputs still have and a line with "none" in it.
// For the drivers behind the sorted order (sort, rank, mode, unique and the weighted twins of the last two; group for the first) the front has refused n_cols >= 2^31
// and n_bins + 1 > 2^32, XHIST_ERR_UNSUPPORTED, and an unknown rank method and a negative size, XHIST_ERR_INVALID.

// xhist_extrema.hip: minimum and maximum (prepare, binning, finalize; `accumulate`: the outputs hold an earlier result), and
// histogram_argextrema (the two prepares, pass 1, pass 2, finalize): out_values [2] (minimum, maximum), out_index [2] int64
// (their positions; -1: empty bin)
int xhist_extrema_run(const ValuesCall& k, double* out_min, double* out_max, int accumulate);
int xhist_argextrema_run(const ValuesCall& k, double* out_values, int64_t* out_index);

// xhist_sum.hip: histogram_sum, the per-bin sum that does not depend on the order of arrival (pass 1 is histogram_extrema's,
// pass 2 adds integer limbs, a finalize rounds once): out_count int64, out_total float64; five planes of scratch from k.alloc.
// XHIST_ERR_UNSUPPORTED for k.n_cols >= 2^31, before any launch.
int xhist_sum_run(const ValuesCall& k, int64_t* out_count, double* out_total);

// The two-pass statistics (two_pass_run<M> of xhist_values.hip.h, which takes its block for the sums of deviations from
// k.alloc): out_first is the int64 count, or the float64 sum of weights of a weighted form (k.third, k.fourth for cov).
//   xhist_meanvar.hip, xhist_meanvar_w.hip   out_mean [1], out_m2 [1]; skew_kurt: out_m2 [3] (M2, M3, M4)
//   xhist_cov.hip, xhist_cov_w.hip           k.third the second value array; out_mean [2] (mean_a, mean_b), out_m2 [3] (M2_a,
//                                            C_ab, M2_b)
int xhist_meanvar_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);
int xhist_meanvar_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);
int xhist_skew_kurt_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);
int xhist_skew_kurt_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);
int xhist_cov_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);
int xhist_cov_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2);

// xhist_quantile.hip, xhist_quantile_w.hip: q (host, n_q values in [0, 1]) and the method code (XHIST_Q_*; the weighted form,
// k.third its weights, is numpy's inverted_cdf) -> out, float64 [n_q, n_rows, n_bins]
int xhist_quantile_run(const ValuesCall& k, const double* q, int n_q, int method, double* out);
int xhist_quantile_w_run(const ValuesCall& k, const double* q, int n_q, double* out);

// xhist_map.hip: the per-sample maps.  op is XHIST_MAP_INDEX (k.values nullptr, no table), XHIST_MAP_TAKE (k.values nullptr,
// centre the table) or XHIST_MAP_ANOMALY (k.values the values, centre the means, scale nullptr or the standard deviations);
// centre and scale are float64 [n_rows, n_bins], out a dense [n_rows, n_cols] block of 8-byte elements, each written once (a
// plan without bins: bytes of all ones, -1 and NaN).
int xhist_map_run(const ValuesCall& k, int op, const double* centre, const double* scale, void* out);

// xhist_group.hip: bin_order, the stable group-by of a row's samples by bin (k.values nullptr).  out_order is a dense int64
// [n_rows, n_cols] block, out_offsets int64 [n_rows, n_bins + 1]; every element of both is written exactly once.  The keys are
// xhist_map_run's XHIST_MAP_INDEX block, in scratch from k.alloc with the counter table.  A plan without bins: offsets
// [n_rows, 1] of zeros, every row's order its positions.  XHIST_ERR_UNSUPPORTED for (n_bins + 1) * 4 bytes beyond the LDS of a
// workgroup, before any launch.
int xhist_group_run(const ValuesCall& k, int64_t* out_order, int64_t* out_offsets);
// xhist_group.hip: the scan of the count / scan / scatter engine (xhist_runs.hip.h) for one batch of rows, whose kernels that unit
// alone defines: totals where a row is cut into several chunks, scan, bases where it is cut.  It turns the counters the count
// kernel wrote into the bases the scatter kernel reads, and writes p.offsets where that is not nullptr.  A width of 256 runs the
// instantiations with that width fixed.  `who` ("group", "sort") names the caller in the message of a failed launch.
int xhist_runs_scan(const ValuesCall& k, const xhist::RunsParams& p, const char* who);

// xhist_sort.hip: bin_sort, a row's samples grouped by bin and sorted by value inside each bin (k.values the values; `descending`
// nonzero: largest first, NaN still last).  The outputs are bin_order's; every element of both is written exactly once.  A
// stable radix sort on 8-bit digits of (value key, position), then of the gathered bin keys: 32 bytes of scratch per sample
// from k.alloc.  A plan without bins: the whole row sorted by value, one offset of 0 per row.
// `hand` (nullptr: nobody asks) receives what bin_rank takes over from the sort: the sorted bin keys [n_rows, n_cols], each in
// [0, n_bins], in scratch of the call (nullptr for a plan without bins), and the rows of one launch.
struct SortHandover {
  const uint64_t* keys;
  int64_t rows_per_launch;
};
int xhist_sort_run(const ValuesCall& k, int descending, int64_t* out_order, int64_t* out_offsets, SortHandover* hand = nullptr);

// xhist_rank.hip: bin_rank, the rank of every sample's value among the non-NaN values of its bin (k.values the values; method
// an XHIST_RANK_* code; `descending` nonzero: largest first; `pct` nonzero: divided by the bin's count of non-NaN values, by its
// distinct values for XHIST_RANK_DENSE).  out is a dense float64 [n_rows, n_cols] block in position order, every element
// written exactly once; NaN for a sample that is not counted and for a NaN value.  It runs xhist_sort_run into scratch and
// six kernels over the sorted order.  Scratch from k.alloc, one block on top of the sort's 32 bytes per sample: 8 bytes per
// sample of order, n_rows * (n_bins + 1) * 8 bytes of offsets, 28 bytes per 64 samples of head and NaN words with their three
// uint32 scalars, 12 bytes per 65536 samples of tile scalars, and n_rows * n_bins * 8 bytes of divisors when pct.  A plan
// without bins: all NaN, bytes of all ones.
int xhist_rank_run(const ValuesCall& k, int method, int descending, int pct, double* out);

// xhist_rank.hip: histogram_mode, per (row, bin) the number of non-NaN values, the number of distinct ones (IEEE ==), the most
// frequent value (the smallest of the most frequent ones, with the bits of its first sample in the sort's ascending order) and
// how often it occurs (k.values the values).  Four [n_rows, n_bins] planes, int64 but out_mode; an empty bin gets 0, 0, NaN
// (0x7ff8000000000000) and 0; every element is written exactly once.  It runs xhist_sort_run into scratch, the four kernels
// that build bin_rank's sorted domain and two of its own.  Scratch from k.alloc is bin_rank's without the divisors; the slots
// of the atomic maximum are the out_mode_count block, zeroed by the call.
int xhist_mode_run(const ValuesCall& k, int64_t* out_count, int64_t* out_nunique, double* out_mode, int64_t* out_mode_count);

// xhist_rank.hip: bin_unique, per row the distinct non-NaN values of every bin in CSR form (k.values the values; equality is
// IEEE ==).  out_offsets int64 [n_rows, n_bins + 1]: the distinct values in the bins below b, always the truth; out_uniques
// float64 and out_counts int64 [n_rows, size]: a bin's values ascending, each with the bits of its first sample in the sort's
// ascending order, and how many samples hold it; entries from min(out_offsets[r, n_bins], size) on are padding (0x7ff8000000000000
// and 0), entries from `size` on are stored nowhere; out_inverse (nullptr: none) int64 [n_rows, n_cols] in position order: the
// sample's entry, beyond `size` too, -1 for a sample that is not counted and for a NaN value.  Every element of every output is
// written and nothing outside them.  It runs xhist_sort_run into scratch, the four kernels that build bin_rank's sorted domain
// and up to five of its own; scratch from k.alloc is bin_rank's without the divisors.  A call without columns and a plan without
// bins: offsets of zeros, padding, an inverse of -1.  size >= 0.
int xhist_unique_run(const ValuesCall& k, int64_t size, double* out_uniques, int64_t* out_counts, int64_t* out_offsets,
                     int64_t* out_inverse);

// xhist_rank.hip: bin_weighted_unique, xhist_unique_run with k.third the weights (any real dtype, taken as float64) and one block
// more, out_weight_sums float64 [n_rows, size]: the float64 sum of the weights of the samples out_counts counts, +0.0 in the
// padding.  The sum of a run is a fixed tree of additions over its samples in the sort's order (xhist_wruns.hip.h): no atomic,
// and the same bits for any grid, batch of rows, width and stream.  Five kernels more for a width above 0, and 16 bytes of scratch
// per 64 samples and per 65536 samples of a row.  out_weight_sums may be nullptr where size == 0.
int xhist_unique_w_run(const ValuesCall& k, int64_t size, double* out_uniques, int64_t* out_counts, double* out_weight_sums,
                       int64_t* out_offsets, int64_t* out_inverse);

// xhist_rank.hip: histogram_weighted_mode, xhist_mode_run's out_count and out_nunique, and per (row, bin) the value whose samples'
// weights (k.third) have the largest float64 sum (IEEE compare, the smallest value among equal sums) and that sum, bitwise what
// xhist_unique_w_run stores for the entry; both 0x7ff8000000000000 where a sum of the bin is NaN; an empty bin gets 0, 0, NaN and
// +0.0.  Four [n_rows, n_bins] planes, every element written exactly once.  The sums go to 8 bytes of scratch per sample; the
// slots of the integer atomics are the out_mode_weight and out_mode blocks, filled by the call and finished in place.
int xhist_mode_w_run(const ValuesCall& k, int64_t* out_count, int64_t* out_nunique, double* out_mode, double* out_mode_weight);
