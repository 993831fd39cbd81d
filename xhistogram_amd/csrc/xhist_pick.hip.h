// xhist_pick.hip.h — kernel pickers of the float32 / float64 vector family.  The template instantiations
// behind them are the bulk of the build (several hundred kernels), so they live in two translation
// units of their own (xhist_pick_f64.hip, xhist_pick_f32.hip) that compile in parallel with
// xhist_capi.hip; each exports the two plain functions declared at the end.
#pragma once

#include "xhist_kernels.hip.h"
#include "xhist_partition.hip.h"
#include "xhist_route.hip.h"
#include "xhist_exchange.hip.h"
#include "xhist_lanes.hip.h"

#include <type_traits>

#include "../../include/xhist_amd.h"

using namespace xhist;

typedef void (*kernel_fn)(const Params);
typedef void (*kernel_fn_acc)(const uint16_t*, const void*, const uint64_t*, void*, int64_t, int, int);
typedef void (*kernel_fn_count)(const Params, uint32_t*);
typedef void (*kernel_fn_lanes)(const Params, int32_t, int64_t);
typedef void (*kernel_fn_scatter)(const uint32_t*, const void*, int64_t, const uint64_t*, uint16_t*, void*, int, int);
typedef void (*kernel_fn_route)(const Params, const RouteArgs);
typedef void (*kernel_fn_acc_chunks)(const RouteArgs, void*, int64_t, int, int, int);

// Samples a lane bins as one branch-free batch = VEC x UNROLL, capped by register pressure: per
// sample and dimension the batch keeps the value, its running count and (linear scan) up to
// SCAN edge values in VGPRs, and 1024-thread workgroups leave 128 VGPRs per lane.
constexpr int unroll_for(int D, int vec, int scan) {
  if (scan_is_pack(scan)) scan = 2;  // packed bucket entries: one 16-byte entry per sample and dimension, as the two-edge scan
  if (scan == kScanArith32) scan = 1;  // float32 arithmetic: lighter than the one-edge scan (the host sizes tiles and grids by this too)
  int cap = D == 1 ? 16 : (D == 2 ? 8 : 4);
  if (D >= 2 && scan >= 3) cap /= 2;
  if (D == 1 && scan >= 3 && vec == 4) cap = 8;
  const int u = cap / vec < 1 ? 1 : cap / vec;
  return u > 4 ? 4 : u;
}

// ---- what the pickers of xhist_exec_device.hip.h can never ask for (round 6, VERDICT r5 "next" #2) -------------------------------
// The dispatch tables below were a plain cross product; the census of round 6 (tests/test_gpu_census.py walks the product with the
// smallest inputs that select each entry) found entries that NO input selects, for reasons of arithmetic, not of test coverage.
// They are not instantiated any more; the rules, with the reason each one holds:
//
//  * ONE input (D == 1), histogram beyond the replicated LDS copies.  The plan's bucket grid has at most 8192 buckets per input, so
//    n bins put n / 8192 edges into a bucket: "one edge per bucket" (SCAN 1) means <= 8192 bins — 64 KB of float64 sums, 32 KB of
//    counts — which always fit LDS next to their edges: no packed-uint16, bin-slice, partition-count or routing kernel is ever
//    asked for with D == 1 and SCAN 1.  Two per bucket (<= 16384 bins) still fit as uint32 counts next to float32 thresholds, so
//    float32 counts never reach the packed / sliced forms with SCAN 2 either; float64 counts do (14 000 bins: the edges take 112 KB).
//    Packed bucket entries (SCAN 6-8) need at least n / 3 sixteen-byte entries: beyond ~10 000 bins they do not fit LDS, below
//    that the histogram fits as uint32 — never with the packed-uint16 home for one input.
//  * The routing pass keeps its tables in LDS next to the sort buffers (>= 70 KB): for ONE input beyond LDS only float32
//    thresholds of a weighted histogram fit (<= 16384 bins, SCAN 0 or 2, the short tile); everything else with one input digitizes
//    arithmetically or takes the three-pass route.
//  * Bin slices keep float64 sums in LDS and counts as packed uint16 pairs: there is no sliced uint32 home.
//  * The generic family keeps its histogram in LDS only when its tables are there too (place_histogram() in xhist_exec_device.hip.h).
constexpr bool one_input_home_exists(bool is_f64, bool unweighted, int scan, int hist_home /* 0 global, 1 lds, 2 packed */) {
  (void)unweighted;
  if (hist_home == 2) return scan == 0 || scan == 3 || scan == 4 || scan == kScanArith || (scan == 2 && is_f64);
  return true;
}

// ---- the "hot" translation unit (round 6) ------------------------------------------------------------------------------------
// HIP loads a translation unit's code object when the first kernel of it is launched: 7-8 ms for each of the 3 MB objects of
// xhist_capi / xhist_pick_f64 / xhist_pick_f32 (tools/first_call_split.py: the first plan paid 8.2 ms for build_tables' module,
// the first execute 7 ms for the histogram kernel's).  The kernels a FIRST call most likely needs — output zeroing, the table
// builders, and the vector kernels for one or two float inputs with a histogram in LDS on uniform-style edges (one edge per bucket,
// or the arithmetic digitize: `bins=int`, np.linspace), i.e. BASELINE C1 / C2 / C4 and most dask-chunk-sized calls — live in a small
// translation unit of their own (xhist_hot.hip, ~40 kernels): its code object loads in a fraction of a millisecond and nothing
// else is loaded until a call needs it.  The big units do not instantiate them (one kernel, one code object).
constexpr bool is_hot_kernel(int D, int scan, int hist) {
  return (D == 1 || D == 2) && hist == kHistLds && (scan == 1 || scan == kScanArith || scan == kScanArith32);
}
kernel_fn xhist_pick_hot(int sdt, int wdt, int D, int scan, int hist);  // nullptr: not a hot kernel (xhist_hot.hip)
kernel_fn xhist_pick_hot_long(int sdt, int scan);                       // the long-tile variants of one unweighted float input
int xhist_hot_zero_words(unsigned long long* p, int64_t n, int grid, hipStream_t stream);  // launches; returns hipGetLastError()
int xhist_hot_build_tables(int dom, bool lut16, const DimTable& t, uint64_t* blob, int32_t* scratch);
int xhist_hot_build_pack_tables(const DimTable& t, uint64_t* blob, int32_t* scratch, const float* thr);
int xhist_hot_minmax_flat(bool f64, const void* x, int64_t n, double* partial, int grid, hipStream_t stream);

// partitioned mode: pseudo "hist" codes selecting the two part_pass kernels, and their geometry
constexpr int kHistPartCount = 4, kHistLanes = 6, kHistLanes16 = 7;
constexpr int kPartMaxParts = 256;

template <typename ST, typename WT, int D, int SCAN>
static kernel_fn fast_pick(int hist) {
  constexpr bool unweighted = std::is_same<WT, NoWeight>::value;
  constexpr int wsz = unweighted ? 0 : (int)sizeof(typename std::conditional<unweighted, float, WT>::type);
  constexpr int VEC = 16 / (((int)sizeof(ST) > wsz) ? (int)sizeof(ST) : wsz);
  constexpr int U = unroll_for(D, VEC, SCAN);
  if (hist == kHistPartCount) {
    if constexpr (D == 1 && SCAN == 1) return nullptr;  // (one input, one edge per bucket: fits LDS, see above)
    else return (kernel_fn)part_count<ST, D, VEC, SCAN>;
  }
  if (hist == kHistLanes) {  // (float64 sum columns; counts take the uint16 columns below and nothing else)
    if constexpr (!unweighted) return (kernel_fn)hist_lanes<ST, WT, D, SCAN, (D == 1 ? 8 : 4), false>;
    else return nullptr;
  }
  if (hist == kHistLanes16) {
    if constexpr (unweighted) return (kernel_fn)hist_lanes<ST, WT, D, SCAN, (D == 1 ? 8 : 4), true>;
    else return nullptr;
  }
  if (hist == kHistLds) {
    if constexpr (is_hot_kernel(D, SCAN, kHistLds) && (std::is_same<ST, double>::value || std::is_same<ST, float>::value)) return nullptr;  // (xhist_hot.hip has it)
    else return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistLds, SCAN>;
  }
  if (hist == kHistPacked) {
    if constexpr (unweighted && (D > 1 || one_input_home_exists(std::is_same<ST, double>::value, true, SCAN, 2))) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistPacked, SCAN>;
    else return nullptr;
  }
  return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistGlobal, SCAN>;
}

// table-free digitize (arithmetic edges): only the kernels that mode is selected for
template <typename ST, typename WT, int D>
static kernel_fn fast_pick_arith(int hist) {
  constexpr bool unweighted = std::is_same<WT, NoWeight>::value;
  constexpr int wsz = unweighted ? 0 : (int)sizeof(typename std::conditional<unweighted, float, WT>::type);
  constexpr int VEC = 16 / (((int)sizeof(ST) > wsz) ? (int)sizeof(ST) : wsz);
  constexpr int U = unroll_for(D, VEC, kScanArith);
  if (hist == kHistPartCount) return (kernel_fn)part_count<ST, D, VEC, kScanArith>;
  if (hist == kHistLds) {
    if constexpr (is_hot_kernel(D, kScanArith, kHistLds)) return nullptr;  // (xhist_hot.hip has it)
    else return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistLds, kScanArith>;
  }
  if (hist == kHistPacked) {
    if constexpr (unweighted) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistPacked, kScanArith>;
    else return nullptr;
  }
  if (hist == kHistGlobal) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistGlobal, kScanArith>;
  return nullptr;
}

// packed bucket entries (count_le_pack / count_le_pack_f32): float64 or float32 samples, histograms in LDS (replicated or
// packed uint16 counters)
template <typename ST, typename WT, int D, int SCAN>
static kernel_fn fast_pick_pack(int hist) {
  if constexpr (std::is_same<ST, double>::value || std::is_same<ST, float>::value) {
    constexpr bool unweighted = std::is_same<WT, NoWeight>::value;
    constexpr int wsz = unweighted ? 0 : (int)sizeof(typename std::conditional<unweighted, float, WT>::type);
    constexpr int VEC = 16 / (((int)sizeof(ST) > wsz) ? (int)sizeof(ST) : wsz);
    constexpr int U = unroll_for(D, VEC, SCAN);
    if constexpr (SCAN == kScanPackG) {  // the row-per-lane family takes the general variant only (one set of kernels)
      if (hist == kHistLanes) {
        if constexpr (!unweighted) return (kernel_fn)hist_lanes<ST, WT, D, SCAN, (D == 1 ? 8 : 4), false>;
        else return nullptr;
      }
      if (hist == kHistLanes16) {
        if constexpr (unweighted) return (kernel_fn)hist_lanes<ST, WT, D, SCAN, (D == 1 ? 8 : 4), true>;
        else return nullptr;
      }
    }
    if (hist == kHistLds) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistLds, SCAN>;
    if (hist == kHistPacked) {
      if constexpr (unweighted && D > 1) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistPacked, SCAN>;  // (one input: see above)
    }
  }
  return nullptr;
}

// float32 samples on arithmetic edges, digitized in float32 arithmetic (bin_arith32_fast): LDS histograms
template <typename ST, typename WT, int D>
static kernel_fn fast_pick_arith32(int hist) {
  if constexpr (std::is_same<ST, float>::value) {
    constexpr bool unweighted = std::is_same<WT, NoWeight>::value;
    constexpr int wsz = unweighted ? 0 : (int)sizeof(typename std::conditional<unweighted, float, WT>::type);
    constexpr int VEC = 16 / (((int)sizeof(ST) > wsz) ? (int)sizeof(ST) : wsz);
    constexpr int U = unroll_for(D, VEC, kScanArith32);
    if (hist == kHistLds) {
      if constexpr (is_hot_kernel(D, kScanArith32, kHistLds)) return nullptr;  // (xhist_hot.hip has it)
      else return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistLds, kScanArith32>;
    }
  }
  return nullptr;
}

template <typename ST, typename WT, int D>
static kernel_fn fast_pick_s(int scan, int hist) {
  switch (scan) {
    case kScanArith: return fast_pick_arith<ST, WT, D>(hist);
    case kScanArith32: return fast_pick_arith32<ST, WT, D>(hist);
    case kScanPack2: return fast_pick_pack<ST, WT, D, kScanPack2>(hist);
    case kScanPack3: return fast_pick_pack<ST, WT, D, kScanPack3>(hist);
    case kScanPackG: return fast_pick_pack<ST, WT, D, kScanPackG>(hist);
    case 1: return fast_pick<ST, WT, D, 1>(hist);
    case 2: return fast_pick<ST, WT, D, 2>(hist);
    case 3: return fast_pick<ST, WT, D, 3>(hist);
    case 4: return fast_pick<ST, WT, D, 4>(hist);
    default: return fast_pick<ST, WT, D, 0>(hist);
  }
}

template <typename ST, typename WT>
static kernel_fn fast_pick_d(int D, int scan, int hist) {
  switch (D) {
    case 1: return fast_pick_s<ST, WT, 1>(scan, hist);
    case 2: return fast_pick_s<ST, WT, 2>(scan, hist);
    case 3: return fast_pick_s<ST, WT, 3>(scan, hist);
    default: return nullptr;
  }
}

template <typename ST>
static kernel_fn fast_pick_w(int wdt, int D, int scan, int hist) {
  switch (wdt) {
    case -1: return fast_pick_d<ST, NoWeight>(D, scan, hist);
    case XHIST_F64: return fast_pick_d<ST, double>(D, scan, hist);
    case XHIST_F32: return fast_pick_d<ST, float>(D, scan, hist);
    default: return nullptr;
  }
}

// ------------------------------------------------------------------------------------------
// bin slices (hist_fast<..., SLICED = true>): float samples, LDS or packed-uint16 histograms, table
// digitize with <= 2 edges per bucket or arithmetic edges
template <typename ST, typename WT, int D, int SCAN>
static kernel_fn sliced_pick(int hist) {
  constexpr bool unweighted = std::is_same<WT, NoWeight>::value;
  constexpr int wsz = unweighted ? 0 : (int)sizeof(typename std::conditional<unweighted, float, WT>::type);
  constexpr int VEC = 16 / (((int)sizeof(ST) > wsz) ? (int)sizeof(ST) : wsz);
  constexpr int U = unroll_for(D, VEC, SCAN);
  // (execute_device asks for float64 sums in LDS when weighted, for packed uint16 counts when not: nothing else; one input:
  //  never with one edge per bucket, and float32 counts not with two — see the rules at the top)
  if (hist == kHistLds) {
    if constexpr (!unweighted && !(D == 1 && SCAN == 1)) return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistLds, SCAN, false, true>;
  }
  if (hist == kHistPacked) {
    if constexpr (unweighted && (D > 1 || SCAN == kScanArith || (SCAN == 2 && std::is_same<ST, double>::value)))
      return (kernel_fn)hist_fast<ST, WT, D, VEC, U, kHistPacked, SCAN, false, true>;
  }
  return nullptr;
}

template <typename ST, typename WT>
static kernel_fn sliced_pick_ds(int D, int scan, int hist) {
#define XH_SLICED_CASE(DD)                                            \
  case DD:                                                            \
    if (scan == 1) return sliced_pick<ST, WT, DD, 1>(hist);           \
    if (scan == 2) return sliced_pick<ST, WT, DD, 2>(hist);           \
    if (scan == kScanArith) return sliced_pick<ST, WT, DD, kScanArith>(hist); \
    return nullptr;
  switch (D) {
    XH_SLICED_CASE(1)
    XH_SLICED_CASE(2)
    XH_SLICED_CASE(3)
    default: return nullptr;
  }
#undef XH_SLICED_CASE
}

// ------------------------------------------------------------------------------------------
// inputs of different dtypes / integer weights, consumed as float64 (hist_fast<..., MIXED = true>): LDS histograms,
// binary search, <= 2 edges per bucket, or arithmetic edges
// (raw and converted copies of a tile are both live for a moment: two vectors per lane and input, one for three inputs)
constexpr int mixed_unroll(int D) { return D >= 3 ? 1 : 2; }

template <typename WT>
static kernel_fn mixed_pick_ds(int D, int scan) {
#define XH_MIXED(DD, SS) (kernel_fn)hist_fast<double, WT, DD, 4, mixed_unroll(DD), kHistLds, SS, false, false, false, true>
#define XH_MIXED_CASE(DD)                                    \
  case DD:                                                   \
    if (scan == 0) return XH_MIXED(DD, 0);                   \
    if (scan == 1) return XH_MIXED(DD, 1);                   \
    if (scan == 2) return XH_MIXED(DD, 2);                   \
    if (scan == kScanArith) {                                \
      /* (one unweighted input is never a "mixture": no such call reaches the arithmetic form — census of round 6) */ \
      if constexpr (DD > 1 || !std::is_same<WT, NoWeight>::value) return XH_MIXED(DD, kScanArith); \
      else return nullptr;                                   \
    }                                                        \
    return nullptr;
  switch (D) {
    XH_MIXED_CASE(1)
    XH_MIXED_CASE(2)
    XH_MIXED_CASE(3)
    default: return nullptr;
  }
#undef XH_MIXED_CASE
#undef XH_MIXED
}

// ------------------------------------------------------------------------------------------
// one-pass routing of the partitioned mode (xhist_route.hip.h): binary search, <= 2 edges per bucket, or
// arithmetic edges; up to three inputs; any of the three weight kinds
constexpr int kWdtPacked48 = 0x100 | XHIST_F64;  // float64 weights, packed 8-byte records (xhist_route.hip.h)

// Long tiles (8 samples per lane) exist only where route_geom_for (xhist_exec_device.hip.h) can pick them: the tile's samples
// and weights — 2 x (bytes of one sample of every input + bytes of its weight) registers — fit next to the sort's state
// (32 registers with the arithmetic digitize, 24 with table lookups), and never float64 samples with float64 weights.
// ONE rule for the host's choice and for what is instantiated: 504 routing kernels became 239 in round 5 (the 512-thread
// variants, reachable only through an A/B override and slower everywhere since round 3, went as well).
constexpr bool route_long_tile_ok(int sample_bytes, int weight_bytes, int D, bool arith) {
  return 2 * (D * sample_bytes + weight_bytes) <= (arith ? 32 : 24) && !(sample_bytes == 8 && weight_bytes == 8);
}
template <typename ST, typename WT, int D, int SCAN, int SPL>
constexpr bool route_variant_exists() {
  constexpr int wb = std::is_same<WT, NoWeight>::value ? 0 : std::is_same<WT, float>::value ? 4 : 8;
  return SPL == 4 || route_long_tile_ok((int)sizeof(ST), wb, D, SCAN == kScanArith);
}
// one input with a table digitize: only float32 thresholds of a weighted histogram fit LDS next to the sort buffers — binary search
// or two edges per bucket, the short tile, one row per pass (the rules at the top of this file; census of round 6)
template <typename ST, typename WT, int D, int SCAN, bool MULTI, int SPL>
constexpr bool route_one_input_ok() {
  return D > 1 || SCAN == kScanArith ||
         (std::is_same<ST, float>::value && !std::is_same<WT, NoWeight>::value && (SCAN == 0 || SCAN == 2) && SPL == 4 && !MULTI);
}
template <typename ST, typename WT, int D, int SCAN, bool MULTI, int BLOCK, int SPL>
static kernel_fn_route route_variant() {
  if constexpr (route_variant_exists<ST, WT, D, SCAN, SPL>() && route_one_input_ok<ST, WT, D, SCAN, MULTI, SPL>())
    return (kernel_fn_route)part_route<ST, WT, D, SCAN, MULTI, BLOCK, SPL>;
  else return nullptr;
}

// (several rows per pass: uniform-style edges only — tables with one edge per bucket, or arithmetic — the shapes a census over
// time steps has; other edges run one row per pass)
template <typename ST, typename WT, int BLOCK, int SPL = 4>
static kernel_fn_route route_pick_ds(int D, int scan, bool multi) {
#define XH_ROUTE_CASE(DD)                                                        \
  case DD:                                                                       \
    if (multi) {                                                                 \
      if (scan == 1) return route_variant<ST, WT, DD, 1, true, BLOCK, SPL>();    \
      if (scan == kScanArith) return route_variant<ST, WT, DD, kScanArith, true, BLOCK, SPL>(); \
      return nullptr;                                                            \
    }                                                                            \
    if (scan == 0) return route_variant<ST, WT, DD, 0, false, BLOCK, SPL>();            \
    if (scan == 1) return route_variant<ST, WT, DD, 1, false, BLOCK, SPL>();            \
    if (scan == 2) return route_variant<ST, WT, DD, 2, false, BLOCK, SPL>();            \
    if (scan == kScanArith) return route_variant<ST, WT, DD, kScanArith, false, BLOCK, SPL>(); \
    if (scan == kScanPackG) return route_variant<ST, WT, DD, kScanPackG, false, BLOCK, SPL>(); \
    return nullptr;
  switch (D) {
    XH_ROUTE_CASE(1)
    XH_ROUTE_CASE(2)
    XH_ROUTE_CASE(3)
    default: return nullptr;
  }
#undef XH_ROUTE_CASE
}

template <typename ST, int BLOCK, int SPL = 4>
static kernel_fn_route route_pick(int wdt, int D, int scan, bool multi) {
  if (wdt == -1) return route_pick_ds<ST, NoWeight, BLOCK, SPL>(D, scan, multi);
  if (wdt == XHIST_F64) return route_pick_ds<ST, double, BLOCK, SPL>(D, scan, multi);
  if (wdt == XHIST_F32) return route_pick_ds<ST, float, BLOCK, SPL>(D, scan, multi);
  if (wdt == kWdtPacked48) return route_pick_ds<ST, Packed48, BLOCK, SPL>(D, scan, multi);
  return nullptr;
}

// ------------------------------------------------------------------------------------------
// what the two picker translation units export (sample type fixed, everything else a run-time choice);
// nullptr = no such kernel
kernel_fn xhist_pick_f64(int wdt, int D, int scan, int hist);
kernel_fn xhist_pick_f32(int wdt, int D, int scan, int hist);
kernel_fn xhist_pick_f64_long(int scan);  // hist_fast<double, NoWeight, 1, 2, 8, kHistLds, scan>
kernel_fn xhist_pick_f32_long(int scan);  // hist_fast<float, NoWeight, 1, 4, 8, kHistLds, scan>
kernel_fn xhist_pick_sliced_f64(int wdt, int D, int scan, int hist);
kernel_fn xhist_pick_sliced_f32(int wdt, int D, int scan, int hist);
kernel_fn xhist_pick_mixed(bool weighted, int D, int scan);  // (xhist_pick_mixed.hip)
typedef void (*kernel_fn_flat)(const Params, int32_t, int32_t, int32_t, uint64_t, int64_t);
kernel_fn_flat xhist_pick_flat_rows(int sdt, int wdt, int D, int scan);  // hist_flat_rows (xhist_pick_flat.hip); nullptr: no such variant
// (xhist_route_{f64,f32}_b1024{,s8}.hip: one translation unit per sample type and tile length)
#define XH_ROUTE_TU(ST, B) kernel_fn_route xhist_pick_route_##ST##_b##B(int wdt, int D, int scan, bool multi);
XH_ROUTE_TU(f64, 1024) XH_ROUTE_TU(f64, 1024s8)
XH_ROUTE_TU(f32, 1024) XH_ROUTE_TU(f32, 1024s8)
#undef XH_ROUTE_TU

// the exchange mode of the partitioned path (xhist_exchange.hip.h; translation unit xhist_exchange.hip): float64 samples,
// float64 weights as packed records, arithmetic edges, 1-3 inputs
typedef void (*kernel_fn_exch)(const ExchArgs);
kernel_fn_exch xhist_pick_exchange(int D, bool exact);  // exact: full float64 records (12 bytes through two rings)
kernel_fn_exch xhist_pick_exchange_probe(int D);
typedef void (*kernel_fn_exch_pick)(const ExchArgs);
typedef void (*kernel_fn_exch_merge)(const ExchArgs, double*, int64_t);
kernel_fn_exch_pick xhist_pick_exchange_pick();
kernel_fn_exch_merge xhist_pick_exchange_merge();
