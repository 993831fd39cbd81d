// xhist_extrema.hip — per-bin minimum and maximum (histogram_extrema): the kernels of xhist_extrema.hip.h, instantiated here and
// nowhere else, the key conversions before and after them, and the driver that orders their launches (the choice and the
// launches themselves: xhist_values.hip.h).
//
// Instantiations (18 binning kernels + 2):
//   extrema_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith          12
//   extrema_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or in global memory                6
//   extrema_prepare, extrema_finalize                                                          2
// and, for histogram_argextrema's second pass (18 + 2; its first pass is the kernels above):
//   argext_fast<ST, D, SCAN>     as extrema_fast                                               12
//   argext_generic<CMP, LDS>     as extrema_generic                                             6
//   argext_prepare, argext_finalize                                                            2
#include "xhist_extrema.hip.h"

using namespace xhist;

namespace xhist {

// The output's doubles -> keys, in place: fresh (the empty markers) or accumulating (NaN = empty, as the result reads).
__global__ void __launch_bounds__(256) extrema_prepare(uint64_t* kmin, uint64_t* kmax, int64_t n, int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!accumulate) {
      kmin[i] = kEmptyMin64;
      kmax[i] = kEmptyMax64;
      continue;
    }
    const double lo = __builtin_bit_cast(double, kmin[i]), hi = __builtin_bit_cast(double, kmax[i]);
    kmin[i] = lo == lo ? extrema_key64(lo) : kEmptyMin64;
    kmax[i] = hi == hi ? extrema_key64(hi) : kEmptyMax64;
  }
}

// ... and back: keys -> doubles, the markers -> NaN
__global__ void __launch_bounds__(256) extrema_finalize(uint64_t* kmin, uint64_t* kmax, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = kmin[i], hi = kmax[i];
    reinterpret_cast<double*>(kmin)[i] = lo == kEmptyMin64 ? nan : extrema_value64(lo);
    reinterpret_cast<double*>(kmax)[i] = hi == kEmptyMax64 ? nan : extrema_value64(hi);
  }
}

// histogram_argextrema: the positions' two planes before pass 2 — no position yet
__global__ void __launch_bounds__(256) argext_prepare(uint64_t* index, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) index[i] = kNoPosition;
}

// ... and after it: the keys of both planes -> doubles, the markers -> NaN; "no position" -> -1
__global__ void __launch_bounds__(256) argext_finalize(uint64_t* kmin, uint64_t* kmax, uint64_t* index, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = kmin[i], hi = kmax[i];
    reinterpret_cast<double*>(kmin)[i] = lo == kEmptyMin64 ? nan : extrema_value64(lo);
    reinterpret_cast<double*>(kmax)[i] = hi == kEmptyMax64 ? nan : extrema_value64(hi);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint64_t at = index[k * n + i];
      reinterpret_cast<int64_t*>(index)[k * n + i] = at == kNoPosition ? (int64_t)-1 : (int64_t)at;
    }
  }
}

}  // namespace xhist

// the binning kernels, for pick_values_kernel
struct ExtremaKernels {
  template <typename ST, int D, int SCAN>
  static values_fn fast() { return extrema_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_fn generic() { return extrema_generic<CMP, LDS>; }
};

// a bin's minimum and maximum keys, in the one pass
static constexpr ValuesSlots kExtremaSlots = {{16, 0}, {8, 0}, false};

int xhist_extrema_run(const ValuesCall& k, double* out_min, double* out_max, int accumulate) {
  const ValuesPlan& pl = k.pl;
  const int64_t n_out = k.n_rows * pl.n_bins;
  uint64_t* kmin = reinterpret_cast<uint64_t*>(out_min);
  uint64_t* kmax = reinterpret_cast<uint64_t*>(out_max);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_VALUES_LAUNCH(extrema_prepare, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, n_out, accumulate);
  XH_VALUES_LAUNCH_CHECK(k, "extrema_prepare launch");

  if (k.n_cols > 0) {
    const ValuesChoice c = choose_values(k, kExtremaSlots);
    const values_fn fn = pick_values_kernel<ExtremaKernels>(c, pl);
    if (!fn) return k.fail(XHIST_ERR_HIP, "internal: no extrema kernel for this combination");
    if (int rc = allow_values_lds(k, fn, c.lds_bytes[0], "extrema: setting the dynamic LDS size failed")) return rc;
    const ValuesGeometry g = values_geometry(pl, c, k.n_rows, k.n_cols);
    if (int rc = launch_values_pass(fn, c.lds_bytes[0], "extrema launch", k, c, g, kmin, kmax, nullptr)) return rc;
    k.describe("extrema family=%s slots=%s scan=%d block=%d segs=%lld lds_bytes=%zu tables_in_lds=%d D=%d cmp=%d",
               c.fast ? "fast" : "generic", c.lds ? "lds" : "global", c.scan, g.block, (long long)g.segs, c.lds_bytes[0],
               (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  XH_VALUES_LAUNCH(extrema_finalize, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, n_out);
  XH_VALUES_LAUNCH_CHECK(k, "extrema_finalize launch");
  return XHIST_OK;
}

// Pass 1 of a statistic of another unit that starts from a bin's extremes (histogram_sum, xhist_sum.hip): extrema_prepare and
// the binning kernel of the choice `c` that the statistic's larger pass made.  The residency, hence the segments per row
// (*segs), is this pass's own: its slots as histogram_extrema keeps them, one copy (*lds_bytes).
int xhist_extrema_pass1(const ValuesCall& k, const ValuesChoice& c, uint64_t* kmin, uint64_t* kmax, int64_t* segs, size_t* lds_bytes) {
  const ValuesPlan& pl = k.pl;
  const int64_t n_out = k.n_rows * pl.n_bins;
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_VALUES_LAUNCH(extrema_prepare, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, n_out, 0);
  XH_VALUES_LAUNCH_CHECK(k, "extrema_prepare launch");
  *segs = 0;
  *lds_bytes = 0;
  if (k.n_cols <= 0) return XHIST_OK;
  ValuesChoice c1 = c;
  if (c.lds_bytes[0]) {
    const size_t own = (size_t)pl.n_bins * (c.fast && c.f32 ? kExtremaSlots.fast32[0] : kExtremaSlots.bytes[0]);
    if (c.lds) c1.lds_bytes[0] = c.lds_bytes[0] - (own << c.copies_log2) + own;  // (the tables, and one copy of the slots)
  }
  c1.lds_bytes[1] = 0;
  c1.copies_log2 = 0;
  const values_fn fn = pick_values_kernel<ExtremaKernels>(c1, pl);
  if (!fn) return k.fail(XHIST_ERR_HIP, "internal: no extrema kernel for this combination");
  if (int rc = allow_values_lds(k, fn, c1.lds_bytes[0], "extrema: setting the dynamic LDS size failed")) return rc;
  const ValuesGeometry g1 = values_geometry(pl, c1, k.n_rows, k.n_cols);
  *segs = g1.segs;
  *lds_bytes = c1.lds_bytes[0];
  return launch_values_pass(fn, c1.lds_bytes[0], "extrema launch", k, c1, g1, kmin, kmax, nullptr);
}

// pass 2 of histogram_argextrema
struct ArgextKernels {
  template <typename ST, int D, int SCAN>
  static auto fast() -> void (*)(const CovParams) { return argext_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static auto generic() -> void (*)(const CovParams) { return argext_generic<CMP, LDS>; }
};

// pass 1: a bin's two keys; pass 2: the keys and the two positions.  The larger pass decides family and home for both, so
// between the 16- and the 32-byte LDS capacity pass 1 runs where pass 2 must, not where histogram_extrema alone would.
static constexpr ValuesSlots kArgextremaSlots = {{16, 32}, {8, 24}, false};

int xhist_argextrema_run(const ValuesCall& k, double* out_values, int64_t* out_index) {
  const ValuesPlan& pl = k.pl;
  const int64_t n_out = k.n_rows * pl.n_bins;
  uint64_t* kmin = reinterpret_cast<uint64_t*>(out_values);
  uint64_t* kmax = kmin + n_out;
  uint64_t* index = reinterpret_cast<uint64_t*>(out_index);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_VALUES_LAUNCH(extrema_prepare, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, n_out, 0);
  XH_VALUES_LAUNCH_CHECK(k, "extrema_prepare launch");
  XH_VALUES_LAUNCH(argext_prepare, dim3(grid_io), dim3(256), 0, k.stream, index, 2 * n_out);
  XH_VALUES_LAUNCH_CHECK(k, "argext_prepare launch");

  if (k.n_cols > 0) {
    const ValuesChoice c = choose_values(k, kArgextremaSlots);
    const values_fn pass1 = pick_values_kernel<ExtremaKernels>(c, pl);
    const auto pass2 = pick_values_kernel<ArgextKernels>(c, pl);
    if (!pass1 || !pass2) return k.fail(XHIST_ERR_HIP, "internal: no argextrema kernel for this combination");
    const char* lds_what = "argextrema: setting the dynamic LDS size failed";
    if (int rc = allow_values_lds(k, pass1, c.lds_bytes[0], lds_what)) return rc;
    if (int rc = allow_values_lds(k, pass2, c.lds_bytes[1], lds_what)) return rc;
    // Family and home are the larger pass's; the residency, hence the segments per row, is each pass's own.  Neither result
    // depends on it, and pass 1's slots are half of pass 2's: with 50 x 50 bins it keeps three workgroups on a CU where pass
    // 2 keeps one, and runs as fast as histogram_extrema alone (0.77 ms against 0.89 ms for 2e8 float64 pairs).
    ValuesChoice c1 = c;
    c1.lds_bytes[1] = 0;
    const ValuesGeometry g1 = values_geometry(pl, c1, k.n_rows, k.n_cols), g = values_geometry(pl, c, k.n_rows, k.n_cols);
    if (int rc = launch_values_pass(pass1, c.lds_bytes[0], "extrema launch", k, c, g1, kmin, kmax, nullptr)) return rc;
    if (int rc = launch_values_pass(pass2, c.lds_bytes[1], "argext launch", k, c, g, index, index + n_out, kmin)) return rc;
    const char* fam = c.fast ? "fast" : "generic";
    const char* home = c.lds ? "lds" : "global";
    k.describe("argextrema pass1=extrema_%s slots=%s pass2=argext_%s slots=%s scan=%d block=%d segs=%lld/%lld lds_bytes=%zu/%zu "
               "tables_in_lds=%d D=%d cmp=%d",
               fam, home, fam, home, c.scan, g.block, (long long)g1.segs, (long long)g.segs, c.lds_bytes[0], c.lds_bytes[1],
               (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  XH_VALUES_LAUNCH(argext_finalize, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, index, n_out);
  XH_VALUES_LAUNCH_CHECK(k, "argext_finalize launch");
  return XHIST_OK;
}
