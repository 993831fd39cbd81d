// xhist_extrema.hip — per-bin minimum and maximum (histogram_extrema): the kernels of xhist_extrema.hip.h, instantiated here and
// nowhere else, the key conversions before and after them, and the driver that orders their launches (the choice and the
// launches themselves: xhist_values.hip.h).
//
// Instantiations (18 binning kernels + 2):
//   extrema_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith          12
//   extrema_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or in global memory                6
//   extrema_prepare, extrema_finalize                                                          2
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

int xhist_extrema_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      double* out_min, double* out_max, int accumulate, hipStream_t stream, char* err, size_t err_cap, char* desc,
                      size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  uint64_t* kmin = reinterpret_cast<uint64_t*>(out_min);
  uint64_t* kmax = reinterpret_cast<uint64_t*>(out_max);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_VALUES_LAUNCH(extrema_prepare, dim3(grid_io), dim3(256), 0, stream, kmin, kmax, n_out, accumulate);
  XH_VALUES_LAUNCH_CHECK("extrema_prepare launch");

  if (n_cols > 0) {
    const ValuesChoice c = choose_values(pl, kExtremaSlots, samples, values, n_cols);
    const values_fn fn = pick_values_kernel<ExtremaKernels>(c, pl);
    if (!fn) {
      snprintf(err, err_cap, "internal: no extrema kernel for this combination");
      return XHIST_ERR_HIP;
    }
    if (int rc = allow_values_lds(fn, c.lds_bytes[0], "extrema: setting the dynamic LDS size failed", err, err_cap)) return rc;
    const ValuesGeometry g = values_geometry(pl, c, n_rows, n_cols);
    if (int rc = launch_values_pass(fn, c.lds_bytes[0], "extrema launch", pl, c, g, samples, values, n_rows, n_cols, kmin, kmax, nullptr,
                                    stream, err, err_cap))
      return rc;
    if (desc && desc_cap)
      snprintf(desc, desc_cap, "extrema family=%s slots=%s scan=%d block=%d segs=%lld lds_bytes=%zu tables_in_lds=%d D=%d cmp=%d",
               c.fast ? "fast" : "generic", c.lds ? "lds" : "global", c.scan, g.block, (long long)g.segs, c.lds_bytes[0],
               (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  XH_VALUES_LAUNCH(extrema_finalize, dim3(grid_io), dim3(256), 0, stream, kmin, kmax, n_out);
  XH_VALUES_LAUNCH_CHECK("extrema_finalize launch");
  return XHIST_OK;
}
