// xhist_meanvar.hip — per-bin count, mean and variance (histogram_mean_var): the kernels of xhist_meanvar.hip.h, instantiated
// here and nowhere else, the steps between and after the two passes, and the driver that orders their launches (the choice
// and the binning launches themselves: xhist_values.hip.h).
//
// Instantiations (36 binning kernels + 2):
//   mv_sum_fast<ST, D, SCAN>, mv_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mv_sum_generic<CMP, LDS>, mv_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   mv_mean, mv_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

using namespace xhist;

namespace xhist {

// the sums of pass 1 -> means, in place: S / n, NaN where no value arrived
__global__ void __launch_bounds__(256) mv_mean(const unsigned long long* cnt, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    sum[i] = c ? sum[i] / (double)c : nan;
  }
}

// the sums of pass 2 -> M2 = max(0, sum(d*d) - sum(d)^2 / n), in place; NaN where no value arrived, and NaN stays NaN
__global__ void __launch_bounds__(256) mv_finalize(const unsigned long long* cnt, const double* sd, double* m2, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    if (!c) {
      m2[i] = nan;
      continue;
    }
    const double s = sd[i];
    const double r = m2[i] - s * s / (double)c;
    m2[i] = r <= 0.0 ? 0.0 : r;
  }
}

}  // namespace xhist

// the binning kernels of each pass, for pick_values_kernel
struct MvSumKernels {
  template <typename ST, int D, int SCAN>
  static values_fn fast() { return mv_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_fn generic() { return mv_sum_generic<CMP, LDS>; }
};
struct MvDevKernels {
  template <typename ST, int D, int SCAN>
  static values_fn fast() { return mv_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_fn generic() { return mv_dev_generic<CMP, LDS>; }
};

// pass 1's count and sum, pass 2's mean and two sums, whatever the type of the values; pass 2's slot decides for both
static constexpr ValuesSlots kMeanVarSlots = {{sizeof(MvSumSlot), sizeof(MvDevSlot)}, {sizeof(MvSumSlot), sizeof(MvDevSlot)}, true};

int xhist_meanvar_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      int64_t* out_count, double* out_mean, double* out_m2, double* sd, hipStream_t stream, char* err, size_t err_cap,
                      char* desc, size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out_count);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  unsigned long long* zero[4] = {cnt, reinterpret_cast<unsigned long long*>(out_mean), reinterpret_cast<unsigned long long*>(out_m2),
                                 reinterpret_cast<unsigned long long*>(sd)};
  for (unsigned long long* z : zero) {
    hipLaunchKernelGGL(zero_words, dim3(grid_io), dim3(256), 0, stream, z, n_out);
    XH_VALUES_LAUNCH_CHECK("mean_var zeroing launch");
  }

  ValuesChoice c;
  ValuesGeometry g;
  values_fn sum = nullptr, dev = nullptr;
  if (n_cols > 0) {
    c = choose_values(pl, kMeanVarSlots, samples, values, n_cols);
    sum = pick_values_kernel<MvSumKernels>(c, pl);
    dev = pick_values_kernel<MvDevKernels>(c, pl);
    if (!sum || !dev) {
      snprintf(err, err_cap, "internal: no mean_var kernel for this combination");
      return XHIST_ERR_HIP;
    }
    for (int k = 0; k < 2; ++k)
      if (int rc = allow_values_lds(k ? dev : sum, c.lds_bytes[k], "mean_var: setting the dynamic LDS size failed", err, err_cap)) return rc;
    g = values_geometry(pl, c, n_rows, n_cols);
    if (int rc = launch_values_pass(sum, c.lds_bytes[0], "mv_sum launch", pl, c, g, samples, values, n_rows, n_cols, cnt, out_mean, nullptr,
                                    stream, err, err_cap))
      return rc;
  }
  XH_VALUES_LAUNCH(mv_mean, dim3(grid_io), dim3(256), 0, stream, cnt, out_mean, n_out);
  XH_VALUES_LAUNCH_CHECK("mv_mean launch");
  if (n_cols > 0) {
    if (int rc = launch_values_pass(dev, c.lds_bytes[1], "mv_dev launch", pl, c, g, samples, values, n_rows, n_cols, sd, out_m2, out_mean,
                                    stream, err, err_cap))
      return rc;
  }
  XH_VALUES_LAUNCH(mv_finalize, dim3(grid_io), dim3(256), 0, stream, cnt, sd, out_m2, n_out);
  XH_VALUES_LAUNCH_CHECK("mv_finalize launch");
  if (desc && desc_cap) {
    const char* fam = !sum ? "none" : c.fast ? "fast" : "generic";
    const char* home = !sum ? "none" : c.lds ? "lds" : "global";
    snprintf(desc, desc_cap,
             "mean_var pass1=mv_sum_%s slots=%s pass2=mv_dev_%s slots=%s scan=%d copies=%d block=%d segs=%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d cmp=%d",
             fam, home, fam, home, c.scan, 1 << c.copies_log2, g.block, (long long)g.segs, c.lds_bytes[0], c.lds_bytes[1],
             (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  return XHIST_OK;
}
