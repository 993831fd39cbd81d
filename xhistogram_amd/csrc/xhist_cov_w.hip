// xhist_cov_w.hip — per-bin sum of weights, weighted means, variances and covariance of two value arrays
// (histogram_weighted_cov): the kernels of xhist_cov_w.hip.h, instantiated here and nowhere else, the steps between and after
// the two passes, and what the driver needs of this statistic: the driver itself is two_pass_run of xhist_values.hip.h, shared
// with histogram_mean_var, its weighted form and histogram_cov (as are the choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   covw_sum_fast<ST, D, SCAN>, covw_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith   12 + 12
//   covw_sum_generic<CMP, LDS>, covw_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory     6 + 6
//   covw_mean, covw_finalize                                                                                            2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_cov_w.hip.h"

using namespace xhist;

namespace xhist {

// the weighted sums of pass 1 -> both means, in place: S / W, NaN where W == 0 (a NaN W gives NaN); `sum` is [2, n]
__global__ void __launch_bounds__(256) covw_mean(const double* wsum, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    sum[i] = w != 0.0 ? sum[i] / w : nan;
    sum[n + i] = w != 0.0 ? sum[n + i] / w : nan;
  }
}

// the sums of pass 2 -> M2_a, C_ab, M2_b, in place in `co` [3, n]; `sd` is [2, n].  The M2 are clamped at 0, the co-moment is
// not; NaN where W == 0, and NaN stays NaN
__global__ void __launch_bounds__(256) covw_finalize(const double* wsum, const double* sd, double* co, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    if (w == 0.0) {
      co[i] = co[n + i] = co[2 * n + i] = nan;
      continue;
    }
    const double sa = sd[i], sb = sd[n + i];
    const double ra = co[i] - sa * sa / w;
    const double rb = co[2 * n + i] - sb * sb / w;
    co[i] = ra <= 0.0 ? 0.0 : ra;
    co[n + i] = co[n + i] - sa * sb / w;
    co[2 * n + i] = rb <= 0.0 ? 0.0 : rb;
  }
}

}  // namespace xhist

typedef void (*cov_w_fn)(const CovWParams);

// the binning kernels of each pass, for pick_values_kernel
struct CovWSumKernels {
  template <typename ST, int D, int SCAN>
  static cov_w_fn fast() { return covw_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_w_fn generic() { return covw_sum_generic<CMP, LDS>; }
};
struct CovWDevKernels {
  template <typename ST, int D, int SCAN>
  static cov_w_fn fast() { return covw_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_w_fn generic() { return covw_dev_generic<CMP, LDS>; }
};

// what the shared driver (two_pass_run, xhist_values.hip.h) needs of this statistic: the second value array travels in the
// place of the weights, the weights as the fourth stream, and the outputs are blocks of several planes
struct CovW {
  using Sum = CovWSumKernels;
  using Dev = CovWDevKernels;
  static constexpr auto mean = covw_mean;
  static constexpr auto finalize = covw_finalize;
  // the slot sizes of histogram_cov's passes, so the same choice
  static constexpr ValuesSlots slots = {{sizeof(CovWSumSlot), sizeof(CovDevSlot)}, {sizeof(CovWSumSlot), sizeof(CovDevSlot)}, true};
  static constexpr int planes[4] = {1, 2, 3, 2};  // W; mean_a, mean_b; M2_a, C_ab, M2_b; the sums of w*da and w*db
  static constexpr const char *name = "cov_w", *prefix = "covw", *spelled = "weighted cov";
  static constexpr const char *lds_what = "cov_w: setting the dynamic LDS size failed";
  static constexpr const char *sum_what = "covw_sum launch", *dev_what = "covw_dev launch";
};

int xhist_cov_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                    const xhist_array* weights, int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_comoment,
                    double* sd, hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap) {
  return two_pass_run<CovW>(pl, samples, values_a, values_b, n_rows, n_cols, out_wsum, out_mean, out_comoment, sd, stream, err, err_cap,
                            desc, desc_cap, weights);
}
