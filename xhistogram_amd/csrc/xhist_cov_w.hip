// xhist_cov_w.hip — per-bin sum of weights, weighted means, variances and covariance of two value arrays
// (histogram_weighted_cov): the kernels of xhist_cov_w.hip.h and the steps between and after the two passes
// (xhist_moments.hip.h), instantiated here and nowhere else, and what the driver needs of this statistic: the driver itself is
// two_pass_run of xhist_values.hip.h, shared with histogram_mean_var, its weighted form and histogram_cov (as are the choice and
// the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   covw_sum_fast<ST, D, SCAN>, covw_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith   12 + 12
//   covw_sum_generic<CMP, LDS>, covw_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory     6 + 6
//   moments_mean<2, double>, moments_finalize<2, double>                                                                2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_cov_w.hip.h"

using namespace xhist;

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
  static constexpr auto mean = moments_mean<2, double>;
  static constexpr auto finalize = moments_finalize<2, double>;
  static constexpr ValuesSlots slots = moment_slots<2, true>();
  static constexpr int planes[4] = {1, 2, 3, 2};  // W; mean_a, mean_b; M2_a, C_ab, M2_b; the sums of w*da and w*db
  static constexpr const char *name = "cov_w", *prefix = "covw", *spelled = "weighted cov";
};

int xhist_cov_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<CovW>(k, static_cast<double*>(out_first), out_mean, out_m2);
}
