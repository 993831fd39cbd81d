// xhist_cov.hip — per-bin count, means, variances and covariance of two value arrays (histogram_cov): the kernels of
// xhist_cov.hip.h and the steps between and after the two passes (xhist_moments.hip.h), instantiated here and nowhere else, and
// what the driver needs of this statistic: the driver itself is two_pass_run of xhist_values.hip.h, shared with
// histogram_mean_var and its weighted form (as are the choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   cov_sum_fast<ST, D, SCAN>, cov_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   cov_sum_generic<CMP, LDS>, cov_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   moments_mean<2, unsigned long long>, moments_finalize<2, unsigned long long>                                        2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_cov.hip.h"

using namespace xhist;

typedef void (*cov_fn)(const CovParams);

// the binning kernels of each pass, for pick_values_kernel
struct CovSumKernels {
  template <typename ST, int D, int SCAN>
  static cov_fn fast() { return cov_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_fn generic() { return cov_sum_generic<CMP, LDS>; }
};
struct CovDevKernels {
  template <typename ST, int D, int SCAN>
  static cov_fn fast() { return cov_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_fn generic() { return cov_dev_generic<CMP, LDS>; }
};

// what the shared driver (two_pass_run, xhist_values.hip.h) needs of this statistic: the second value array travels in the
// place of the weights, and the outputs are blocks of several planes
struct Cov {
  using Sum = CovSumKernels;
  using Dev = CovDevKernels;
  static constexpr auto mean = moments_mean<2, unsigned long long>;
  static constexpr auto finalize = moments_finalize<2, unsigned long long>;
  static constexpr ValuesSlots slots = moment_slots<2, false>();
  static constexpr int planes[4] = {1, 2, 3, 2};  // the count; mean_a, mean_b; M2_a, C_ab, M2_b; the sums of da and db
  static constexpr const char *name = "cov", *prefix = "cov", *spelled = "cov";
};

int xhist_cov_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<Cov>(k, static_cast<unsigned long long*>(out_first), out_mean, out_m2);
}
