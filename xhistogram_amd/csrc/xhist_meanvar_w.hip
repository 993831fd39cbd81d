// xhist_meanvar_w.hip — per-bin sum of weights, weighted mean and variance (histogram_mean_var with weights): the weighted
// kernels of xhist_meanvar.hip.h and the steps between and after the two passes (xhist_moments.hip.h), instantiated here and
// nowhere else, and what the driver needs of this form: the driver itself is two_pass_run of xhist_values.hip.h, shared with the
// unweighted form and the covariance (as are the choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   mvw_sum_fast<ST, D, SCAN>, mvw_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mvw_sum_generic<CMP, LDS>, mvw_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   moments_mean<1, double>, moments_finalize<1, double>                                                                2
// and, for the weighted histogram_skew_kurt, whose pass 1 and means are the ones above (18 binning kernels + 1):
//   skw_dev_fast<ST, D, SCAN>                               ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith         12
//   skw_dev_generic<CMP, LDS>                               CMP 0 / 1 / 3, slots in LDS or sums in global memory         6
//   moments_finalize4<double>                                                                                           1
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

using namespace xhist;

typedef void (*values_w_fn)(const WParams);

// the binning kernels of each weighted pass, for pick_values_kernel
struct MvwSumKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return mvw_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return mvw_sum_generic<CMP, LDS>; }
};
struct MvwDevKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return mvw_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return mvw_dev_generic<CMP, LDS>; }
};

// what the shared driver (two_pass_run, xhist_values.hip.h) needs of this form
struct MeanVarW {
  using Sum = MvwSumKernels;
  using Dev = MvwDevKernels;
  static constexpr auto mean = moments_mean<1, double>;
  static constexpr auto finalize = moments_finalize<1, double>;
  static constexpr ValuesSlots slots = moment_slots<1, true>();
  static constexpr int planes[4] = {1, 1, 1, 1};
  static constexpr const char *name = "mean_var_w", *prefix = "mvw", *spelled = "weighted mean_var";
};

int xhist_meanvar_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<MeanVarW>(k, static_cast<double*>(out_first), out_mean, out_m2);
}

// ---- the weighted histogram_skew_kurt: the weighted mean_var's pass 1, then the four sums of pass 2 ----------------------------
typedef void (*skw_fn)(const CovParams);

struct SkwDevKernels {
  template <typename ST, int D, int SCAN>
  static skw_fn fast() { return skw_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static skw_fn generic() { return skw_dev_generic<CMP, LDS>; }
};

struct SkewKurtW {
  using Sum = MvwSumKernels;
  using Dev = SkwDevKernels;
  static constexpr auto mean = moments_mean<1, double>;
  static constexpr auto finalize = moments_finalize4<double>;
  static constexpr ValuesSlots slots = moment4_slots<true>();
  static constexpr int planes[4] = {1, 1, 3, 1};  // W; mean; M2, M3, M4; D
  static constexpr const char *name = "skew_kurt_w", *prefix = "skw", *sum_prefix = "mvw", *spelled = "weighted skew_kurt";
};

int xhist_skew_kurt_w_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<SkewKurtW>(k, static_cast<double*>(out_first), out_mean, out_m2);
}
