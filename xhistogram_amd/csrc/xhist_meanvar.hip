// xhist_meanvar.hip — per-bin count, mean and variance (histogram_mean_var): the kernels of xhist_meanvar.hip.h and the steps
// between and after the two passes (xhist_moments.hip.h), instantiated here and nowhere else, and what the driver needs of this
// form: the driver itself is two_pass_run of xhist_values.hip.h, shared with the weighted form and the covariance (as are the
// choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   mv_sum_fast<ST, D, SCAN>, mv_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mv_sum_generic<CMP, LDS>, mv_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   moments_mean<1, unsigned long long>, moments_finalize<1, unsigned long long>                                      2
// and, for histogram_skew_kurt, whose pass 1 and means are the ones above (18 binning kernels + 1):
//   sk_dev_fast<ST, D, SCAN>                              ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith         12
//   sk_dev_generic<CMP, LDS>                              CMP 0 / 1 / 3, slots in LDS or sums in global memory         6
//   moments_finalize4<unsigned long long>                                                                             1
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

using namespace xhist;

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

// what the shared driver (two_pass_run, xhist_values.hip.h) needs of this form
struct MeanVar {
  using Sum = MvSumKernels;
  using Dev = MvDevKernels;
  static constexpr auto mean = moments_mean<1, unsigned long long>;
  static constexpr auto finalize = moments_finalize<1, unsigned long long>;
  static constexpr ValuesSlots slots = moment_slots<1, false>();
  static constexpr int planes[4] = {1, 1, 1, 1};
  static constexpr const char *name = "mean_var", *prefix = "mv", *spelled = "mean_var";
};

int xhist_meanvar_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<MeanVar>(k, static_cast<unsigned long long*>(out_first), out_mean, out_m2);
}

// ---- histogram_skew_kurt: mean_var's pass 1, then the four sums of pass 2 ------------------------------------------------------
typedef void (*sk_fn)(const CovParams);

struct SkDevKernels {
  template <typename ST, int D, int SCAN>
  static sk_fn fast() { return sk_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static sk_fn generic() { return sk_dev_generic<CMP, LDS>; }
};

struct SkewKurt {
  using Sum = MvSumKernels;
  using Dev = SkDevKernels;
  static constexpr auto mean = moments_mean<1, unsigned long long>;
  static constexpr auto finalize = moments_finalize4<unsigned long long>;
  static constexpr ValuesSlots slots = moment4_slots<false>();
  static constexpr int planes[4] = {1, 1, 3, 1};  // n; mean; M2, M3, M4; D
  static constexpr const char *name = "skew_kurt", *prefix = "sk", *sum_prefix = "mv", *spelled = "skew_kurt";
};

int xhist_skew_kurt_run(const ValuesCall& k, void* out_first, double* out_mean, double* out_m2) {
  return two_pass_run<SkewKurt>(k, static_cast<unsigned long long*>(out_first), out_mean, out_m2);
}
