// xhist_cov.hip — per-bin count, means, variances and covariance of two value arrays (histogram_cov): the kernels of
// xhist_cov.hip.h, instantiated here and nowhere else, the steps between and after the two passes, and what the driver needs
// of this statistic: the driver itself is two_pass_run of xhist_values.hip.h, shared with histogram_mean_var and its weighted
// form (as are the choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   cov_sum_fast<ST, D, SCAN>, cov_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   cov_sum_generic<CMP, LDS>, cov_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   cov_mean, cov_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_cov.hip.h"

using namespace xhist;

namespace xhist {

// the sums of pass 1 -> both means, in place: S / n, NaN where no pair arrived; `sum` is [2, n]
__global__ void __launch_bounds__(256) cov_mean(const unsigned long long* cnt, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    sum[i] = c ? sum[i] / (double)c : nan;
    sum[n + i] = c ? sum[n + i] / (double)c : nan;
  }
}

// the sums of pass 2 -> M2_a, C_ab, M2_b, in place in `co` [3, n]; `sd` is [2, n].  The M2 are clamped at 0, the co-moment is
// not; NaN where no pair arrived, and NaN stays NaN
__global__ void __launch_bounds__(256) cov_finalize(const unsigned long long* cnt, const double* sd, double* co, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    if (!c) {
      co[i] = co[n + i] = co[2 * n + i] = nan;
      continue;
    }
    const double sa = sd[i], sb = sd[n + i];
    const double ra = co[i] - sa * sa / (double)c;
    const double rb = co[2 * n + i] - sb * sb / (double)c;
    co[i] = ra <= 0.0 ? 0.0 : ra;
    co[n + i] = co[n + i] - sa * sb / (double)c;
    co[2 * n + i] = rb <= 0.0 ? 0.0 : rb;
  }
}

}  // namespace xhist

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
  static constexpr auto mean = cov_mean;
  static constexpr auto finalize = cov_finalize;
  // pass 1's count and two sums, pass 2's two means and five sums, whatever the type of the values; pass 2's slot decides for both
  static constexpr ValuesSlots slots = {{sizeof(CovSumSlot), sizeof(CovDevSlot)}, {sizeof(CovSumSlot), sizeof(CovDevSlot)}, true};
  static constexpr int planes[4] = {1, 2, 3, 2};  // the count; mean_a, mean_b; M2_a, C_ab, M2_b; the sums of da and db
  static constexpr const char *name = "cov", *prefix = "cov", *spelled = "cov";
  static constexpr const char *lds_what = "cov: setting the dynamic LDS size failed";
  static constexpr const char *sum_what = "cov_sum launch", *dev_what = "cov_dev launch";
};

int xhist_cov_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                  int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_comoment, double* sd,
                  hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap) {
  return two_pass_run<Cov>(pl, samples, values_a, values_b, n_rows, n_cols, reinterpret_cast<unsigned long long*>(out_count), out_mean,
                           out_comoment, sd, stream, err, err_cap, desc, desc_cap);
}
