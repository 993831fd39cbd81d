// xhist_meanvar_w.hip — per-bin sum of weights, weighted mean and variance (histogram_mean_var with weights): the weighted
// kernels of xhist_meanvar.hip.h, instantiated here and nowhere else, the steps between and after the two passes, and what the
// driver needs of this form: the driver itself is two_pass_run of xhist_values.hip.h, shared with the unweighted form and the
// covariance (as are the choice and the binning launches themselves).
//
// Instantiations (36 binning kernels + 2):
//   mvw_sum_fast<ST, D, SCAN>, mvw_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mvw_sum_generic<CMP, LDS>, mvw_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   mvw_mean, mvw_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

using namespace xhist;

namespace xhist {

// the weighted sums of pass 1 -> means, in place: S / W, NaN where W == 0 (a NaN W gives NaN)
__global__ void __launch_bounds__(256) mvw_mean(const double* wsum, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    sum[i] = w != 0.0 ? sum[i] / w : nan;
  }
}

// the sums of pass 2 -> M2 = max(0, sum(w*d*d) - sum(w*d)^2 / W), in place; NaN where W == 0, and NaN stays NaN
__global__ void __launch_bounds__(256) mvw_finalize(const double* wsum, const double* sd, double* m2, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    if (w == 0.0) {
      m2[i] = nan;
      continue;
    }
    const double s = sd[i];
    const double r = m2[i] - s * s / w;
    m2[i] = r <= 0.0 ? 0.0 : r;
  }
}

}  // namespace xhist

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
  static constexpr auto mean = mvw_mean;
  static constexpr auto finalize = mvw_finalize;
  // pass 1's sums of weights and of w*v, pass 2's mean and two sums: the slot sizes of the unweighted passes, so the same choice
  static constexpr ValuesSlots slots = {{sizeof(MvwSumSlot), sizeof(MvDevSlot)}, {sizeof(MvwSumSlot), sizeof(MvDevSlot)}, true};
  static constexpr int planes[4] = {1, 1, 1, 1};
  static constexpr const char *name = "mean_var_w", *prefix = "mvw", *spelled = "weighted mean_var";
  static constexpr const char *lds_what = "mean_var_w: setting the dynamic LDS size failed";
  static constexpr const char *sum_what = "mvw_sum launch", *dev_what = "mvw_dev launch";
};
static_assert(sizeof(MvwSumSlot) == sizeof(MvSumSlot), "the weighted pass 1 keeps the slot size of the unweighted one");

int xhist_meanvar_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, const xhist_array* weights,
                        int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_m2, double* sd, hipStream_t stream,
                        char* err, size_t err_cap, char* desc, size_t desc_cap) {
  return two_pass_run<MeanVarW>(pl, samples, values, weights, n_rows, n_cols, out_wsum, out_mean, out_m2, sd, stream, err, err_cap, desc,
                                desc_cap);
}
