// xhist_cov.hip.h — per-bin count, means, sums of squared deviations and co-moment of TWO value arrays (histogram_cov): the
// binning kernels (their driver: two_pass_run of xhist_values.hip.h).
//
// Two value arrays (NV = 2), unweighted, of the moments of xhist_moments.hip.h, where the formulas, the slots and the policy
// live.  The second value array travels where the weights of the weighted statistics travel (WParams::x_*), so the skeletons
// hand the policy the pair (a, b).  Pass 1 -> out_count (uint64) and out_mean [2]; pass 2 -> the scratch block of sum(da),
// sum(db) [2] and out_comoment [3] (aa, ab, bb).  Outputs of k planes are [k, n_rows, n_bins] blocks: CovParams::plane is the
// distance of two planes in 8-byte elements, and the kernels take CovParams.
#pragma once

#include "xhist_moments.hip.h"

namespace xhist {

// The binning kernels of the two passes: cov_sum_generic / cov_dev_generic<CMP, LDS> (block 512) and cov_sum_fast /
// cov_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h; instantiated in xhist_cov.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) cov_sum_generic(const CovParams p) {
  values_generic_body<MomentAcc<2, false, 1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) cov_dev_generic(const CovParams p) {
  values_generic_body<MomentAcc<2, false, 2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) cov_sum_fast(const CovParams p) {
  values_fast_body<MomentAcc<2, false, 1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) cov_dev_fast(const CovParams p) {
  values_fast_body<MomentAcc<2, false, 2>, ST, D, SCAN>(p);
}

}  // namespace xhist

// The launches of histogram_cov for DEVICE arrays the caller has validated, n_rows * n_bins > 0, the plan's device current
// (two_pass_run<Cov>, xhist_cov.hip).  out_mean is [2, n_rows, n_bins] (mean_a, mean_b), out_comoment [3, n_rows, n_bins] (M2_a, C_ab, M2_b), `sd`
// a float64 [2, n_rows, n_bins] block of the caller's for the sums of da and db.  Returns XHIST_OK, or an error status with a
// message in `err`; `desc` receives a line about the launches.  (Called by xhist_plan_execute_cov, xhist_capi.hip.)
int xhist_cov_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                  int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_comoment, double* sd,
                  hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap);
