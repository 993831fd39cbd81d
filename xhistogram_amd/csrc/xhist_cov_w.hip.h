// xhist_cov_w.hip.h — per-bin sum of weights, weighted means, weighted sums of squared deviations and weighted co-moment of TWO
// value arrays (histogram_weighted_cov): the binning kernels (their driver: two_pass_run of xhist_values.hip.h).
//
// Two value arrays (NV = 2) with frequency weights, of the moments of xhist_moments.hip.h, where the formulas, the slots and
// the policy live.  The second value array travels in WParams::x_* as histogram_cov's does (xhist_cov.hip.h), the weights are a
// fourth stream in CovWParams::y_*, and the skeletons hand the policy the triple (a, b, w).  Pass 1 -> out_wsum (float64) and
// out_mean [2]; pass 2 -> the scratch block of sum(w*da), sum(w*db) [2] and out_comoment [3].  Outputs of k planes are
// [k, n_rows, n_bins] blocks, CovParams::plane apart; the kernels take CovWParams.  The slots keep histogram_cov's sizes, so the
// family rule, the copies, the geometry and the LDS borders are those of histogram_cov.
#pragma once

#include "xhist_cov.hip.h"

namespace xhist {

// The binning kernels of the two passes: covw_sum_generic / covw_dev_generic<CMP, LDS> (block 512) and covw_sum_fast /
// covw_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h; instantiated in xhist_cov_w.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) covw_sum_generic(const CovWParams p) {
  values_generic_body<MomentAcc<2, true, 1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) covw_dev_generic(const CovWParams p) {
  values_generic_body<MomentAcc<2, true, 2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) covw_sum_fast(const CovWParams p) {
  values_fast_body<MomentAcc<2, true, 1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) covw_dev_fast(const CovWParams p) {
  values_fast_body<MomentAcc<2, true, 2>, ST, D, SCAN>(p);
}

}  // namespace xhist
