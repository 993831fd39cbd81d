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
