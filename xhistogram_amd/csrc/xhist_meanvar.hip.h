// xhist_meanvar.hip.h — per-bin count, mean and sum of squared deviations of a value array (histogram_mean_var), and the
// weighted form: the binning kernels of both (their driver: two_pass_run of xhist_values.hip.h).
//
// One value array (NV = 1) of the moments of xhist_moments.hip.h, where the formulas, the slots and the policy live.
//   unweighted  the skeletons hand the policy v; pass 1 -> out_count (uint64) and out_mean, pass 2 -> the scratch block of
//               sum(d) and out_m2.  Kernels take Params.
//   weighted    frequency weights as the skeletons' third stream (WParams::x_*): the policy is handed (v, w); pass 1 ->
//               out_wsum (float64) and out_mean, pass 2 -> sum(w*d) and out_m2.  Kernels take WParams; the slots keep the
//               unweighted sizes, so the choice, the copies and the geometry are those of the unweighted call.
// Every output is one [n_rows, n_bins] plane.
#pragma once

#include "xhist_moments.hip.h"

namespace xhist {

// The binning kernels of the two passes: mv_sum_generic / mv_dev_generic<CMP, LDS> (block 512) and mv_sum_fast /
// mv_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_sum_generic(const Params p) {
  values_generic_body<MomentAcc<1, false, 1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_dev_generic(const Params p) {
  values_generic_body<MomentAcc<1, false, 2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_sum_fast(const Params p) {
  values_fast_body<MomentAcc<1, false, 1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_dev_fast(const Params p) {
  values_fast_body<MomentAcc<1, false, 2>, ST, D, SCAN>(p);
}

// ... and of the weighted passes: mvw_sum_generic / mvw_dev_generic<CMP, LDS> (block 512), mvw_sum_fast / mvw_dev_fast<ST, D,
// SCAN> (block 256), instantiated in xhist_meanvar_w.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mvw_sum_generic(const WParams p) {
  values_generic_body<MomentAcc<1, true, 1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mvw_dev_generic(const WParams p) {
  values_generic_body<MomentAcc<1, true, 2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mvw_sum_fast(const WParams p) {
  values_fast_body<MomentAcc<1, true, 1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mvw_dev_fast(const WParams p) {
  values_fast_body<MomentAcc<1, true, 2>, ST, D, SCAN>(p);
}

// The binning kernels of pass 2 of the third and fourth moments (histogram_skew_kurt): sk_dev_generic<CMP, LDS> / sk_dev_fast<ST,
// D, SCAN>, instantiated in xhist_meanvar.hip only beside the mv_sum_* they follow, and the weighted skw_dev_*, instantiated in
// xhist_meanvar_w.hip only beside mvw_sum_*.  Pass 1 is mean_var's own.  They take CovParams: out2 is a block of three planes
// (Q2, Q3, Q4); the unweighted ones read no x_* stream.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) sk_dev_generic(const CovParams p) {
  values_generic_body<Moment4Acc<false>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) sk_dev_fast(const CovParams p) {
  values_fast_body<Moment4Acc<false>, ST, D, SCAN>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) skw_dev_generic(const CovParams p) {
  values_generic_body<Moment4Acc<true>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) skw_dev_fast(const CovParams p) {
  values_fast_body<Moment4Acc<true>, ST, D, SCAN>(p);
}

}  // namespace xhist
