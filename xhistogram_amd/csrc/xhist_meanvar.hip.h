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

// ---- host side ---------------------------------------------------------------------------------------------------------------
// The launches of histogram_mean_var for DEVICE arrays the caller has validated, n_rows * n_bins > 0, the plan's device
// current (two_pass_run<MeanVar>, xhist_meanvar.hip).  `sd` is a float64 [n_rows, n_bins] block of the caller's for the sums of
// d.  Returns XHIST_OK, or an error status with a message in `err`; `desc` receives a line about the launches.  (Called by
// xhist_plan_execute_mean_var, xhist_capi.hip.)
int xhist_meanvar_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      int64_t* out_count, double* out_mean, double* out_m2, double* sd, hipStream_t stream, char* err, size_t err_cap,
                      char* desc, size_t desc_cap);

// The same for the weighted form (two_pass_run<MeanVarW>, xhist_meanvar_w.hip): `weights` a validated DEVICE array of the
// samples' logical shape, the sums of weights into out_wsum (float64).  (Called by xhist_plan_execute_mean_var_weighted,
// xhist_capi.hip.)
int xhist_meanvar_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, const xhist_array* weights,
                        int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_m2, double* sd, hipStream_t stream,
                        char* err, size_t err_cap, char* desc, size_t desc_cap);

// The launches of histogram_skew_kurt (two_pass_run<SkewKurt>, xhist_meanvar.hip): mean_var's pass 1 and means, then the four
// sums of pass 2 and moments_finalize4.  out_moments is a float64 [3, n_rows, n_bins] block (M2, M3, M4), `sd` a float64
// [n_rows, n_bins] block of the caller's for D.  (Called by xhist_plan_execute_skew_kurt, xhist_capi.hip.)
int xhist_skew_kurt_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                        int64_t* out_count, double* out_mean, double* out_moments, double* sd, hipStream_t stream, char* err,
                        size_t err_cap, char* desc, size_t desc_cap);

// The same for the weighted form (two_pass_run<SkewKurtW>, xhist_meanvar_w.hip).  (Called by
// xhist_plan_execute_skew_kurt_weighted, xhist_capi.hip.)
int xhist_skew_kurt_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, const xhist_array* weights,
                          int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_moments, double* sd,
                          hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap);
