// xhist_cov_w.hip.h — per-bin sum of weights, weighted means, weighted sums of squared deviations and weighted co-moment of TWO
// value arrays (histogram_weighted_cov): the two passes' policies for the shared kernel skeletons of xhist_values.hip.h, and
// the binning kernels (their driver: two_pass_run of xhist_values.hip.h).
//
// Which samples count is decided exactly as for histogram_cov (xhist_cov.hip.h): the second value array travels in
// WParams::x_*, the weights are a fourth stream in CovWParams::y_*, and the skeletons hand a policy the triple (a, b, w).  The
// skeletons drop a sample whose a is NaN, the policies one whose b is NaN, whatever its weight (pairwise-complete).  Frequency
// weights, as in the weighted histogram_mean_var (MvwAcc, xhist_meanvar.hip.h), whose terms these are:
//   pass 1 (covw_sum_*)  W = sum(w), Swa = sum(w*a), Swb = sum(w*b)    -> out_wsum [1], out_mean [2] (float64 atomics)
//   covw_mean            mean_a = Swa / W, mean_b = Swb / W (NaN where W == 0), in place
//   pass 2 (covw_dev_*)  da = a - mean_a, db = b - mean_b in float64, wda = w*da, wdb = w*db; the sums of wda and wdb -> a
//                        float64 scratch block [2], the sums of wda*da, wda*db and wdb*db -> out_comoment [3]
//   covw_finalize        M2_a = max(0, sum(w*da^2) - sum(w*da)^2 / W), C_ab = sum(w*da*db) - sum(w*da) sum(w*db) / W (not
//                        clamped), M2_b likewise; NaN where W == 0, in place
// Outputs of k planes are [k, n_rows, n_bins] blocks, CovParams::plane apart, as histogram_cov's.
//
// LDS slots behind the staged tables: pass 1 keeps a bin's three float64 sums in 24 bytes, pass 2 both means and five float64
// sums in 56 bytes (CovDevSlot itself) — the sizes of CovSumSlot and CovDevSlot, so the family rule, the copies, the geometry
// and the LDS borders are those of histogram_cov.
#pragma once

#include "xhist_cov.hip.h"

namespace xhist {

// pass 1: one bin's sum of weights and the weighted sums of both values
struct CovWSumSlot {
  double w, sa, sb;
};
static_assert(sizeof(CovWSumSlot) == sizeof(CovSumSlot) && sizeof(CovWSumSlot) == 24 && sizeof(CovDevSlot) == 56,
              "the weighted passes keep the slot sizes of histogram_cov: the same choice, copies, geometry and LDS borders");

// The policies of the two passes (kWeighted and kSecond: the skeletons hand them (a, b, w)).  Arrays pre-advanced to row
// p.row0, planes p.plane elements apart —
//   pass 1: out = the float64 sums of weights [1], out2 = the float64 sums of w*a and w*b [2];
//   pass 2: as CovAcc<2>, the sums of w*da and w*db [2] and of (w*da)*da, (w*da)*db, (w*db)*db [3].
// A flush skips a bin whose sums are all 0 (nothing reached it, or it adds nothing); a NaN sum is not 0 and reaches global memory.
template <int PASS>
struct CovWAcc;

template <>
struct CovWAcc<1> {
  using slot_t = CovWSumSlot;
  static constexpr bool kCopies = true, kWeighted = true, kSecond = true;
  static __device__ __forceinline__ void init(slot_t* s, const CovParams& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].w = 0.0;
      s[i].sa = 0.0;
      s[i].sb = 0.0;
    }
  }
  template <typename V>  // (values and weights are accumulated in float64 whatever their type)
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, V b, V w) {
    if (!(b == b)) return;  // pairwise-complete: a NaN b drops the triple, whatever its weight (a NaN a never gets here)
    unsafeAtomicAdd(&s[i].w, (double)w);
    unsafeAtomicAdd(&s[i].sa, (double)w * (double)a);
    unsafeAtomicAdd(&s[i].sb, (double)w * (double)b);
  }
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double a, double b, double w) {
    if (!(b == b)) return;
    const int64_t i = row * p.n_bins + bin;
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, w);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, w * a);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + p.plane + i, w * b);
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const CovParams& p, int64_t row) {
    double* ws = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* sum = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double w = 0.0, sa = 0.0, sb = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t x = s[(b << p.copies_log2) + c];
        w += x.w;
        sa += x.sa;
        sb += x.sb;
      }
      if (w == 0.0 && sa == 0.0 && sb == 0.0) continue;
      unsafeAtomicAdd(ws + b, w);
      unsafeAtomicAdd(sum + b, sa);
      unsafeAtomicAdd(sum + p.plane + b, sb);
    }
  }
};

// pass 2: CovAcc<2>'s slots, staging of the means and flush; the terms are the weighted mean_var kernels' (w*d)*d
template <>
struct CovWAcc<2> : CovAcc<2> {
  static constexpr bool kSecond = true;
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, V b, V w) {
    if (!(b == b)) return;
    const double da = (double)a - s[i].ma;
    const double db = (double)b - s[i].mb;
    const double wda = (double)w * da;
    const double wdb = (double)w * db;
    unsafeAtomicAdd(&s[i].sda, wda);
    unsafeAtomicAdd(&s[i].sdb, wdb);
    unsafeAtomicAdd(&s[i].saa, wda * da);
    unsafeAtomicAdd(&s[i].sab, wda * db);
    unsafeAtomicAdd(&s[i].sbb, wdb * db);
  }
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double a, double b, double w) {
    if (!(b == b)) return;
    const int64_t i = row * p.n_bins + bin;
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr);
    const double da = a - mean[i];
    const double db = b - mean[p.plane + i];
    const double wda = w * da;
    const double wdb = w * db;
    double* sd = reinterpret_cast<double*>(p.out);
    double* co = reinterpret_cast<double*>(p.out2);
    unsafeAtomicAdd(sd + i, wda);
    unsafeAtomicAdd(sd + p.plane + i, wdb);
    unsafeAtomicAdd(co + i, wda * da);
    unsafeAtomicAdd(co + p.plane + i, wda * db);
    unsafeAtomicAdd(co + 2 * p.plane + i, wdb * db);
  }
};

// The binning kernels of the two passes: covw_sum_generic / covw_dev_generic<CMP, LDS> (block 512) and covw_sum_fast /
// covw_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h; instantiated in xhist_cov_w.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) covw_sum_generic(const CovWParams p) {
  values_generic_body<CovWAcc<1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) covw_dev_generic(const CovWParams p) {
  values_generic_body<CovWAcc<2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) covw_sum_fast(const CovWParams p) {
  values_fast_body<CovWAcc<1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) covw_dev_fast(const CovWParams p) {
  values_fast_body<CovWAcc<2>, ST, D, SCAN>(p);
}

}  // namespace xhist

// The launches of histogram_weighted_cov for DEVICE arrays the caller has validated, n_rows * n_bins > 0, the plan's device
// current (two_pass_run<CovW>, xhist_cov_w.hip).  out_wsum is [n_rows, n_bins], out_mean [2, n_rows, n_bins] (mean_a, mean_b),
// out_comoment [3, n_rows, n_bins] (M2_a, C_ab, M2_b), `sd` a float64 [2, n_rows, n_bins] block of the caller's for the sums
// of w*da and w*db.  Returns XHIST_OK, or an error status with a message in `err`; `desc` receives a line about the launches.
// (Called by xhist_plan_execute_cov_weighted, xhist_capi.hip.)
int xhist_cov_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                    const xhist_array* weights, int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_comoment,
                    double* sd, hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap);
