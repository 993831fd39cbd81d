// xhist_cov.hip.h — per-bin count, means, sums of squared deviations and co-moment of TWO value arrays (histogram_cov): the
// slots and the two passes' policies for the shared kernel skeletons of xhist_values.hip.h, and the binning kernels (their
// driver: two_pass_run of xhist_values.hip.h).
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  The second value array
// travels where the weights of the weighted statistics travel (WParams::x_*), so the skeletons hand a policy the pair (a, b);
// the skeletons drop a sample whose a is NaN, the policies one whose b is NaN (pairwise-complete).  Two passes over the three
// streams, the corrected two-pass form of histogram_mean_var (xhist_meanvar.hip.h) extended by the co-moment:
//   pass 1 (cov_sum_*)  n, Sa = sum(a), Sb = sum(b)                   -> out_count (uint64 atomics), out_mean [2] (float64 atomics)
//   cov_mean            mean_a = Sa / n, mean_b = Sb / n (NaN where n == 0), in place
//   pass 2 (cov_dev_*)  da = a - mean_a, db = b - mean_b in float64; the sums of da and db -> a float64 scratch block [2], the
//                       sums of da*da, da*db and db*db -> out_comoment [3]
//   cov_finalize        M2_a = max(0, sum(da^2) - sum(da)^2 / n), C_ab = sum(da*db) - sum(da) sum(db) / n (not clamped: a
//                       covariance may be negative), M2_b likewise; NaN where n == 0, in place
// Outputs of k planes are [k, n_rows, n_bins] blocks: CovParams::plane is the distance of two planes in 8-byte elements.
//
// LDS slots behind the staged tables: pass 1 keeps a bin's uint32 count and two float64 sums in 24 bytes (ds_add_u32 and two
// ds_add_f64); pass 2 both means (staged from out_mean) and five float64 sums in 56 bytes (two reads and five ds_add_f64 per
// sample).  Copies, flushes and the generic family's global home are those of MvAcc (xhist_meanvar.hip.h).
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

// pass 1: one bin's count and the sums of both values
struct CovSumSlot {
  uint32_t n, pad;
  double sa, sb;
};
// pass 2: one bin's means and its sums of da, db, da*da, da*db, db*db
struct CovDevSlot {
  double ma, mb, sda, sdb, saa, sab, sbb;
};
static_assert(sizeof(CovSumSlot) == 24 && sizeof(CovDevSlot) == 56, "the slot sizes the family rule and the tests restate");

// The policies of the two passes (kWeighted: the skeletons hand them (a, b)).  Arrays pre-advanced to row p.row0, planes
// p.plane elements apart —
//   pass 1: out = the uint64 counts [1], out2 = the float64 sums of a and b [2];
//   pass 2: w2_ptr = the float64 means [2] (read only), out = the float64 sums of da and db [2], out2 = the float64 sums of
//           da*da, da*db, db*db [3].
template <int PASS>
struct CovAcc;

template <>
struct CovAcc<1> {
  using slot_t = CovSumSlot;
  static constexpr bool kCopies = true, kWeighted = true;
  static __device__ __forceinline__ void init(slot_t* s, const CovParams& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].n = 0u;
      s[i].sa = 0.0;
      s[i].sb = 0.0;
    }
  }
  template <typename V>  // (values are accumulated in float64 whatever their type)
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, V b) {
    if (!(b == b)) return;  // pairwise-complete: a NaN b drops the pair (a NaN a never gets here)
    atomicAdd(&s[i].n, 1u);
    unsafeAtomicAdd(&s[i].sa, (double)a);
    unsafeAtomicAdd(&s[i].sb, (double)b);
  }
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double a, double b) {
    if (!(b == b)) return;
    const int64_t i = row * p.n_bins + bin;
    atomicAdd(reinterpret_cast<unsigned long long*>(p.out) + i, 1ull);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, a);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + p.plane + i, b);
  }
  // a workgroup's slots into its row; bins nothing reached are skipped
  static __device__ __forceinline__ void flush(const slot_t* s, const CovParams& p, int64_t row) {
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p.out) + row * p.n_bins;
    double* sum = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      uint32_t n = 0;
      double sa = 0.0, sb = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t x = s[(b << p.copies_log2) + c];
        n += x.n;
        sa += x.sa;
        sb += x.sb;
      }
      if (!n) continue;
      atomicAdd(cnt + b, (unsigned long long)n);
      unsafeAtomicAdd(sum + b, sa);
      unsafeAtomicAdd(sum + p.plane + b, sb);
    }
  }
};

template <>
struct CovAcc<2> {
  using slot_t = CovDevSlot;
  static constexpr bool kCopies = true, kWeighted = true;
  static __device__ __forceinline__ void init(slot_t* s, const CovParams& p, int64_t row) {
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr) + row * p.n_bins;
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].ma = mean[i >> p.copies_log2];
      s[i].mb = mean[p.plane + (i >> p.copies_log2)];
      s[i].sda = 0.0;
      s[i].sdb = 0.0;
      s[i].saa = 0.0;
      s[i].sab = 0.0;
      s[i].sbb = 0.0;
    }
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, V b) {
    if (!(b == b)) return;
    const double da = (double)a - s[i].ma;
    const double db = (double)b - s[i].mb;
    unsafeAtomicAdd(&s[i].sda, da);
    unsafeAtomicAdd(&s[i].sdb, db);
    unsafeAtomicAdd(&s[i].saa, da * da);
    unsafeAtomicAdd(&s[i].sab, da * db);
    unsafeAtomicAdd(&s[i].sbb, db * db);
  }
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double a, double b) {
    if (!(b == b)) return;
    const int64_t i = row * p.n_bins + bin;
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr);
    const double da = a - mean[i];
    const double db = b - mean[p.plane + i];
    double* sd = reinterpret_cast<double*>(p.out);
    double* co = reinterpret_cast<double*>(p.out2);
    unsafeAtomicAdd(sd + i, da);
    unsafeAtomicAdd(sd + p.plane + i, db);
    unsafeAtomicAdd(co + i, da * da);
    unsafeAtomicAdd(co + p.plane + i, da * db);
    unsafeAtomicAdd(co + 2 * p.plane + i, db * db);
  }
  // a bin whose five sums are 0 is skipped (nothing reached it, or it adds nothing); a NaN sum is not 0 and reaches global memory
  static __device__ __forceinline__ void flush(const slot_t* s, const CovParams& p, int64_t row) {
    double* sd = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* co = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double da = 0.0, db = 0.0, aa = 0.0, ab = 0.0, bb = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t& x = s[(b << p.copies_log2) + c];
        da += x.sda;
        db += x.sdb;
        aa += x.saa;
        ab += x.sab;
        bb += x.sbb;
      }
      if (da == 0.0 && db == 0.0 && aa == 0.0 && ab == 0.0 && bb == 0.0) continue;
      unsafeAtomicAdd(sd + b, da);
      unsafeAtomicAdd(sd + p.plane + b, db);
      unsafeAtomicAdd(co + b, aa);
      unsafeAtomicAdd(co + p.plane + b, ab);
      unsafeAtomicAdd(co + 2 * p.plane + b, bb);
    }
  }
};

// The binning kernels of the two passes: cov_sum_generic / cov_dev_generic<CMP, LDS> (block 512) and cov_sum_fast /
// cov_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h; instantiated in xhist_cov.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) cov_sum_generic(const CovParams p) {
  values_generic_body<CovAcc<1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) cov_dev_generic(const CovParams p) {
  values_generic_body<CovAcc<2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) cov_sum_fast(const CovParams p) {
  values_fast_body<CovAcc<1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) cov_dev_fast(const CovParams p) {
  values_fast_body<CovAcc<2>, ST, D, SCAN>(p);
}

}  // namespace xhist

// The launches of histogram_cov for DEVICE arrays the caller has validated, n_rows * n_bins > 0, the plan's device current
// (two_pass_run<Cov>, xhist_cov.hip).  out_mean is [2, n_rows, n_bins] (mean_a, mean_b), out_comoment [3, n_rows, n_bins] (M2_a, C_ab, M2_b), `sd`
// a float64 [2, n_rows, n_bins] block of the caller's for the sums of da and db.  Returns XHIST_OK, or an error status with a
// message in `err`; `desc` receives a line about the launches.  (Called by xhist_plan_execute_cov, xhist_capi.hip.)
int xhist_cov_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                  int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_comoment, double* sd,
                  hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap);
