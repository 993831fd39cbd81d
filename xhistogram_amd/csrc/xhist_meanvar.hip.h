// xhist_meanvar.hip.h — per-bin count, mean and sum of squared deviations of a value array (histogram_mean_var): the slots
// and the two passes' policies for the shared kernel skeletons of xhist_values.hip.h, and the binning kernels of the unweighted
// and the weighted form (their driver: two_pass_run of xhist_values.hip.h).
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  A counted sample whose
// value (converted to float64, numpy's astype) is not NaN contributes that value.  Two passes over the data, the corrected
// two-pass formula of Chan, Golub & LeVeque:
//   pass 1 (mv_sum_*)  n = #values, S = sum of the values             -> out_count (uint64 atomics), out_mean (float64 atomics)
//   mv_mean            mean = S / n (NaN where n == 0), in place in out_mean
//   pass 2 (mv_dev_*)  d = v - mean[bin] in float64; the sums of d and of d*d -> a float64 scratch block and out_m2
//   mv_finalize        M2 = max(0, sum(d*d) - sum(d)^2 / n), NaN where n == 0 (and where a sum is NaN), in place in out_m2
// The sum(d) term corrects the rounding of the mean: M2 keeps the digits that sum(v*v) / n - mean^2 cancels away when
// |mean| >> std.  Float64 atomics add in arbitrary order, so the last bits can differ between runs; data whose sums are exact
// in every order give the same bits every time.
//
// LDS slots behind the staged tables: pass 1 keeps a bin's uint32 count and float64 sum in one 16-byte slot (ds_add_u32 +
// ds_add_f64); pass 2 keeps a bin's mean (staged from out_mean) and its two float64 sums in 24 bytes (one ds_read_b64 and two
// ds_add_f64 per sample).  With few bins, the fast family keeps 2^copies_log2 copies of every slot, lane i adding into copy
// i mod 2^copies_log2, so that the lanes of a wavefront that meet the same bin do not queue on one LDS address.  Measured on
// an MI355X (tools/meanvar_bench.py under rocprofv3): C4's 50 bins, pass 1 / pass 2 917 / 982 us with one copy, 584 / 604 us
// with 16 (the weighted histogram: 553); C2's 100 bins 2662 / 2612 us with one, 2489 / 2448 with 8 (histogram: 2274).
// Each workgroup flushes the bins it reached with global atomics, the copies summed in copy order.  Without LDS room the
// generic family adds straight into the global arrays, and pass 2 reads the means through L2.
//
// Weighted (frequency weights, xhist_meanvar_w.hip): the skeletons' third stream hands each pass the pair (v, w), both in
// float64 (a float32 w*v is exact there), and the same two passes run on weighted sums:
//   pass 1 (mvw_sum_*)  W = sum(w), S = sum(w*v)                      -> out_wsum, out_mean (float64 atomics)
//   mvw_mean            mean = S / W (NaN where W == 0)
//   pass 2 (mvw_dev_*)  d = v - mean[bin]; the sums of w*d and of w*d*d -> the scratch block and out_m2
//   mvw_finalize        M2 = max(0, sum(w*d*d) - sum(w*d)^2 / W), NaN where W == 0
// The slots keep today's sizes: pass 1 {W, S} in 16 bytes (two ds_add_f64), pass 2 the MvDevSlot of the unweighted pass, so
// the choice, the copies and the geometry are those of the unweighted call.
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

// pass 1: one bin's count and sum
struct __attribute__((aligned(16))) MvSumSlot {
  uint32_t n, pad;
  double s;
};
// pass 2: one bin's mean and its sums of d and d*d
struct MvDevSlot {
  double mean, sd, s2;
};

// The statistic of the shared skeletons (xhist_values.hip.h), one policy per pass, with copies of the slots.  [n_rows, n_bins]
// arrays pre-advanced to row p.row0 —
//   pass 1: out = the uint64 counts, out2 = the float64 sums;
//   pass 2: w2_ptr = the float64 means (read only), out = the float64 sums of d, out2 = the float64 sums of d*d.
template <int PASS>
struct MvAcc;

template <>
struct MvAcc<1> {
  using slot_t = MvSumSlot;
  static constexpr bool kCopies = true;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].n = 0u;
      s[i].s = 0.0;
    }
  }
  template <typename V>  // (values are accumulated in float64 whatever their type)
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V v) {
    atomicAdd(&s[i].n, 1u);
    unsafeAtomicAdd(&s[i].s, (double)v);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v) {
    const int64_t i = row * p.n_bins + b;
    atomicAdd(reinterpret_cast<unsigned long long*>(p.out) + i, 1ull);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, v);
  }
  // a workgroup's slots into its row; bins nothing reached are skipped
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p.out) + row * p.n_bins;
    double* sum = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      uint32_t n = 0;
      double a = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t x = s[(b << p.copies_log2) + c];
        n += x.n;
        a += x.s;
      }
      if (!n) continue;
      atomicAdd(cnt + b, (unsigned long long)n);
      unsafeAtomicAdd(sum + b, a);
    }
  }
};

template <>
struct MvAcc<2> {
  using slot_t = MvDevSlot;
  static constexpr bool kCopies = true;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t row) {
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr) + row * p.n_bins;
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].mean = mean[i >> p.copies_log2];
      s[i].sd = 0.0;
      s[i].s2 = 0.0;
    }
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V v) {
    const double d = (double)v - s[i].mean;
    unsafeAtomicAdd(&s[i].sd, d);
    unsafeAtomicAdd(&s[i].s2, d * d);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v) {
    const int64_t i = row * p.n_bins + b;
    const double d = v - reinterpret_cast<const double*>(p.w2_ptr)[i];
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, d);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, d * d);
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    double* sd = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* s2 = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double a = 0.0, q = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        a += s[(b << p.copies_log2) + c].sd;
        q += s[(b << p.copies_log2) + c].s2;
      }
      if (a == 0.0 && q == 0.0) continue;  // (nothing reached the bin, or adds nothing: d = 0 every time)
      unsafeAtomicAdd(sd + b, a);
      unsafeAtomicAdd(s2 + b, q);
    }
  }
};

// The weighted passes' policies (kWeighted: the skeletons hand them (v, w)).  [n_rows, n_bins] arrays pre-advanced to row
// p.row0 —
//   pass 1: out = the float64 sums of weights W, out2 = the float64 sums of w*v;
//   pass 2: as MvAcc<2>, the sums of w*d and w*d*d.
// A flush skips a bin whose two sums are 0 (nothing reached it, or it adds nothing); a NaN sum is not 0 and reaches global memory.
struct __attribute__((aligned(16))) MvwSumSlot {
  double w, s;
};

template <int PASS>
struct MvwAcc;

template <>
struct MvwAcc<1> {
  using slot_t = MvwSumSlot;
  static constexpr bool kCopies = true, kWeighted = true;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].w = 0.0;
      s[i].s = 0.0;
    }
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V v, V w) {
    unsafeAtomicAdd(&s[i].w, (double)w);
    unsafeAtomicAdd(&s[i].s, (double)w * (double)v);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v, double w) {
    const int64_t i = row * p.n_bins + b;
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, w);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, w * v);
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    double* ws = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* sum = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double w = 0.0, a = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t x = s[(b << p.copies_log2) + c];
        w += x.w;
        a += x.s;
      }
      if (w == 0.0 && a == 0.0) continue;
      unsafeAtomicAdd(ws + b, w);
      unsafeAtomicAdd(sum + b, a);
    }
  }
};

template <>
struct MvwAcc<2> : MvAcc<2> {
  static constexpr bool kWeighted = true;
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V v, V w) {
    const double d = (double)v - s[i].mean;
    const double wd = (double)w * d;
    unsafeAtomicAdd(&s[i].sd, wd);
    unsafeAtomicAdd(&s[i].s2, wd * d);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v, double w) {
    const int64_t i = row * p.n_bins + b;
    const double d = v - reinterpret_cast<const double*>(p.w2_ptr)[i];
    const double wd = w * d;
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, wd);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, wd * d);
  }
};

// The binning kernels of the two passes: mv_sum_generic / mv_dev_generic<CMP, LDS> (block 512) and mv_sum_fast /
// mv_dev_fast<ST, D, SCAN> (block 256), the families of xhist_values.hip.h.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_sum_generic(const Params p) {
  values_generic_body<MvAcc<1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_dev_generic(const Params p) {
  values_generic_body<MvAcc<2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_sum_fast(const Params p) {
  values_fast_body<MvAcc<1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_dev_fast(const Params p) {
  values_fast_body<MvAcc<2>, ST, D, SCAN>(p);
}

// ... and of the weighted passes: mvw_sum_generic / mvw_dev_generic<CMP, LDS> (block 512), mvw_sum_fast / mvw_dev_fast<ST, D,
// SCAN> (block 256), instantiated in xhist_meanvar_w.hip only.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mvw_sum_generic(const WParams p) {
  values_generic_body<MvwAcc<1>, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mvw_dev_generic(const WParams p) {
  values_generic_body<MvwAcc<2>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mvw_sum_fast(const WParams p) {
  values_fast_body<MvwAcc<1>, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mvw_dev_fast(const WParams p) {
  values_fast_body<MvwAcc<2>, ST, D, SCAN>(p);
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
