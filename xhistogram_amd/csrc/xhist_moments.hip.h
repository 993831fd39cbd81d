// xhist_moments.hip.h — the per-bin first and second moments of NV value arrays, with frequency weights (WT) or without: the
// slots, the one accumulator policy of the shared kernel skeletons (xhist_values.hip.h) and the steps between and after the two
// passes, for histogram_mean_var (NV 1; xhist_meanvar.hip.h), its weighted form, histogram_cov (NV 2; xhist_cov.hip.h) and
// histogram_weighted_cov (xhist_cov_w.hip.h).  Their driver is two_pass_run of xhist_values.hip.h.  histogram_skew_kurt runs
// mean_var's pass 1 and a pass 2 of its own for the second, third and fourth moments (Moment4Acc, moments_finalize4, below).
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  A counted sample hands the
// policy its NV values v_k and, weighted, its weight w, all converted to float64 before any product (numpy's astype; a float32
// w*v is exact there).  The skeletons drop a sample whose first value is NaN, the policy one whose second is, whatever its weight
// (pairwise-complete).  Two passes over the data, the corrected two-pass formula of Chan, Golub & LeVeque:
//   pass 1            the first: n = #samples (uint64 atomics), weighted W = sum(w); S_k = sum(v_k), weighted sum(w*v_k)
//   moments_mean      mean_k = S_k / first (NaN where the first is 0), in place
//   pass 2            d_k = v_k - mean_k[bin], wd_k = d_k, weighted w*d_k; the sums of wd_k -> a float64 scratch block, the
//                     sums of wd_j*d_k for j <= k (NV 1: d*d; NV 2: aa, ab, bb) -> the second-moment output
//   moments_finalize  M_jk = sum(wd_j*d_k) - sum(wd_j) sum(wd_k) / first, the M2 (j == k) clamped at 0 and the co-moment not (a
//                     covariance may be negative); NaN where the first is 0 (and where a sum is NaN), in place
// The sum(wd) terms correct the rounding of the means: M2 keeps the digits that sum(v*v) / n - mean^2 cancels away when
// |mean| >> std.  Float64 atomics add in arbitrary order, so the last bits can differ between runs; data whose sums are exact
// in every order give the same bits every time.
//
// LDS slots behind the staged tables: pass 1 keeps a bin's first and its NV sums (ds_add_u32 or ds_add_f64, and NV ds_add_f64
// per sample), pass 2 its NV means (staged from the means' output) and its NV + NV (NV + 1) / 2 sums.  With few bins, the fast
// family keeps 2^copies_log2 copies of every slot, lane i adding into copy i mod 2^copies_log2, so that the lanes of a wavefront
// that meet the same bin do not queue on one LDS address.  Measured on an MI355X (tools/meanvar_bench.py under rocprofv3): C4's
// 50 bins, pass 1 / pass 2 917 / 982 us with one copy, 584 / 604 us with 16 (the weighted histogram: 553); C2's 100 bins 2662 /
// 2612 us with one, 2489 / 2448 with 8 (histogram: 2274).  Each workgroup flushes the bins it reached with global atomics, the
// copies summed in copy order.  Without LDS room the generic family adds straight into the global arrays, and pass 2 reads the
// means through L2.
#pragma once

#include "xhist_values.hip.h"

#include <cstddef>

namespace xhist {

// pass 1: one bin's first (the uint32 count, or the float64 sum of weights) and its NV sums
template <int NV, bool WT>
struct __attribute__((aligned(NV == 1 ? 16 : 8))) MomentSumSlot {
  std::conditional_t<WT, double, uint32_t> n;
  double s[NV];
};
// pass 2: one bin's NV means, its sums of wd_k and its sums of wd_j*d_k, j <= k (NV 2: aa, ab, bb)
template <int NV>
struct MomentDevSlot {
  static constexpr int NQ = NV * (NV + 1) / 2;
  double m[NV], sd[NV], q[NQ];
};
static_assert(sizeof(MomentSumSlot<1, false>) == 16 && sizeof(MomentSumSlot<1, true>) == 16 && sizeof(MomentSumSlot<2, false>) == 24 &&
                  sizeof(MomentSumSlot<2, true>) == 24 && sizeof(MomentDevSlot<1>) == 24 && sizeof(MomentDevSlot<2>) == 56,
              "the slot sizes the family rule and the tests restate; weights do not change them, so neither the choice, the "
              "copies, the geometry nor the LDS borders");
static_assert(offsetof(MomentDevSlot<1>, m) == 0 && offsetof(MomentDevSlot<1>, sd) == 8 && offsetof(MomentDevSlot<1>, q) == 16 &&
                  offsetof(MomentDevSlot<2>, m) == 0 && offsetof(MomentDevSlot<2>, sd) == 16 && offsetof(MomentDevSlot<2>, q) == 32,
              "pass 2's slot: the NV means, the NV first-order sums, then the second-order sums (q[0..2]: aa, ab, bb)");

// the slots for the family rule (choose_values): the same whatever the type of the values, with copies; pass 2's slot decides
template <int NV, bool WT>
constexpr ValuesSlots moment_slots() {
  return {{sizeof(MomentSumSlot<NV, WT>), sizeof(MomentDevSlot<NV>)}, {sizeof(MomentSumSlot<NV, WT>), sizeof(MomentDevSlot<NV>)}, true};
}

// The policy of pass PASS (1 or 2).  The skeletons hand it a sample as the first value and kExtra more arguments: the second
// value (NV 2), then the weight (WT).  [n_rows, n_bins] arrays pre-advanced to row p.row0; an output of several planes is a
// block of such arrays CovParams::plane 8-byte elements apart (the kernels of one value array write single planes, and their
// Params have no `plane`) —
//   pass 1: out = the first [1], out2 = the sums [NV];
//   pass 2: w2_ptr = the means [NV] (read only), out = the sums of wd_k [NV], out2 = the sums of wd_j*d_k [NV (NV + 1) / 2].
// A flush skips a bin nothing reached: its count is 0 or, where no count is kept, its sums are all 0 (then it adds nothing; a
// NaN sum is not 0 and reaches global memory).
//
// The second value's terms are written out under `if constexpr (NV == 2)`, not as loops over k: sums that a flush carries round
// its loop over the copies in an array indexed by a loop variable reach registers only once that loop is unrolled, and the
// kernels then allocate their registers differently (the generic ones of two value arrays moved by up to 130 instructions).
template <int NV, bool WT>
struct MomentTerms {
  static_assert(NV == 1 || NV == 2, "one value array, or two");
  using params_t = std::conditional_t<NV == 1, Params, CovParams>;
  static constexpr bool kCopies = true;
  static constexpr int kExtra = NV - 1 + (WT ? 1 : 0);
  // x, or w * x with the weight of the sample in[0 .. kExtra] (the skeletons' arguments in their order)
  template <typename V>
  static __device__ __forceinline__ double weigh(const V (&in)[1 + kExtra], double x) {
    if constexpr (WT) return (double)in[NV] * x;
    else return x;
  }
};

template <int NV, bool WT, int PASS>
struct MomentAcc;

template <int NV, bool WT>
struct MomentAcc<NV, WT, 1> : MomentTerms<NV, WT> {
  using T = MomentTerms<NV, WT>;
  using typename T::params_t;
  using slot_t = MomentSumSlot<NV, WT>;
  static __device__ __forceinline__ void init(slot_t* s, const params_t& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].n = 0;
      s[i].s[0] = 0.0;
      if constexpr (NV == 2) s[i].s[1] = 0.0;
    }
  }
  template <typename V, typename... X>  // (the sample type, or float64 from the generic family)
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, X... x) {
    const V in[] = {a, x...};
    if constexpr (NV == 2)
      if (!(in[1] == in[1])) return;  // pairwise-complete: a NaN second value drops the sample, whatever its weight
    if constexpr (WT) unsafeAtomicAdd(&s[i].n, (double)in[NV]);
    else atomicAdd(&s[i].n, 1u);
    unsafeAtomicAdd(&s[i].s[0], T::weigh(in, (double)in[0]));
    if constexpr (NV == 2) unsafeAtomicAdd(&s[i].s[1], T::weigh(in, (double)in[1]));
  }
  template <typename... X>
  static __device__ __forceinline__ void global_add(const params_t& p, int64_t row, int64_t bin, double a, X... x) {
    const double in[] = {a, x...};
    if constexpr (NV == 2)
      if (!(in[1] == in[1])) return;
    const int64_t i = row * p.n_bins + bin;
    if constexpr (WT) unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, in[NV]);
    else atomicAdd(reinterpret_cast<unsigned long long*>(p.out) + i, 1ull);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + i, T::weigh(in, in[0]));
    if constexpr (NV == 2) unsafeAtomicAdd(reinterpret_cast<double*>(p.out2) + p.plane + i, T::weigh(in, in[1]));
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const params_t& p, int64_t row) {
    using first_t = std::conditional_t<WT, double, unsigned long long>;
    first_t* first = reinterpret_cast<first_t*>(p.out) + row * p.n_bins;
    double* sum = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      decltype(slot_t::n) n = 0;
      double a[NV] = {};
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t x = s[(b << p.copies_log2) + c];
        n += x.n;
        a[0] += x.s[0];
        if constexpr (NV == 2) a[1] += x.s[1];
      }
      if constexpr (!WT) {
        if (!n) continue;
      } else if constexpr (NV == 1) {
        if (n == 0.0 && a[0] == 0.0) continue;
      } else {
        if (n == 0.0 && a[0] == 0.0 && a[1] == 0.0) continue;
      }
      if constexpr (WT) unsafeAtomicAdd(first + b, n);
      else atomicAdd(first + b, (unsigned long long)n);
      unsafeAtomicAdd(sum + b, a[0]);
      if constexpr (NV == 2) unsafeAtomicAdd(sum + p.plane + b, a[1]);
    }
  }
};

template <int NV, bool WT>
struct MomentAcc<NV, WT, 2> : MomentTerms<NV, WT> {
  using T = MomentTerms<NV, WT>;
  using typename T::params_t;
  using slot_t = MomentDevSlot<NV>;
  static __device__ __forceinline__ void init(slot_t* s, const params_t& p, int64_t row) {
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr) + row * p.n_bins;
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].m[0] = mean[i >> p.copies_log2];
      if constexpr (NV == 2) s[i].m[1] = mean[p.plane + (i >> p.copies_log2)];
      s[i].sd[0] = 0.0;
      if constexpr (NV == 2) s[i].sd[1] = 0.0;
      s[i].q[0] = 0.0;
      if constexpr (NV == 2) {
        s[i].q[1] = 0.0;
        s[i].q[2] = 0.0;
      }
    }
  }
  template <typename V, typename... X>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, X... x) {
    const V in[] = {a, x...};
    if constexpr (NV == 2)
      if (!(in[1] == in[1])) return;
    double d[NV], wd[NV];
    d[0] = (double)in[0] - s[i].m[0];
    if constexpr (NV == 2) d[1] = (double)in[1] - s[i].m[1];
    wd[0] = T::weigh(in, d[0]);
    if constexpr (NV == 2) wd[1] = T::weigh(in, d[1]);
    unsafeAtomicAdd(&s[i].sd[0], wd[0]);
    if constexpr (NV == 2) unsafeAtomicAdd(&s[i].sd[1], wd[1]);
    unsafeAtomicAdd(&s[i].q[0], wd[0] * d[0]);
    if constexpr (NV == 2) {
      unsafeAtomicAdd(&s[i].q[1], wd[0] * d[1]);
      unsafeAtomicAdd(&s[i].q[2], wd[1] * d[1]);
    }
  }
  template <typename... X>
  static __device__ __forceinline__ void global_add(const params_t& p, int64_t row, int64_t bin, double a, X... x) {
    const double in[] = {a, x...};
    if constexpr (NV == 2)
      if (!(in[1] == in[1])) return;
    const int64_t i = row * p.n_bins + bin;
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr);
    double d[NV], wd[NV];
    d[0] = in[0] - mean[i];
    if constexpr (NV == 2) d[1] = in[1] - mean[p.plane + i];
    wd[0] = T::weigh(in, d[0]);
    if constexpr (NV == 2) wd[1] = T::weigh(in, d[1]);
    double* sd = reinterpret_cast<double*>(p.out);
    double* co = reinterpret_cast<double*>(p.out2);
    unsafeAtomicAdd(sd + i, wd[0]);
    if constexpr (NV == 2) unsafeAtomicAdd(sd + p.plane + i, wd[1]);
    unsafeAtomicAdd(co + i, wd[0] * d[0]);
    if constexpr (NV == 2) {
      unsafeAtomicAdd(co + p.plane + i, wd[0] * d[1]);
      unsafeAtomicAdd(co + 2 * p.plane + i, wd[1] * d[1]);
    }
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const params_t& p, int64_t row) {
    double* sd = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* co = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double a[NV] = {}, q[slot_t::NQ] = {};
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t& x = s[(b << p.copies_log2) + c];
        a[0] += x.sd[0];
        if constexpr (NV == 2) a[1] += x.sd[1];
        q[0] += x.q[0];
        if constexpr (NV == 2) {
          q[1] += x.q[1];
          q[2] += x.q[2];
        }
      }
      if constexpr (NV == 1) {
        if (a[0] == 0.0 && q[0] == 0.0) continue;
      } else {
        if (a[0] == 0.0 && a[1] == 0.0 && q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0) continue;
      }
      unsafeAtomicAdd(sd + b, a[0]);
      if constexpr (NV == 2) unsafeAtomicAdd(sd + p.plane + b, a[1]);
      unsafeAtomicAdd(co + b, q[0]);
      if constexpr (NV == 2) {
        unsafeAtomicAdd(co + p.plane + b, q[1]);
        unsafeAtomicAdd(co + 2 * p.plane + b, q[2]);
      }
    }
  }
};

// ---- the third and fourth central moments of one value array (histogram_skew_kurt) ---------------------------------------------
// Pass 1 and the means are those of mean_var (MomentAcc<1, WT, 1>, moments_mean<1, First>).  Pass 2 keeps, per bin, the mean and
// four sums of the terms of a sample, formed in float64 in exactly this order of products:
//   d = v - mean[bin];  t1 = d (weighted: w * d);  t2 = t1 * d;  t3 = t2 * d;  t4 = t3 * d
//   D = sum(t1), Q2 = sum(t2), Q3 = sum(t3), Q4 = sum(t4)
// moments_finalize4 then carries the corrected two-pass formula to the fourth order (see there).
struct Moment4Slot {
  double m, d, q2, q3, q4;
};
static_assert(sizeof(Moment4Slot) == 40 && offsetof(Moment4Slot, m) == 0 && offsetof(Moment4Slot, d) == 8 &&
                  offsetof(Moment4Slot, q2) == 16 && offsetof(Moment4Slot, q4) == 32,
              "pass 2's slot of the four moments: the mean, then D, Q2, Q3, Q4; the size the family rule and the tests restate");

// the slots for the family rule: mean_var's pass 1 beside the 40-byte slot of pass 2, which decides (copies, geometry, borders)
template <bool WT>
constexpr ValuesSlots moment4_slots() {
  return {{sizeof(MomentSumSlot<1, WT>), sizeof(Moment4Slot)}, {sizeof(MomentSumSlot<1, WT>), sizeof(Moment4Slot)}, true};
}

// The policy of pass 2, a sibling of MomentAcc<1, WT, 2>: w2_ptr = the means (read only), out = D [1 plane], out2 = Q2, Q3, Q4
// [3 planes, CovParams::plane elements apart].  Four ds_add_f64 per sample; a flush sums the copies in copy order and skips a
// bin whose four sums are all 0 (a NaN sum is not 0 and reaches global memory).  The skeletons hand it v, then w (WT).
template <bool WT>
struct Moment4Acc {
  using params_t = CovParams;
  using slot_t = Moment4Slot;
  static constexpr bool kCopies = true;
  static constexpr int kExtra = WT ? 1 : 0;
  static __device__ __forceinline__ void init(slot_t* s, const params_t& p, int64_t row) {
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr) + row * p.n_bins;
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].m = mean[i >> p.copies_log2];
      s[i].d = 0.0;
      s[i].q2 = 0.0;
      s[i].q3 = 0.0;
      s[i].q4 = 0.0;
    }
  }
  template <typename V, typename... X>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V a, X... x) {
    const V in[] = {a, x...};
    const double d = (double)in[0] - s[i].m;
    double t1 = d;
    if constexpr (WT) t1 = (double)in[1] * d;
    const double t2 = t1 * d, t3 = t2 * d, t4 = t3 * d;
    unsafeAtomicAdd(&s[i].d, t1);
    unsafeAtomicAdd(&s[i].q2, t2);
    unsafeAtomicAdd(&s[i].q3, t3);
    unsafeAtomicAdd(&s[i].q4, t4);
  }
  template <typename... X>
  static __device__ __forceinline__ void global_add(const params_t& p, int64_t row, int64_t bin, double a, X... x) {
    const double in[] = {a, x...};
    const int64_t i = row * p.n_bins + bin;
    const double d = in[0] - reinterpret_cast<const double*>(p.w2_ptr)[i];
    double t1 = d;
    if constexpr (WT) t1 = in[1] * d;
    const double t2 = t1 * d, t3 = t2 * d, t4 = t3 * d;
    double* q = reinterpret_cast<double*>(p.out2);
    unsafeAtomicAdd(reinterpret_cast<double*>(p.out) + i, t1);
    unsafeAtomicAdd(q + i, t2);
    unsafeAtomicAdd(q + p.plane + i, t3);
    unsafeAtomicAdd(q + 2 * p.plane + i, t4);
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const params_t& p, int64_t row) {
    double* sd = reinterpret_cast<double*>(p.out) + row * p.n_bins;
    double* q = reinterpret_cast<double*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      double a = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0;
      for (uint32_t c = 0; c < copies; ++c) {
        const slot_t& x = s[(b << p.copies_log2) + c];
        a += x.d;
        q2 += x.q2;
        q3 += x.q3;
        q4 += x.q4;
      }
      if (a == 0.0 && q2 == 0.0 && q3 == 0.0 && q4 == 0.0) continue;
      unsafeAtomicAdd(sd + b, a);
      unsafeAtomicAdd(q + b, q2);
      unsafeAtomicAdd(q + p.plane + b, q3);
      unsafeAtomicAdd(q + 2 * p.plane + b, q4);
    }
  }
};

// The steps between and after the passes, over [n] arrays and [k, n] blocks; First is the type of pass 1's first output,
// unsigned long long (the counts) or double (the sums of weights).
// the sums of pass 1 -> the NV means, in place in `sum` [NV, n]: S / first, NaN where the first is 0 (a NaN W gives NaN)
template <int NV, typename First>
__global__ void __launch_bounds__(256) moments_mean(const First* first, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const First c = first[i];
    sum[i] = c != 0 ? sum[i] / (double)c : nan;
    if constexpr (NV == 2) sum[n + i] = c != 0 ? sum[n + i] / (double)c : nan;
  }
}

// the sums of pass 2 -> the second moments, in place in `co` [NV (NV + 1) / 2, n] (NV 2: M2_a, C_ab, M2_b); `sd` is [NV, n].
// The M2 are clamped at 0, the co-moment is not; NaN where the first is 0, and NaN stays NaN
template <int NV, typename First>
__global__ void __launch_bounds__(256) moments_finalize(const First* first, const double* sd, double* co, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const First c = first[i];
    if (c == 0) {
      if constexpr (NV == 1) co[i] = nan;
      else co[i] = co[n + i] = co[2 * n + i] = nan;
      continue;
    }
    double s[NV], r[NV];
    s[0] = sd[i];
    if constexpr (NV == 2) s[1] = sd[n + i];
    r[0] = co[i] - s[0] * s[0] / (double)c;
    if constexpr (NV == 2) r[1] = co[2 * n + i] - s[1] * s[1] / (double)c;
    co[i] = r[0] <= 0.0 ? 0.0 : r[0];
    if constexpr (NV == 2) {
      co[n + i] = co[n + i] - s[0] * s[1] / (double)c;
      co[2 * n + i] = r[1] <= 0.0 ? 0.0 : r[1];
    }
  }
}

// the sums of pass 2 of the four moments -> M2, M3, M4, in place in `q` [3, n] (Q2, Q3, Q4 on entry); `sd` is D [n].  With
// x = first and delta = D / x, every product and sum rounded on its own (no contraction), evaluated in this order:
//   M2 = max(0, Q2 - (D * D) / x)                                    (moments_finalize<1, First>'s very expression)
//   d2 = delta * delta;  d3 = d2 * delta;  d4 = d2 * d2
//   M3 = (Q3 - (3 * delta) * Q2) + (2 * x) * d3                      (not clamped)
//   M4 = max(0, ((Q4 - (4 * delta) * Q3) + (6 * d2) * Q2) - (3 * x) * d4)
// NaN where the first is 0, and NaN stays NaN.
template <typename First>
__global__ void __launch_bounds__(256) moments_finalize4(const First* first, const double* sd, double* q, int64_t n) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const First c = first[i];
    if (c == 0) {
      q[i] = q[n + i] = q[2 * n + i] = nan;
      continue;
    }
    const double x = (double)c, s = sd[i], q2 = q[i], q3 = q[n + i], q4 = q[2 * n + i];
    const double delta = s / x;
    const double d2 = delta * delta, d3 = d2 * delta, d4 = d2 * d2;
    const double r2 = q2 - s * s / x;
    const double r4 = ((q4 - (4.0 * delta) * q3) + (6.0 * d2) * q2) - (3.0 * x) * d4;
    q[i] = r2 <= 0.0 ? 0.0 : r2;
    q[n + i] = (q3 - (3.0 * delta) * q2) + (2.0 * x) * d3;
    q[2 * n + i] = r4 <= 0.0 ? 0.0 : r4;
  }
}

}  // namespace xhist
