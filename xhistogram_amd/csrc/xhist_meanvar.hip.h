// xhist_meanvar.hip.h — per-bin count, mean and sum of squared deviations of a value array (histogram_mean_var): the kernels,
// and what the C ABI (xhist_capi.hip) hands the selection function of the translation unit xhist_meanvar.hip.
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
#pragma once

#include "xhist_extrema.hip.h"

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

// Params of both passes: samples and values (w_*) as for extrema_generic / extrema_fast; [n_rows, n_bins] arrays pre-advanced
// to row p.row0 —
//   pass 1: out = the uint64 counts, out2 = the float64 sums;
//   pass 2: w2_ptr = the float64 means (read only), out = the float64 sums of d, out2 = the float64 sums of d*d.
// The slots sit behind the staged tables, 16-byte aligned, as in the extrema kernels; bin b's copy c is slot
// (b << p.copies_log2) + c (the generic family: one copy).
template <int PASS>
struct MvAcc;

template <>
struct MvAcc<1> {
  using slot_t = MvSumSlot;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].n = 0u;
      s[i].s = 0.0;
    }
  }
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, double v) {
    atomicAdd(&s[i].n, 1u);
    unsafeAtomicAdd(&s[i].s, v);
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
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t row) {
    const double* mean = reinterpret_cast<const double*>(p.w2_ptr) + row * p.n_bins;
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[i].mean = mean[i >> p.copies_log2];
      s[i].sd = 0.0;
      s[i].s2 = 0.0;
    }
  }
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, double v) {
    const double d = v - s[i].mean;
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

// ---------------------------------------------------------------------------------------------
// GENERIC family body: any dtype per input and for the values, any element strides (broadcast and grouped rows), 1..8 inputs,
// compare domains 0 (float64), 1 (int64) and 3 (per input).  LDS: the slots of every bin in LDS behind the tables (which are
// then in LDS too).  Else every sample adds into the global arrays, and the tables are read from LDS when they fit there
// (p.tables_in_lds) and through L2 otherwise.
// ---------------------------------------------------------------------------------------------
template <int PASS, int CMP, bool LDS>
__device__ __forceinline__ void mv_generic_body(const Params& p) {
  using CT = typename Dom<CMP>::T;
  using A = MvAcc<PASS>;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = p.tables_in_lds ? stage_tables(p) : p.tables;
  typename A::slot_t* slots = reinterpret_cast<typename A::slot_t*>(xhist_smem + ext_slots_offset(p));
  if (LDS) A::init(slots, p, row);
  __syncthreads();

  const int nd = p.n_dims;
  int64_t roff[kMaxDims];
#pragma unroll
  for (int d = 0; d < kMaxDims; ++d) roff[d] = d < nd ? row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]) : 0;
  const int64_t voff = row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);

  const int64_t stride = (int64_t)p.segs * blockDim.x;
  for (int64_t i = (int64_t)seg * blockDim.x + threadIdx.x; i < p.n_cols; i += stride) {
    const double v = load_as<double>(p.w_ptr, p.w_dt, voff + i * p.w_cs);
    bool ok = v == v;  // NaN values are ignored (np.nanmean / np.nanvar)
    int64_t flat = 0;
#pragma unroll
    for (int d = 0; d < kMaxDims; ++d) {
      if (d < nd) {
        const CT x = load_dom<CMP>(p.s_ptr[d], p.s_dt[d], roff[d] + i * p.s_cs[d], p.dim[d]);
        const int b = digitize<CMP>(x, p.dim[d], tab);
        ok &= (b >= 0);
        flat += (int64_t)b * p.dim[d].out_stride;
      }
    }
    if (!ok) continue;
    if (LDS) A::lds_add(slots, (uint32_t)flat, v);  // (one copy of the slots: p.copies_log2 == 0)
    else A::global_add(p, row, flat, v);
  }
  if (LDS) {
    __syncthreads();
    A::flush(slots, p, row);
  }
}

template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_sum_generic(const Params p) {
  mv_generic_body<1, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) mv_dev_generic(const Params p) {
  mv_generic_body<2, CMP, LDS>(p);
}

// ---------------------------------------------------------------------------------------------
// VECTOR fast path body: float32 or float64 samples with values of the same type, unit column stride, one or two inputs, slots
// in LDS; digitize by the tables with at most two edges per bucket (SCAN 1 / 2) or by arithmetic (kScanArith).  Tiles as in
// extrema_fast: VEC elements per 16-byte non-temporal load, UNROLL loads in flight per array and lane; the workgroups of a row
// walk its tiles interleaved.  Values are accumulated in float64 whatever their type.
// ---------------------------------------------------------------------------------------------
template <int PASS, typename ST, int D, int SCAN>
__device__ __forceinline__ void mv_fast_body(const Params& p) {
  static_assert(__is_same(ST, double) || __is_same(ST, float), "float32 / float64 samples and values");
  static_assert(SCAN == 1 || SCAN == 2 || SCAN == kScanArith, "tables with <= 2 edges per bucket, or arithmetic edges");
  constexpr int CMP = (__is_same(ST, float) && SCAN != kScanArith) ? 2 : 0;
  constexpr int VEC = 16 / (int)sizeof(ST);
  constexpr int UNROLL = D == 1 ? 4 : 8 / VEC;
  using A = MvAcc<PASS>;
  using svec = typename VecOf<ST, VEC>::type;

  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = stage_tables(p);
  typename A::slot_t* slots = reinterpret_cast<typename A::slot_t*>(xhist_smem + ext_slots_offset(p));
  A::init(slots, p, row);
  __syncthreads();

  const ST* sp[D];
#pragma unroll
  for (int d = 0; d < D; ++d) sp[d] = reinterpret_cast<const ST*>(p.s_ptr[d]) + row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]);
  const ST* vp = reinterpret_cast<const ST*>(p.w_ptr) + row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);
  const uint32_t nb1 = D == 2 ? (uint32_t)p.dim[1].nb : 1u;
  const uint32_t mycopy = (uint32_t)tid & ((1u << p.copies_log2) - 1u);

  const int64_t tile_elems = (int64_t)blockDim.x * VEC * UNROLL;
  const int64_t n_tiles = (p.n_cols + tile_elems - 1) / tile_elems;
  for (int64_t t = seg; t < n_tiles; t += p.segs) {
    const int64_t base = t * tile_elems;
    svec xv[D][UNROLL], vv[UNROLL];
    if (base + tile_elems <= p.n_cols) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d][u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(sp[d] + i));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(vp + i));
      }
    } else {  // the ragged last tile: positions past the end become NaN samples, which digitize drops
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const bool in = i + v < p.n_cols;
#pragma unroll
          for (int d = 0; d < D; ++d) xv[d][u][v] = in ? sp[d][i + v] : (ST)__builtin_nanf("");
          vv[u][v] = in ? vp[i + v] : (ST)__builtin_nanf("");
        }
      }
    }
    uint32_t cnt[D][UNROLL][VEC];
    count_le_tile<CMP, SCAN, D, UNROLL, VEC>(xv, p, tab, 1, cnt);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const ST val = vv[u][v];
        bool ok = val == val;
        uint32_t flat = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int b = bin_from_tile_count<CMP, SCAN>((typename Dom<CMP>::T)xv[d][u][v], p.dim[d], cnt[d][u][v]);
          ok &= b >= 0;
          flat = d == 0 ? (uint32_t)b : flat * nb1 + (uint32_t)b;
        }
        if (ok) A::lds_add(slots, (flat << p.copies_log2) + mycopy, (double)val);
      }
  }
  __syncthreads();
  A::flush(slots, p, row);
}

template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_sum_fast(const Params p) {
  mv_fast_body<1, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) mv_dev_fast(const Params p) {
  mv_fast_body<2, ST, D, SCAN>(p);
}

}  // namespace xhist

// ---- the selection function of xhist_meanvar.hip, called by xhist_plan_execute_mean_var (xhist_capi.hip) --------------------
// What it needs of a plan is what the extrema unit needs (ExtremaPlan, xhist_extrema.hip.h).
// The zeroing and the five launches on `stream` (pass 1, mean, pass 2, finalize) for DEVICE arrays the caller has validated,
// n_rows * n_bins > 0, the plan's device current.  `sd` is a float64 [n_rows, n_bins] block of the caller's for the sums of d.
// Returns XHIST_OK, or an error status with a message in `err`; `desc` receives a line about the launches.
int xhist_meanvar_run(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      int64_t* out_count, double* out_mean, double* out_m2, double* sd, hipStream_t stream, char* err, size_t err_cap,
                      char* desc, size_t desc_cap);
