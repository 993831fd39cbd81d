// xhist_quantile_w.hip.h — exact weighted per-bin quantiles of a value array (histogram_weighted_quantile, numpy's
// method="inverted_cdf" with weights): the state of a weighted selection, the two weighted policies it plugs into the shared
// kernel skeletons of xhist_values.hip.h, its binning kernels and the short-row kernel (the driver of xhist_quantile_w.hip is
// declared in xhist_values_api.h; its shared host steps are those of xhist_quantile.hip.h).
//
// Samples, values and keys are those of xhist_quantile.hip.h; every counted sample whose value is not NaN also brings its
// weight (float64).  Per (row, bin): W = the sum of its weights, C(x) = the sum of the weights of its values <= x.  A target
// is one (row, bin, q): the smallest value x with C(x) / W >= q and C(x) > 0 (one float64 division, numpy's
// cdf /= cdf[-1]; searchsorted(cdf, q, "left")), or the largest value of positive weight when rounding leaves none.  NaN where
// the bin has no value, W is not finite and positive, or a weight of the bin fails w >= 0 (such a weight adds NaN to W).
//
// RADIX (long rows): the passes of the unweighted family with sums of weights in place of counts.
//   pass 0        the weighted window policy: per (row, bin) the minimum and maximum key, and W
//   qw_init       per target: NaN or constant bins settle at once; else the prefix = the common high bits of min and max
//   digit passes  the weighted digit policy: a value whose key matches a target's prefix adds its weight to that target's
//                 float64 sum of its next d-bit digit (LDS sums by ds_add_f64, flushed with float64 global atomics; or
//                 global sums straight)
//   qw_select     per target: one running sum over its 2^d bucket sums in order; the first bucket with a positive sum and
//                 (below + cum) / W >= q extends the prefix, else the last bucket with a positive sum; sums -> 0
//   qw_finalize   the key of each target into the output (inverted_cdf returns a value of the bin: no successor pass)
// The host launches the worst case, ceil(64 / d) digit passes; a digit pass whose flag word is zero returns at once.  No device ->
// host read inside the call.
//
// SHORT (rows of at most kQWShortCols values): one workgroup sorts the (bin, key, weight) triples of a few whole rows in LDS
// and walks each (row, bin) run with a sequential running sum, which is also numpy's order of additions.
//
// On weights whose float64 sums are exact in any order every result equals numpy's bit for bit.  On other weights the
// atomics' order moves C and W in their last bits, and the result may be a neighbouring value of the bin.
//
// A launch's fields ride in Params as for the unweighted family: part_counts -> the flag word, n_parts -> targets per bin,
// part_shift -> d, w2_ptr -> the targets.
#pragma once

#include "xhist_quantile.hip.h"

namespace xhist {

// The short-row family takes rows of at most this many values: a triple is 20 bytes (key 8, weight 8, slot 4) where the
// unweighted pair is 12, so 2048 of them sort in 40 KiB of LDS, four workgroups per CU (4096 would need 80 KiB).  The bound is
// LDS's.  The two families have not been measured on either side of it yet.
constexpr int kQWShortCols = 2048;
// The digit pass's LDS budget is kQLdsBudget, kept from the unweighted family, where it was measured for 4-byte counters; it
// has not been measured again for the 8-byte sums.

// pass 0's record per (row, bin).  No count is kept: a bin has a value exactly when mn <= mx.
struct QWWin {
  uint64_t mn, mx;  // the minimum and maximum key of the bin's values (mn = ~0, mx = 0 before the pass)
  double w;         // W (NaN once a weight fails w >= 0)
};
// one target's selection state
struct QWTgt {
  uint64_t pre;    // the key prefix found so far (the key itself once nfix == 64)
  double below;    // the weight of every value under the prefix
  double w;        // W of the bin
  uint32_t nfix;   // high key bits fixed (64: settled)
  uint32_t flags;  // kQWNan: the result is NaN
};
constexpr uint32_t kQWNan = 1u;

// the arguments of the steps between the binning passes (one chunk of rows, one group of targets)
struct QWStep {
  QWTgt* tgt;      // [rows, bins, G]
  QWWin* win0;     // [rows, bins]
  double* sum;     // [rows, bins, G, 2^d]
  uint32_t* flags; // [1 + passes]: [1 + j] digit pass j has a live target ([0]: unused, pass 0 always runs)
  double* out;     // [n_q, n_rows_total, bins]
  double q[kQGroup];
  int64_t rows, bins, row0, n_rows_total;
  int32_t G, qi0, d, pass;
};

// a weight as the sums take it: NaN unless w >= 0
__device__ __forceinline__ double qw_weight(double w) { return w >= 0.0 ? w : __builtin_nan(""); }
// numpy's test of one cdf value, in float64
__device__ __forceinline__ bool qw_reached(double c, double w, double q) { return c / w >= q; }

// ---- the weighted window policy (pass 0) ---------------------------------------------------------------------------------
// LDS: per bin {mn, mx, W}.  Global records: p.out = QWWin [rows, bins].
struct QWWinAcc {
  using slot_t = uint64_t;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 1;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t) {
    const uint32_t n = (uint32_t)p.n_bins;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[3 * i] = ~0ull;
      s[3 * i + 1] = 0ull;
      reinterpret_cast<double*>(s)[3 * i + 2] = 0.0;
    }
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t bin, V v, V w) {
    const uint64_t k = extrema_key64((double)v);
    uint64_t* x = s + 3 * (size_t)bin;
    if (k < x[0]) atomicMin(reinterpret_cast<unsigned long long*>(x), (unsigned long long)k);
    if (k > x[1]) atomicMax(reinterpret_cast<unsigned long long*>(x + 1), (unsigned long long)k);
    if ((double)w != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(x + 2), qw_weight((double)w));
  }
  // The record's index within the launch in 32 bits (the driver keeps a chunk's rows x bins below 2^32) and unconditional
  // atomics: with a 64-bit index the float64-domain kernel reserved 36 bytes of scratch for its SGPR spills.
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v, double w) {
    const unsigned long long k = extrema_key64(v);
    QWWin* r = reinterpret_cast<QWWin*>(p.out) + (size_t)((uint32_t)row * (uint32_t)p.n_bins + (uint32_t)b);
    atomicMin(reinterpret_cast<unsigned long long*>(&r->mn), k);
    atomicMax(reinterpret_cast<unsigned long long*>(&r->mx), k);
    unsafeAtomicAdd(&r->w, qw_weight(w));
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    QWWin* r = reinterpret_cast<QWWin*>(p.out) + row * p.n_bins;
    for (uint32_t i = threadIdx.x; i < (uint32_t)p.n_bins; i += blockDim.x) {
      const uint64_t lo = s[3 * i], hi = s[3 * i + 1];
      if (lo > hi) continue;  // (no value arrived)
      const double w = reinterpret_cast<const double*>(s)[3 * i + 2];
      atomicMin(reinterpret_cast<unsigned long long*>(&r[i].mn), (unsigned long long)lo);
      atomicMax(reinterpret_cast<unsigned long long*>(&r[i].mx), (unsigned long long)hi);
      if (w != 0.0) unsafeAtomicAdd(&r[i].w, w);  // (a NaN sum is not 0 and reaches global memory)
    }
  }
};

// ---- the weighted digit policy ----------------------------------------------------------------------------------------------
// LDS: [bins * T] targets {pre, himask, dshift | dmask << 32} (dmask 0: settled), then [bins * T * 2^d] float64 sums.
// Global: p.w2_ptr = QWTgt [rows, bins, T] (read only), p.out = float64 sums [rows, bins, T, 2^d].
struct QWDigitAcc {
  using slot_t = uint64_t;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 1;
  static __device__ __forceinline__ void digit_of(const QWTgt& t, uint32_t d, uint64_t& him, uint32_t& dshift, uint32_t& dmask) {
    him = q_himask(t.nfix);
    const uint32_t left = 64u - t.nfix, dd = left < d ? left : d;
    dshift = left - dd;
    dmask = t.nfix >= 64 ? 0u : (1u << dd) - 1u;
  }
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = (uint32_t)p.n_bins * (uint32_t)p.n_parts, d = (uint32_t)p.part_shift;
    if (threadIdx.x == 0) q_hdr() = QHdr{(uint32_t)p.n_parts, d, n * 3u};
    const QWTgt* tg = reinterpret_cast<const QWTgt*>(p.w2_ptr) + row * (int64_t)n;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const QWTgt t = tg[i];
      uint64_t him;
      uint32_t dshift, dmask;
      digit_of(t, d, him, dshift, dmask);
      s[3 * i] = t.pre & him;
      s[3 * i + 1] = him;
      s[3 * i + 2] = (uint64_t)dshift | (uint64_t)dmask << 32;
    }
    double* sum = reinterpret_cast<double*>(s + (size_t)n * 3);
    for (uint32_t i = threadIdx.x; i < (n << d); i += blockDim.x) sum[i] = 0.0;
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t bin, V v, V w) {
    if (!((double)w > 0.0)) return;  // (zero weights add nothing; a bin with any other such weight is NaN by its W)
    const uint64_t k = extrema_key64((double)v);
    const QHdr h = q_hdr();
    double* sum = reinterpret_cast<double*>(s + h.cnt_off);
    for (uint32_t t = 0; t < h.T; ++t) {
      const uint32_t i = bin * h.T + t;
      const uint64_t sh = s[3 * i + 2];
      const uint32_t dmask = (uint32_t)(sh >> 32);
      if (!dmask || ((k & s[3 * i + 1]) != s[3 * i])) continue;
      unsafeAtomicAdd(sum + ((i << h.d) | ((uint32_t)(k >> (uint32_t)sh) & dmask)), (double)w);
    }
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v, double w) {
    if (!(w > 0.0)) return;
    const uint64_t k = extrema_key64(v);
    const int64_t T = p.n_parts;
    const uint32_t d = (uint32_t)p.part_shift;
    const int64_t i0 = (row * p.n_bins + b) * T;
    const QWTgt* tg = reinterpret_cast<const QWTgt*>(p.w2_ptr) + i0;
    double* sum = reinterpret_cast<double*>(p.out);
    for (int64_t t = 0; t < T; ++t) {
      const QWTgt x = tg[t];
      uint64_t him;
      uint32_t dshift, dmask;
      digit_of(x, d, him, dshift, dmask);
      if (!dmask || ((k ^ x.pre) & him)) continue;
      unsafeAtomicAdd(sum + (((i0 + t) << d) | ((k >> dshift) & dmask)), w);
    }
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = ((uint32_t)p.n_bins * (uint32_t)p.n_parts) << p.part_shift;
    double* g = reinterpret_cast<double*>(p.out) + row * (int64_t)n;
    const double* sum = reinterpret_cast<const double*>(s + q_hdr().cnt_off);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
      if (sum[i] != 0.0) unsafeAtomicAdd(g + i, sum[i]);
  }
};

// The binning kernels: qw_win_* and qw_digit_*, generic<CMP, LDS> (block 512) and fast<ST, D, SCAN> (block 256), the
// families of xhist_values.hip.h with the weights of WParams.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) qw_win_generic(const WParams p) {
  values_generic_body<QWWinAcc, CMP, LDS>(p);  // (pass 0 is always live)
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) qw_digit_generic(const WParams p) {
  if (q_live(p)) values_generic_body<QWDigitAcc, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) qw_win_fast(const WParams p) {
  values_fast_body<QWWinAcc, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) qw_digit_fast(const WParams p) {
  if (q_live(p)) values_fast_body<QWDigitAcc, ST, D, SCAN>(p);
}

// ---- the short-row family ---------------------------------------------------------------------------------------------------
// As q_short, each pair carrying its weight: one workgroup of 256 lanes takes p.lane_rows whole rows (at most kQWShortCols
// values in all, p.slice_n = the power of two above), sorts (row-local flat bin, key, weight) in LDS, and each of its
// (row, bin) lanes walks the bin's run: once for W, then once per target with one running sum.
template <int CMP>
__global__ void __launch_bounds__(256) qw_short(const WParams p, const QWStep st) {
  using CT = typename Dom<CMP>::T;
  const uint32_t N = (uint32_t)p.slice_n, R = (uint32_t)p.lane_rows;
  uint64_t* key = reinterpret_cast<uint64_t*>(xhist_smem);
  double* wt = reinterpret_cast<double*>(key + N);
  uint32_t* slot = reinterpret_cast<uint32_t*>(wt + N);
  const int64_t row_base = (int64_t)blockIdx.x * R;
  const uint32_t nb = (uint32_t)p.n_bins;
  const int nd = p.n_dims;
  const uint32_t total = R * (uint32_t)p.n_cols;
  for (uint32_t j = threadIdx.x; j < N; j += blockDim.x) {
    uint32_t sl = ~0u;
    uint64_t k = 0;
    double w = 0.0;
    if (j < total) {
      const uint32_t lr = j % R;
      const int64_t i = j / R, row = row_base + lr;
      if (row < p.n_rows) {
        const int64_t r = p.row0 + row;
        const double v = load_as<double>(p.w_ptr, p.w_dt, row_offset(r, p.w_rs, p.w_ir, p.w_os) + i * p.w_cs);
        bool ok = v == v;
        int64_t flat = 0;
#pragma unroll
        for (int d = 0; d < kMaxDims; ++d) {
          if (d < nd) {
            const CT x = load_dom<CMP>(p.s_ptr[d], p.s_dt[d], row_offset(r, p.s_rs[d], p.s_ir[d], p.s_os[d]) + i * p.s_cs[d], p.dim[d]);
            const int b = digitize<CMP>(x, p.dim[d], p.tables);
            ok &= (b >= 0);
            flat += (int64_t)b * p.dim[d].out_stride;
          }
        }
        if (ok) {
          sl = lr * nb + (uint32_t)flat;
          k = extrema_key64(v);
          w = qw_weight(load_as<double>(p.x_ptr, p.x_dt, row_offset(r, p.x_rs, p.x_ir, p.x_os) + i * p.x_cs));
        }
      }
    }
    slot[j] = sl;
    key[j] = k;
    wt[j] = w;
  }
  __syncthreads();
  for (uint32_t kk = 2; kk <= N; kk <<= 1)
    for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
      for (uint32_t i = threadIdx.x; i < N / 2; i += blockDim.x) {
        const uint32_t lo = 2 * jj * (i / jj) + (i % jj), hi = lo + jj;
        const bool up = (lo & kk) == 0;
        const uint32_t sa = slot[lo], sb = slot[hi];
        const uint64_t ka = key[lo], kb = key[hi];
        if (q_pair_gt(sa, ka, sb, kb) == up) {
          const double wa = wt[lo], wb = wt[hi];
          slot[lo] = sb;
          slot[hi] = sa;
          key[lo] = kb;
          key[hi] = ka;
          wt[lo] = wb;
          wt[hi] = wa;
        }
      }
      __syncthreads();
    }
  const double nan = __builtin_nan("");
  for (uint32_t j = threadIdx.x; j < R * nb; j += blockDim.x) {
    const int64_t row = row_base + j / nb;
    if (row >= p.n_rows) break;
    uint32_t a = 0, e = N;  // the first triple of slot j
    while (a < e) {
      const uint32_t m = (a + e) / 2;
      if (slot[m] < j) a = m + 1;
      else e = m;
    }
    uint32_t c = a, f = N;  // and the first after it
    while (c < f) {
      const uint32_t m = (c + f) / 2;
      if (slot[m] <= j) c = m + 1;
      else f = m;
    }
    double W = 0.0;  // (a NaN weight makes it NaN)
    for (uint32_t i = a; i < c; ++i) W += wt[i];
    const bool good = c > a && W > 0.0 && W < __builtin_inf();
    for (int t = 0; t < st.G; ++t) {
      double r = nan;
      if (good) {
        const double q = st.q[t];
        double cum = 0.0;
        uint32_t last = a;
        for (uint32_t i = a; i < c; ++i) {
          const double w = wt[i];
          cum += w;
          if (w > 0.0) {
            last = i;
            if (qw_reached(cum, W, q)) break;
          }
        }
        r = extrema_value64(key[last]);
      }
      st.out[((int64_t)(st.qi0 + t) * st.n_rows_total + p.row0 + row) * (int64_t)nb + (j % nb)] = r;
    }
  }
}

}  // namespace xhist
