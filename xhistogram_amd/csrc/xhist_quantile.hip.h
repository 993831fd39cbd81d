// xhist_quantile.hip.h — exact per-bin quantiles of a value array (histogram_quantile): the state of a selection, the two
// policies it plugs into the shared kernel skeletons of xhist_values.hip.h, its binning kernels, the short-row kernel, the
// host steps that the driver of xhist_quantile.hip shares with the weighted one of xhist_quantile_w.hip (templates over the
// launch-parameter type, at the end; the drivers are declared in xhist_values_api.h).
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  A counted sample whose
// value (converted to float64) is not NaN contributes the order-preserving key of that value (extrema_key64: unsigned order
// is the total order with -0.0 < +0.0).  A target is one (row, bin, q): the value of rank r among the bin's n values, r the
// floor of numpy's virtual index.  Two families:
//
// RADIX (long rows): exact radix select, most significant digit first, in streaming passes over the data.
//   pass 0        the window policy with the window [0, ~0]: per (row, bin) n and the minimum and maximum key
//   q_init        rank r per target; its prefix = the common high bits of min and max; an empty bin, or one whose min equals
//                 its max, is settled at once
//   digit passes  the digit policy: a value whose key matches a target's prefix adds 1 to that target's counter of its next
//                 d-bit digit (LDS counters, flushed to global ones; or global counters straight)
//   q_select      per target: the digit that holds the remaining rank extends the prefix, the rank shrinks, counters -> 0
//   successor     linear / midpoint need rank r + 1 too: the same key when the target's remaining rank k and the number m of
//                 values equal to its key satisfy k + 1 < m, else the smallest key in (key, ~0] — one more run of the window
//                 policy, one window per target
//   q_finalize    numpy's interpolation into the output
// The host launches the worst case, ceil(64 / d) digit passes; a pass whose flag word q_select (q_init for the first) left at
// zero returns at once.  No device -> host read inside the call.
//
// SHORT (rows of at most kQShortCols values, e.g. a reduction over a leading time axis): one workgroup sorts the (bin, key)
// pairs of a few whole rows in LDS (bitonic) and reads every order statistic by index, in one pass over the data.  On such
// rows the radix family would stream ~9 times and keep 2^d counters per (row, bin, q) in global memory.
//
// A launch's quantile fields ride in the Params fields of the partitioned histogram, which the values kernels never read:
//   part_counts -> the launch's flag word, n_parts -> targets per bin of its records, part_shift -> d.
#pragma once

#include "xhist_values.hip.h"
#include "xhist_extrema.hip.h"  // extrema_key64 / extrema_value64 (templates and inline functions only)

namespace xhist {

constexpr int kQGroup = 8;          // targets (q values) per group: the q values of a group ride in the kernel arguments
// The short-row family takes rows of at most this many values: 4096 (bin, key) pairs of 12 bytes sort in 48 KiB of LDS, three
// workgroups per CU.  The bound is LDS's, and the families were measured on both sides of it (tools/quantile_bench.py, 100
// bins, median): 2000 rows of 4096 float32 values 0.50 ms sorted, 2000 rows of 4097 1.68 ms by radix select.
constexpr int kQShortCols = 4096;
constexpr size_t kQScratchCap = (size_t)256 << 20;  // the radix family's per-chunk scratch (rows are processed in chunks)
// LDS of a digit pass when a choice within it exists: four workgroups of 256 lanes per CU.  Measured on an MI355X
// (tools/quantile_bench.py under rocprofv3): C2's median at d = 8 took 105 KiB per workgroup, one per CU, and each digit pass
// ran at 4.95 ms against 2.38 for the weighted histogram; pass 0 (6 KiB) at 2.99.
constexpr size_t kQLdsBudget = 40 * 1024;

// one window of keys per (row, bin, target): [lo, hi] in; count, minimum and maximum key of the values inside out
struct QWin {
  uint64_t lo, hi, n, mn, mx;
};
// one target's selection state
struct QTgt {
  uint64_t pre;   // the key prefix found so far (the key itself once nfix == 64)
  uint64_t k;     // rank among the values that match the prefix
  uint64_t m;     // values in the last digit chosen (once settled: values equal to the key)
  uint64_t n;     // the bin's values
  uint32_t nfix;  // high key bits fixed (64: settled)
  uint32_t flags; // kQNeedNext: the method needs rank r + 1 too
};
constexpr uint32_t kQNeedNext = 1u;

// the arguments of the steps between the binning passes (one chunk of rows, one group of targets)
struct QStep {
  QTgt* tgt;            // [rows, bins, G]
  QWin* win0;           // [rows, bins]: pass 0
  QWin* win;            // [rows, bins, G]: the successor windows
  unsigned long long* cnt;  // [rows, bins, G, 2^d]
  uint32_t* flags;      // [2 + passes]: pass 0, the digit passes, the successor pass
  double* out;          // [n_q, n_rows_total, bins]
  double q[kQGroup];
  int64_t rows, bins, row0, n_rows_total;
  int32_t G, qi0, method, d, pass;
};

__device__ __forceinline__ uint64_t q_himask(uint32_t nfix) { return nfix ? ~0ull << (64 - nfix) : 0ull; }

// The numpy arithmetic (numpy/lib/_function_base_impl.py, _QuantileMethods, _get_indexes, _get_gamma, _lerp) in float64,
// without contraction: the virtual index of q among n values, and the rank of the first value it reads.
__device__ __forceinline__ double q_virtual(int method, uint64_t n, double q) {
#pragma clang fp contract(off)
  const double x = (double)(n - 1) * q;
  switch (method) {
    case XHIST_Q_LOWER: return floor(x);
    case XHIST_Q_HIGHER: return ceil(x);
    case XHIST_Q_MIDPOINT: return 0.5 * (floor(x) + ceil(x));
    case XHIST_Q_NEAREST: return rint(x);  // np.around: half to even
    default: return x;
  }
}
__device__ __forceinline__ bool q_lerps(int method) { return method == XHIST_Q_LINEAR || method == XHIST_Q_MIDPOINT; }
// the rank read first: the index itself for the taking methods; floor (n - 1 above the bounds) for the interpolating ones
__device__ __forceinline__ uint64_t q_rank(int method, uint64_t n, double vi) {
  if (!q_lerps(method)) return (uint64_t)vi;
  return vi >= (double)(n - 1) ? n - 1 : (uint64_t)floor(vi);
}
// the value of a target: a = the value of rank r, b = that of rank r + 1 (unused by the taking methods)
__device__ __forceinline__ double q_value(int method, uint64_t n, double vi, double a, double b) {
#pragma clang fp contract(off)
  if (!q_lerps(method)) return a;
  const bool above = vi >= (double)(n - 1);
  if (above) b = a;  // previous = next = the last value
  double gamma;
  if (method == XHIST_Q_LINEAR) gamma = vi - (above ? -1.0 : floor(vi));
  else gamma = vi == floor(vi) ? 0.0 : 0.5;  // midpoint's fix_gamma: 0 where the index is whole
  const double diff = b - a;
  return gamma >= 0.5 ? b - diff * (1.0 - gamma) : a + diff * gamma;
}

// what lds_add needs of its launch, set by init
struct QHdr {
  uint32_t T, d, cnt_off;
};
__device__ __forceinline__ QHdr& q_hdr() {
  __shared__ QHdr h;
  return h;
}

// ---- the window policy (pass 0 and the successor) ----------------------------------------------------------------------
// LDS: [bins * T] windows {lo, hi, mn, mx}, then [bins * T] uint32 counts.  Global records: p.out = QWin [rows, bins, T].
struct QWinAcc {
  using slot_t = uint64_t;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 0;
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = (uint32_t)p.n_bins * (uint32_t)p.n_parts;
    if (threadIdx.x == 0) q_hdr() = QHdr{(uint32_t)p.n_parts, 0u, n * 4u};
    const QWin* w = reinterpret_cast<const QWin*>(p.out) + row * (int64_t)n;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(s + (size_t)n * 4);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      s[4 * i] = w[i].lo;
      s[4 * i + 1] = w[i].hi;
      s[4 * i + 2] = ~0ull;
      s[4 * i + 3] = 0ull;
      cnt[i] = 0u;
    }
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t bin, V v) {
    const uint64_t k = extrema_key64((double)v);
    const uint32_t T = q_hdr().T;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(s + q_hdr().cnt_off);
    for (uint32_t t = 0; t < T; ++t) {
      const uint32_t i = bin * T + t;
      uint64_t* w = s + 4 * (size_t)i;
      if (k < w[0] || k > w[1]) continue;
      atomicAdd(cnt + i, 1u);
      if (k < w[2]) atomicMin(reinterpret_cast<unsigned long long*>(w + 2), (unsigned long long)k);
      if (k > w[3]) atomicMax(reinterpret_cast<unsigned long long*>(w + 3), (unsigned long long)k);
    }
  }
  static __device__ __forceinline__ void global_one(QWin* w, uint64_t n, uint64_t lo, uint64_t hi) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&w->n), (unsigned long long)n);
    if (lo < __hip_atomic_load(&w->mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(reinterpret_cast<unsigned long long*>(&w->mn), (unsigned long long)lo);
    if (hi > __hip_atomic_load(&w->mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(reinterpret_cast<unsigned long long*>(&w->mx), (unsigned long long)hi);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v) {
    const uint64_t k = extrema_key64(v);
    const int64_t T = p.n_parts;
    QWin* w = reinterpret_cast<QWin*>(p.out) + (row * p.n_bins + b) * T;
    for (int64_t t = 0; t < T; ++t)
      if (k >= w[t].lo && k <= w[t].hi) global_one(w + t, 1, k, k);
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = (uint32_t)p.n_bins * (uint32_t)p.n_parts;
    QWin* w = reinterpret_cast<QWin*>(p.out) + row * (int64_t)n;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(s + (size_t)n * 4);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
      if (cnt[i]) global_one(w + i, cnt[i], s[4 * i + 2], s[4 * i + 3]);
  }
};

// ---- the digit policy -------------------------------------------------------------------------------------------------------
// LDS: [bins * T] targets {pre, himask, dshift | dmask << 32} (dmask 0: settled), then [bins * T * 2^d] uint32 counters.
// Global: p.w2_ptr = QTgt [rows, bins, T] (read only), p.out = uint64 counters [rows, bins, T, 2^d].
struct QDigitAcc {
  using slot_t = uint64_t;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 0;
  // a target's prefix mask, digit shift and digit mask for digits of d bits
  static __device__ __forceinline__ void digit_of(const QTgt& t, uint32_t d, uint64_t& him, uint32_t& dshift, uint32_t& dmask) {
    him = q_himask(t.nfix);
    const uint32_t left = 64u - t.nfix, dd = left < d ? left : d;
    dshift = left - dd;
    dmask = t.nfix >= 64 ? 0u : (1u << dd) - 1u;
  }
  static __device__ __forceinline__ void init(slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = (uint32_t)p.n_bins * (uint32_t)p.n_parts, d = (uint32_t)p.part_shift;
    if (threadIdx.x == 0) q_hdr() = QHdr{(uint32_t)p.n_parts, d, n * 3u};
    const QTgt* tg = reinterpret_cast<const QTgt*>(p.w2_ptr) + row * (int64_t)n;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const QTgt t = tg[i];
      uint64_t him;
      uint32_t dshift, dmask;
      digit_of(t, d, him, dshift, dmask);
      s[3 * i] = t.pre & him;
      s[3 * i + 1] = him;
      s[3 * i + 2] = (uint64_t)dshift | (uint64_t)dmask << 32;
    }
    uint32_t* cnt = reinterpret_cast<uint32_t*>(s + (size_t)n * 3);
    for (uint32_t i = threadIdx.x; i < (n << d); i += blockDim.x) cnt[i] = 0u;
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t bin, V v) {
    const uint64_t k = extrema_key64((double)v);
    const QHdr h = q_hdr();
    uint32_t* cnt = reinterpret_cast<uint32_t*>(s + h.cnt_off);
    for (uint32_t t = 0; t < h.T; ++t) {
      const uint32_t i = bin * h.T + t;
      const uint64_t sh = s[3 * i + 2];
      const uint32_t dmask = (uint32_t)(sh >> 32);
      if (!dmask || ((k & s[3 * i + 1]) != s[3 * i])) continue;
      atomicAdd(cnt + ((i << h.d) | ((uint32_t)(k >> (uint32_t)sh) & dmask)), 1u);
    }
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t b, double v) {
    const uint64_t k = extrema_key64(v);
    const int64_t T = p.n_parts;
    const uint32_t d = (uint32_t)p.part_shift;
    const int64_t i0 = (row * p.n_bins + b) * T;
    const QTgt* tg = reinterpret_cast<const QTgt*>(p.w2_ptr) + i0;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p.out);
    for (int64_t t = 0; t < T; ++t) {
      const QTgt x = tg[t];
      uint64_t him;
      uint32_t dshift, dmask;
      digit_of(x, d, him, dshift, dmask);
      if (!dmask || ((k ^ x.pre) & him)) continue;
      atomicAdd(cnt + (((i0 + t) << d) | ((k >> dshift) & dmask)), 1ull);
    }
  }
  static __device__ __forceinline__ void flush(const slot_t* s, const Params& p, int64_t row) {
    const uint32_t n = ((uint32_t)p.n_bins * (uint32_t)p.n_parts) << p.part_shift;
    unsigned long long* g = reinterpret_cast<unsigned long long*>(p.out) + row * (int64_t)n;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(s + q_hdr().cnt_off);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
      if (cnt[i]) atomicAdd(g + i, (unsigned long long)cnt[i]);
  }
};

// a binning pass returns at once when its flag word says that no target of the launch is active
__device__ __forceinline__ bool q_live(const Params& p) { return *reinterpret_cast<const volatile uint32_t*>(p.part_counts) != 0u; }

// The binning kernels: q_win_* and q_digit_*, generic<CMP, LDS> (block 512) and fast<ST, D, SCAN> (block 256), the families
// of xhist_values.hip.h.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) q_win_generic(const Params p) {
  if (q_live(p)) values_generic_body<QWinAcc, CMP, LDS>(p);
}
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) q_digit_generic(const Params p) {
  if (q_live(p)) values_generic_body<QDigitAcc, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) q_win_fast(const Params p) {
  if (q_live(p)) values_fast_body<QWinAcc, ST, D, SCAN>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) q_digit_fast(const Params p) {
  if (q_live(p)) values_fast_body<QDigitAcc, ST, D, SCAN>(p);
}

// ---- the short-row family ---------------------------------------------------------------------------------------------------
// One workgroup of 256 lanes takes p.lane_rows whole rows (at most kQShortCols values in all, p.slice_n = the power of two
// above): it loads (row-local flat bin, key) pairs, column-major over its rows so that neighbouring lanes read neighbouring
// rows, sorts them in LDS, and for each of its (row, bin) finds the bin's run by binary search and reads the targets.
__device__ __forceinline__ bool q_pair_gt(uint32_t sa, uint64_t ka, uint32_t sb, uint64_t kb) { return sa != sb ? sa > sb : ka > kb; }

template <int CMP>
__global__ void __launch_bounds__(256) q_short(const Params p, const QStep st) {
  using CT = typename Dom<CMP>::T;
  const uint32_t N = (uint32_t)p.slice_n, R = (uint32_t)p.lane_rows;
  uint64_t* key = reinterpret_cast<uint64_t*>(xhist_smem);
  uint32_t* slot = reinterpret_cast<uint32_t*>(key + N);
  const int64_t row_base = (int64_t)blockIdx.x * R;
  const uint32_t nb = (uint32_t)p.n_bins;
  const int nd = p.n_dims;
  const uint32_t total = R * (uint32_t)p.n_cols;
  for (uint32_t j = threadIdx.x; j < N; j += blockDim.x) {
    uint32_t sl = ~0u;
    uint64_t k = 0;
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
        }
      }
    }
    slot[j] = sl;
    key[j] = k;
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
          slot[lo] = sb;
          slot[hi] = sa;
          key[lo] = kb;
          key[hi] = ka;
        }
      }
      __syncthreads();
    }
  const double nan = __builtin_nan("");
  for (uint32_t j = threadIdx.x; j < R * nb; j += blockDim.x) {
    const int64_t row = row_base + j / nb;
    if (row >= p.n_rows) break;
    uint32_t a = 0, e = N;  // the first pair of slot j
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
    const uint64_t n = c - a;
    for (int t = 0; t < st.G; ++t) {
      double r = nan;
      if (n) {
        const double vi = q_virtual(st.method, n, st.q[t]);
        const uint64_t rk = q_rank(st.method, n, vi);
        const double va = extrema_value64(key[a + rk]);
        const double vb = q_lerps(st.method) && rk + 1 < n ? extrema_value64(key[a + rk + 1]) : va;
        r = q_value(st.method, n, vi, va, vb);
      }
      st.out[((int64_t)(st.qi0 + t) * st.n_rows_total + p.row0 + row) * (int64_t)nb + (j % nb)] = r;
    }
  }
}

// ---- host side: the steps the driver shares with the weighted one (xhist_quantile_w.hip) ------------------------------------
// Templates over the launch-parameter type P (Params, or WParams for the weighted kernels), as launch_values_pass<P> is.

// a quantile driver's call: the caller's record with the driver's own copy of the plan (its lds_max less the launch header
// q_hdr(), static LDS next to the dynamic slots), and the quantiles; `third` the weights (nullptr: the unweighted statistic)
struct QuantileCall : ValuesCall {
  const double* q;
  int n_q;
  QuantileCall(const ValuesCall& k, const double* q, int n_q) : ValuesCall(k), q(q), n_q(n_q) { pl.lds_max -= 64; }
  // the statistic in error messages
  const char* name() const { return third ? "weighted quantile" : "quantile"; }
  const char* lds_what() const {
    return third ? "weighted quantile: setting the dynamic LDS size failed" : "quantile: setting the dynamic LDS size failed";
  }
};

// one binning pass of the radix family: the choice, the geometry and the kernel
template <class P>
struct Pass {
  ValuesChoice c;
  ValuesGeometry g;
  void (*fn)(const P) = nullptr;
};

// the pass of kernel set K with `slot` bytes of LDS per bin, over chunks of `rows` rows
template <class K, class P>
static int pick_pass(Pass<P>& ps, const QuantileCall& k, size_t slot, int64_t rows, const char* what) {
  const ValuesSlots sl = {{slot, 0}, {slot, 0}, false};
  ps.c = choose_values(k, sl);
  ps.fn = pick_values_kernel<K>(ps.c, k.pl);
  if (!ps.fn) return k.fail(XHIST_ERR_HIP, "internal: no %s %s kernel for this combination", k.name(), what);
  ps.g = values_geometry(k.pl, ps.c, rows, k.n_cols);
  return allow_values_lds(k, ps.fn, ps.c.lds_bytes[0], k.lds_what());
}

// One binning pass over rows [r0, r0 + nr) of a chunk: `recs` the launch's records (Params::out), `tgt` the targets of
// `tgt_bytes` each (w2_ptr; nullptr: the pass reads none), `flag` its flag word, T records or targets per bin, digits of d bits.
template <class P>
static int launch_quantile_pass(const Pass<P>& ps, const QuantileCall& k, int64_t r0, int64_t nr, void* recs, size_t rec_row_bytes,
                                const void* tgt, size_t tgt_bytes, uint32_t* flag, int T, int d, const char* what) {
  for (int64_t i = 0; i < nr; i += ps.g.max_rows) {
    const int64_t n = std::min(ps.g.max_rows, nr - i);
    P kp;
    static_cast<Params&>(kp) = values_params(k, ps.c, ps.g.segs, r0 + i, n);
    if constexpr (std::is_same<P, WParams>::value) weights_params(kp, k.third);
    kp.out = static_cast<char*>(recs) + i * rec_row_bytes;
    kp.w2_ptr = reinterpret_cast<const uint64_t*>(tgt ? static_cast<const char*>(tgt) + i * k.pl.n_bins * T * tgt_bytes : nullptr);
    kp.part_counts = flag;
    kp.n_parts = T;
    kp.part_shift = d;
    XH_VALUES_LAUNCH(ps.fn, dim3((unsigned)(n * ps.g.segs)), dim3(ps.g.block), ps.c.lds_bytes[0], k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, what);
  }
  return XHIST_OK;
}

// the targets of one group of a step struct (QStep, QWStep): q[g0 .. g0 + G), at most G of them
template <class Step>
static void quantile_group(Step& st, const QuantileCall& k, int g0, int G) {
  st.qi0 = g0;
  st.G = std::min(G, k.n_q - g0);
  for (int t = 0; t < st.G; ++t) st.q[t] = k.q[g0 + t];
}

// The radix family's group size G and digit width d, the digit passes of a group, and the rows of a chunk.  (G, d): the fewest
// streaming passes, groups x ceil(64 / d) (ties: the wider d), first over the (G, d) whose digit pass takes at most
// kQLdsBudget of LDS, then over those that fit LDS at all, both with d >= 4; if none does, counters (sums) in global memory,
// under the scratch cap.  digit_bytes(G, d): a bin's LDS slots in a digit pass; radix_row_bytes(bins, G, d): the scratch of
// one row of a chunk.
struct QRadix {
  int G = 0, d = 0, passes = 0;
  int64_t chunk = 0;
};
static inline QRadix quantile_radix(const QuantileCall& k, size_t (*digit_bytes)(int, int), size_t (*radix_row_bytes)(int64_t, int, int)) {
  QRadix r;
  int64_t best = INT64_MAX;
  for (int tier = 0; tier < 3 && !r.G; ++tier) {
    for (int g = std::min(kQGroup, k.n_q); g >= 1; --g)
      for (int dd = 8; dd >= (tier < 2 ? 4 : 1); --dd) {
        const int64_t cost = (int64_t)((k.n_q + g - 1) / g) * ((64 + dd - 1) / dd);
        if (cost >= best) continue;
        if (radix_row_bytes(k.pl.n_bins, g, dd) > kQScratchCap && !(g == 1 && dd == 1)) continue;
        const ValuesSlots sl = {{digit_bytes(g, dd), 0}, {digit_bytes(g, dd), 0}, false};
        const ValuesChoice c = choose_values(k, sl);
        if (c.lds != (tier < 2) || (tier == 0 && c.lds_bytes[0] > kQLdsBudget)) continue;
        best = cost;
        r.G = g;
        r.d = dd;
      }
  }
  r.passes = (64 + r.d - 1) / r.d;
  r.chunk = std::max<int64_t>(1, std::min<int64_t>(k.n_rows, (int64_t)(kQScratchCap / radix_row_bytes(k.pl.n_bins, r.G, r.d))));
  return r;
}

// the radix family's describe() line (`name`: quantile / weighted_quantile); `succ`: the unweighted family's successor pass
// (nullptr: the statistic has none), appended as successor=<family>/<home>/<lds_bytes>
template <class P>
static void describe_quantile_radix(const char* name, const QuantileCall& k, const QRadix& r, const Pass<P>& win0, const Pass<P>& digit,
                                    const Pass<P>* succ = nullptr) {
  auto fam = [](const Pass<P>& p) { return p.c.fast ? "fast" : "generic"; };
  auto home = [](const Pass<P>& p) { return p.c.lds ? "lds" : "global"; };
  const int n = snprintf(k.desc, k.desc_cap,
                         "%s family=radix window=%s/%s digits=%s/%s scan=%d/%d d=%d group=%d groups=%d passes=%d chunks=%lld "
                         "rows_per_chunk=%lld block=%d segs=%lld lds_bytes=%zu/%zu D=%d cmp=%d",
                         name, fam(win0), home(win0), fam(digit), home(digit), win0.c.scan, digit.c.scan, r.d, r.G,
                         (k.n_q + r.G - 1) / r.G, r.passes, (long long)((k.n_rows + r.chunk - 1) / r.chunk), (long long)r.chunk,
                         digit.g.block, (long long)digit.g.segs, win0.c.lds_bytes[0], digit.c.lds_bytes[0], k.pl.n_dims,
                         values_cmp(k.pl));
  if (succ && n > 0 && (size_t)n < k.desc_cap)
    snprintf(k.desc + n, k.desc_cap - n, " successor=%s/%s/%zu", fam(*succ), home(*succ), succ->c.lds_bytes[0]);
}

// The short-row family's launches: R whole rows per workgroup of 256 lanes (at most `short_cols` values in all, and R x bins
// slots below 2^32), N the power of two above R x n_cols sorted elements of `elem_bytes` bytes of LDS each; per group of
// targets, row chunks below 2^31 workgroups.  `fn`: the kernel for the compare domains 0, 1 and 3.
struct QShort {
  int64_t R = 0;
  uint32_t N = 2;
  size_t lds = 0;
};
template <class P, class Step>
static int launch_quantile_short(const QuantileCall& k, void (*const (&fn)[3])(const P, const Step), Step& st, int short_cols,
                                 size_t elem_bytes, QShort& sh) {
  const int64_t R = std::max<int64_t>(1, std::min<int64_t>(short_cols / std::max<int64_t>(k.n_cols, 1), (((int64_t)1 << 32) - 2) / k.pl.n_bins));
  uint32_t N = 2;
  while (N < (uint32_t)(R * k.n_cols)) N <<= 1;
  const size_t lds = (size_t)N * elem_bytes;
  sh = QShort{R, N, lds};
  if (lds > 48 * 1024) return values_error(k, k.third ? "internal: weighted short-row LDS" : "internal: short-row LDS", hipErrorInvalidValue);
  const int cmp = values_cmp(k.pl);
  const auto short_fn = fn[cmp == 0 ? 0 : cmp == 1 ? 1 : 2];
  const int64_t max_wg = ((int64_t)1 << 31) - 1;
  for (int g0 = 0; g0 < k.n_q; g0 += kQGroup) {
    quantile_group(st, k, g0, kQGroup);
    for (int64_t r0 = 0; r0 < k.n_rows; r0 += max_wg * R) {
      const int64_t nr = std::min(max_wg * R, k.n_rows - r0);
      ValuesChoice c;
      c.tab = &k.pl.native;
      P kp;
      static_cast<Params&>(kp) = values_params(k, c, 1, r0, nr);
      if constexpr (std::is_same<P, WParams>::value) weights_params(kp, k.third);
      kp.tables_in_lds = 0;  // (the tables are read through L2)
      kp.lane_rows = (int32_t)R;
      kp.slice_n = (int32_t)N;
      XH_VALUES_LAUNCH(short_fn, dim3((unsigned)((nr + R - 1) / R)), dim3(256), lds, k.stream, kp, st);
      XH_VALUES_LAUNCH_CHECK(k, k.third ? "qw_short launch" : "q_short launch");
    }
  }
  return XHIST_OK;
}

}  // namespace xhist
