// xhist_quantile_w.hip — exact weighted per-bin quantiles (histogram_weighted_quantile): the kernels of
// xhist_quantile_w.hip.h, instantiated here and nowhere else, the steps between the binning passes, and the driver: the list of
// its passes, with the 2^32 records check and no successor pass.  The host steps it shares with the unweighted driver are the
// templates at the end of xhist_quantile.hip.h; the choice and the binning geometry: xhist_values.hip.h.
//
// Instantiations (36 binning kernels + 3 short-row kernels + 4):
//   qw_win_fast<ST, D, SCAN>, qw_digit_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith      12 + 12
//   qw_win_generic<CMP, LDS>, qw_digit_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   qw_short<CMP>                                           CMP 0 / 1 / 3                                               3
//   qw_window, qw_init, qw_select, qw_finalize                                                                          4
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_quantile_w.hip.h"

using namespace xhist;

namespace xhist {

// pass 0's records of one chunk, before the pass
__global__ void __launch_bounds__(256) qw_window(const QWStep s) {
  const int64_t n = s.rows * s.bins;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    s.win0[i] = QWWin{~0ull, 0ull, 0.0};
  }
}

// pass 0 -> the targets of group s.qi0 .. s.qi0 + G - 1: settled at once where the result is NaN or the bin is constant
__global__ void __launch_bounds__(256) qw_init(const QWStep s) {
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const QWWin w = s.win0[i / s.G];
    QWTgt x;
    x.pre = w.mn;
    x.below = 0.0;
    x.w = w.w;
    x.nfix = 64;
    x.flags = 0;
    if (!(w.mn <= w.mx && w.w > 0.0 && w.w < __builtin_inf())) {
      x.flags = kQWNan;
    } else if (w.mn != w.mx) {
      x.nfix = (uint32_t)__builtin_clzll(w.mn ^ w.mx);
      x.pre = w.mn & q_himask(x.nfix);
      s.flags[1] = 1u;
    }
    s.tgt[i] = x;
  }
}

// after digit pass s.pass: each active target takes the first bucket with a positive sum whose cdf value reaches q (the last
// bucket with a positive sum if none does), and zeroes its sums
__global__ void __launch_bounds__(256) qw_select(const QWStep s) {
  if (!*reinterpret_cast<const volatile uint32_t*>(s.flags + 1 + s.pass)) return;
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    QWTgt x = s.tgt[i];
    if (x.nfix >= 64) continue;
    const double q = s.q[i % s.G];
    const uint32_t left = 64u - x.nfix, dd = left < (uint32_t)s.d ? left : (uint32_t)s.d;
    double* c = s.sum + (i << s.d);
    double cum = 0.0, under = 0.0;  // the running sum, and its value before the bucket taken
    uint64_t dig = 0;
    bool found = false;
    for (uint32_t j = 0; j < (1u << dd); ++j) {
      const double cj = c[j];
      c[j] = 0.0;
      if (found || !(cj > 0.0)) continue;
      dig = j;
      under = cum;
      cum += cj;
      found = qw_reached(x.below + cum, x.w, q);
    }
    x.below += under;
    x.nfix += dd;
    x.pre |= dig << (64u - x.nfix);
    if (x.nfix < 64) s.flags[2 + s.pass] = 1u;
    s.tgt[i] = x;
  }
}

// the targets -> the value of each, into out[qi0 + t, row0 + row, bin]
__global__ void __launch_bounds__(256) qw_finalize(const QWStep s) {
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % s.G);
    const int64_t rb = i / s.G, row = rb / s.bins, b = rb % s.bins;
    const QWTgt x = s.tgt[i];
    s.out[((int64_t)(s.qi0 + t) * s.n_rows_total + s.row0 + row) * s.bins + b] =
        (x.flags & kQWNan) ? __builtin_nan("") : extrema_value64(x.pre);
  }
}

}  // namespace xhist

typedef void (*values_w_fn)(const WParams);

// the binning kernels of each pass, for pick_values_kernel
struct QWWinKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return qw_win_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return qw_win_generic<CMP, LDS>; }
};
struct QWDigitKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return qw_digit_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return qw_digit_generic<CMP, LDS>; }
};

namespace {

// LDS bytes of a bin's slots: the window policy, and the digit policy with G targets of 2^d float64 sums
constexpr size_t kWinBytes = 24;
size_t digit_bytes(int G, int d) { return (size_t)G * (24 + ((size_t)8 << d)); }
// the radix family's scratch per row of a chunk: pass 0's records, and per target its state and its sums
size_t radix_row_bytes(int64_t bins, int G, int d) { return (size_t)bins * (sizeof(QWWin) + (size_t)G * (sizeof(QWTgt) + ((size_t)8 << d))); }

constexpr void (*kShortKernels[3])(const WParams, const QWStep) = {qw_short<0>, qw_short<1>, qw_short<3>};

}  // namespace

int xhist_quantile_w_run(const ValuesCall& call, const double* q, int n_q, double* out) {
  const QuantileCall k(call, q, n_q);
  const ValuesPlan& pl = k.pl;
  const int64_t bins = pl.n_bins, n_rows = k.n_rows;
  const hipStream_t stream = k.stream;
  QWStep st;
  memset(&st, 0, sizeof st);
  st.bins = bins;
  st.n_rows_total = n_rows;
  st.out = out;

  // ---- short rows: one workgroup sorts whole rows in LDS -------------------------------------------------------------------
  if (k.n_cols <= kQWShortCols) {
    QShort sh;
    if (int rc = launch_quantile_short(k, kShortKernels, st, kQWShortCols, 20, sh)) return rc;
    k.describe("weighted_quantile family=short rows_per_wg=%lld triples=%u lds_bytes=%zu groups=%d block=256 D=%d cmp=%d", (long long)sh.R,
               sh.N, sh.lds, (n_q + kQGroup - 1) / kQGroup, pl.n_dims, values_cmp(pl));
    return XHIST_OK;
  }

  // ---- long rows: radix select, by the rule of the unweighted family over the 8-byte sums ------------------------------------
  const QRadix r = quantile_radix(k, digit_bytes, radix_row_bytes);
  const int G = r.G, d = r.d, passes = r.passes;
  if ((uint64_t)r.chunk * (uint64_t)bins >> 32)  // (the no-LDS window kernel indexes a launch's records in 32 bits)
    return k.fail(XHIST_ERR_UNSUPPORTED, "weighted quantiles of %lld bins are not supported (at most 2^32 - 1)", (long long)bins);
  Pass<WParams> digit, win0;
  if (int rc = pick_pass<QWDigitKernels>(digit, k, digit_bytes(G, d), r.chunk, "digit")) return rc;
  if (int rc = pick_pass<QWWinKernels>(win0, k, kWinBytes, r.chunk, "window")) return rc;

  const size_t n_rb = (size_t)r.chunk * bins;
  QWWin* w0 = static_cast<QWWin*>(k.scratch(n_rb * sizeof(QWWin)));
  QWTgt* tg = static_cast<QWTgt*>(k.scratch(n_rb * G * sizeof(QWTgt)));
  double* sum = static_cast<double*>(k.scratch((n_rb * G << d) * 8));
  uint32_t* flags = static_cast<uint32_t*>(k.scratch(8 * ((size_t)passes + 8)));
  if (!w0 || !tg || !sum || !flags)
    return k.fail(XHIST_ERR_NOMEM, "allocation of the weighted quantile scratch (%zu bytes per chunk) failed",
                  radix_row_bytes(bins, G, d) * r.chunk);
  const int64_t n_flag_words = (2 + passes + 1) / 2;  // flags: [1 + j] digit pass j (and the word qw_select writes last)
  XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(2048), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(sum), (int64_t)(n_rb * G << d));
  XH_VALUES_LAUNCH_CHECK(k, "weighted quantile zeroing launch");
  st.tgt = tg;
  st.win0 = w0;
  st.sum = sum;
  st.flags = flags;
  st.d = d;
  for (int64_t r0 = 0; r0 < n_rows; r0 += r.chunk) {
    const int64_t nr = std::min(r.chunk, n_rows - r0);
    st.rows = nr;
    st.row0 = r0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (nr * bins * G + 255) / 256));
    XH_VALUES_LAUNCH(qw_window, dim3(grid), dim3(256), 0, stream, st);
    XH_VALUES_LAUNCH_CHECK(k, "qw_window launch");
    if (int rc = launch_quantile_pass(win0, k, r0, nr, w0, bins * sizeof(QWWin), nullptr, 0, flags, 1, d,
                                      "weighted quantile window launch"))
      return rc;
    for (int g0 = 0; g0 < n_q; g0 += G) {
      quantile_group(st, k, g0, G);
      // the flags of the digit passes start at zero for every group
      XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(1), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(flags), n_flag_words);
      XH_VALUES_LAUNCH_CHECK(k, "weighted quantile zeroing launch");
      XH_VALUES_LAUNCH(qw_init, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK(k, "qw_init launch");
      for (int j = 0; j < passes; ++j) {
        st.pass = j;
        if (int rc = launch_quantile_pass(digit, k, r0, nr, sum, ((size_t)bins * st.G * 8) << d, tg, sizeof(QWTgt), flags + 1 + j, st.G, d,
                                          "weighted quantile digit launch"))
          return rc;
        XH_VALUES_LAUNCH(qw_select, dim3(grid), dim3(256), 0, stream, st);
        XH_VALUES_LAUNCH_CHECK(k, "qw_select launch");
      }
      XH_VALUES_LAUNCH(qw_finalize, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK(k, "qw_finalize launch");
    }
  }
  describe_quantile_radix("weighted_quantile", k, r, win0, digit);
  return XHIST_OK;
}
