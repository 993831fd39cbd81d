// xhist_quantile.hip — exact per-bin quantiles (histogram_quantile): the kernels of xhist_quantile.hip.h, instantiated here and
// nowhere else, the steps between the binning passes, and the driver: the list of its passes, with the successor window pass
// and the method.  The host steps it shares with the weighted driver (picking and launching a pass, the (G, d) search, the
// short-row launches, the radix describe() line) are the templates at the end of xhist_quantile.hip.h; the choice and the
// binning geometry: xhist_values.hip.h.
//
// Instantiations (36 binning kernels + 3 short-row kernels + 4):
//   q_win_fast<ST, D, SCAN>, q_digit_fast<ST, D, SCAN>      ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith      12 + 12
//   q_win_generic<CMP, LDS>, q_digit_generic<CMP, LDS>      CMP 0 / 1 / 3, slots in LDS or counts in global memory     6 + 6
//   q_short<CMP>                                            CMP 0 / 1 / 3                                               3
//   q_window, q_init, q_select, q_finalize                                                                              4
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_quantile.hip.h"

using namespace xhist;

namespace xhist {

// the windows of one chunk: pass 0's full window (mode 0, records [rows, bins]), or each target's successor window (mode 1,
// records [rows, bins, G]): (key, ~0] where the method needs rank r + 1 and it is not the target's own key, else empty
__global__ void __launch_bounds__(256) q_window(const QStep s, int mode) {
  const int64_t n = mode ? s.rows * s.bins * s.G : s.rows * s.bins;
  QWin* w = mode ? s.win : s.win0;
  uint32_t* flag = s.flags + (mode ? 2 + s.pass : 0);  // (mode 1: s.pass = the number of digit passes)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0ull, hi = ~0ull;
    if (mode) {
      const QTgt t = s.tgt[i];
      const bool open = (t.flags & kQNeedNext) && t.k + 1 >= t.m;
      lo = open ? t.pre + 1 : ~0ull;
      hi = open ? ~0ull : 0ull;
      if (open) *flag = 1u;
    } else if (i == 0) {
      *flag = 1u;
    }
    w[i] = QWin{lo, hi, 0ull, ~0ull, 0ull};
  }
}

// pass 0 -> the targets of group s.qi0 .. s.qi0 + G - 1: rank, prefix, settled at once where the bin is empty or constant
__global__ void __launch_bounds__(256) q_init(const QStep s) {
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % s.G);
    const QWin w = s.win0[i / s.G];
    QTgt x;
    x.n = w.n;
    x.m = w.n;
    x.k = 0;
    x.flags = 0;
    x.pre = w.mn;
    x.nfix = 64;
    if (w.n) {
      const double vi = q_virtual(s.method, w.n, s.q[t]);
      x.k = q_rank(s.method, w.n, vi);
      x.flags = q_lerps(s.method) && vi < (double)(w.n - 1) ? kQNeedNext : 0u;
      if (w.mn != w.mx) {
        x.nfix = (uint32_t)__builtin_clzll(w.mn ^ w.mx);
        x.pre = w.mn & q_himask(x.nfix);
        s.flags[1] = 1u;
      }
    }
    s.tgt[i] = x;
  }
}

// after digit pass s.pass: each active target takes the digit that holds its remaining rank, and zeroes its counters
__global__ void __launch_bounds__(256) q_select(const QStep s) {
  if (!*reinterpret_cast<const volatile uint32_t*>(s.flags + 1 + s.pass)) return;
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    QTgt x = s.tgt[i];
    if (x.nfix >= 64) continue;
    const uint32_t left = 64u - x.nfix, dd = left < (uint32_t)s.d ? left : (uint32_t)s.d;
    unsigned long long* c = s.cnt + (i << s.d);
    uint64_t below = 0, dig = 0, m = 0;
    bool found = false;
    for (uint32_t j = 0; j < (1u << dd); ++j) {
      const uint64_t cj = c[j];
      c[j] = 0ull;
      if (found) continue;
      if (below + cj > x.k) {
        dig = j;
        m = cj;
        found = true;
      } else {
        below += cj;
      }
    }
    x.k -= below;
    x.m = m;
    x.nfix += dd;
    x.pre |= dig << (64u - x.nfix);
    if (x.nfix < 64) s.flags[2 + s.pass] = 1u;
    s.tgt[i] = x;
  }
}

// the targets and the successor windows -> numpy's value of each, into out[qi0 + t, row0 + row, bin]
__global__ void __launch_bounds__(256) q_finalize(const QStep s) {
  const int64_t n = s.rows * s.bins * s.G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % s.G);
    const int64_t rb = i / s.G, row = rb / s.bins, b = rb % s.bins;
    const QTgt x = s.tgt[i];
    double r = __builtin_nan("");
    if (x.n) {
      const double vi = q_virtual(s.method, x.n, s.q[t]);
      const double a = extrema_value64(x.pre);
      const double b2 = (x.flags & kQNeedNext) && x.k + 1 >= x.m ? extrema_value64(s.win[i].mn) : a;
      r = q_value(s.method, x.n, vi, a, b2);
    }
    s.out[((int64_t)(s.qi0 + t) * s.n_rows_total + s.row0 + row) * s.bins + b] = r;
  }
}

}  // namespace xhist

// the binning kernels of each pass, for pick_values_kernel
struct QWinKernels {
  template <typename ST, int D, int SCAN>
  static values_fn fast() { return q_win_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_fn generic() { return q_win_generic<CMP, LDS>; }
};
struct QDigitKernels {
  template <typename ST, int D, int SCAN>
  static values_fn fast() { return q_digit_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_fn generic() { return q_digit_generic<CMP, LDS>; }
};

namespace {

// LDS bytes of a bin's slots: the window policy with T windows, the digit policy with T targets of 2^d counters
size_t win_bytes(int T) { return (size_t)T * 36; }
size_t digit_bytes(int G, int d) { return (size_t)G * (24 + ((size_t)4 << d)); }
// the radix family's scratch per row of a chunk: pass 0's windows, and per target its state, its window and its counters
size_t radix_row_bytes(int64_t bins, int G, int d) { return (size_t)bins * (sizeof(QWin) + (size_t)G * (sizeof(QTgt) + sizeof(QWin) + ((size_t)8 << d))); }

constexpr void (*kShortKernels[3])(const Params, const QStep) = {q_short<0>, q_short<1>, q_short<3>};

}  // namespace

int xhist_quantile_run(const ValuesCall& call, const double* q, int n_q, int method, double* out) {
  const QuantileCall k(call, q, n_q);
  const ValuesPlan& pl = k.pl;
  const int64_t bins = pl.n_bins, n_rows = k.n_rows;
  const hipStream_t stream = k.stream;
  QStep st;
  memset(&st, 0, sizeof st);
  st.bins = bins;
  st.n_rows_total = n_rows;
  st.method = method;
  st.out = out;

  // ---- short rows: one workgroup sorts whole rows in LDS -------------------------------------------------------------------
  if (k.n_cols <= kQShortCols) {
    QShort sh;
    if (int rc = launch_quantile_short(k, kShortKernels, st, kQShortCols, 12, sh)) return rc;
    k.describe("quantile family=short rows_per_wg=%lld pairs=%u lds_bytes=%zu groups=%d block=256 D=%d cmp=%d", (long long)sh.R, sh.N,
               sh.lds, (n_q + kQGroup - 1) / kQGroup, pl.n_dims, values_cmp(pl));
    return XHIST_OK;
  }

  // ---- long rows: radix select -------------------------------------------------------------------------------------------
  const QRadix r = quantile_radix(k, digit_bytes, radix_row_bytes);
  const int G = r.G, d = r.d, passes = r.passes;
  Pass<Params> digit, win0, winG;
  if (int rc = pick_pass<QDigitKernels>(digit, k, digit_bytes(G, d), r.chunk, "digit")) return rc;
  if (int rc = pick_pass<QWinKernels>(win0, k, win_bytes(1), r.chunk, "window")) return rc;
  if (int rc = pick_pass<QWinKernels>(winG, k, win_bytes(G), r.chunk, "window")) return rc;

  const size_t n_rb = (size_t)r.chunk * bins;
  QWin* w0 = static_cast<QWin*>(k.scratch(n_rb * sizeof(QWin)));
  QWin* wg = static_cast<QWin*>(k.scratch(n_rb * G * sizeof(QWin)));
  QTgt* tg = static_cast<QTgt*>(k.scratch(n_rb * G * sizeof(QTgt)));
  unsigned long long* cnt = static_cast<unsigned long long*>(k.scratch((n_rb * G << d) * 8));
  uint32_t* flags = static_cast<uint32_t*>(k.scratch(8 * ((size_t)passes + 8)));
  if (!w0 || !wg || !tg || !cnt || !flags)
    return k.fail(XHIST_ERR_NOMEM, "allocation of the quantile scratch (%zu bytes per chunk) failed", radix_row_bytes(bins, G, d) * r.chunk);
  const int64_t n_flag_words = (3 + passes + 1) / 2;  // flags: [0] pass 0, [1 + j] digit pass j, [2 + passes] the successor
  XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(2048), dim3(256), 0, stream, cnt, (int64_t)(n_rb * G << d));
  XH_VALUES_LAUNCH_CHECK(k, "quantile zeroing launch");
  st.tgt = tg;
  st.win0 = w0;
  st.win = wg;
  st.cnt = cnt;
  st.flags = flags;
  st.d = d;
  for (int64_t r0 = 0; r0 < n_rows; r0 += r.chunk) {
    const int64_t nr = std::min(r.chunk, n_rows - r0);
    st.rows = nr;
    st.row0 = r0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (nr * bins * G + 255) / 256));
    XH_VALUES_LAUNCH(q_window, dim3(grid), dim3(256), 0, stream, st, 0);
    XH_VALUES_LAUNCH_CHECK(k, "q_window launch");
    if (int rc = launch_quantile_pass(win0, k, r0, nr, w0, bins * sizeof(QWin), nullptr, 0, flags, 1, d, "quantile window launch"))
      return rc;
    for (int g0 = 0; g0 < n_q; g0 += G) {
      quantile_group(st, k, g0, G);
      // the flags of the digit passes and of the successor start at zero for every group (pass 0 has run: its flag may go too)
      XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(1), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(flags), n_flag_words);
      XH_VALUES_LAUNCH_CHECK(k, "quantile zeroing launch");
      XH_VALUES_LAUNCH(q_init, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK(k, "q_init launch");
      for (int j = 0; j < passes; ++j) {
        st.pass = j;
        if (int rc = launch_quantile_pass(digit, k, r0, nr, cnt, ((size_t)bins * st.G * 8) << d, tg, sizeof(QTgt), flags + 1 + j, st.G, d,
                                          "quantile digit launch"))
          return rc;
        XH_VALUES_LAUNCH(q_select, dim3(grid), dim3(256), 0, stream, st);
        XH_VALUES_LAUNCH_CHECK(k, "q_select launch");
      }
      st.pass = passes;
      XH_VALUES_LAUNCH(q_window, dim3(grid), dim3(256), 0, stream, st, 1);
      XH_VALUES_LAUNCH_CHECK(k, "q_window launch");
      if (int rc = launch_quantile_pass(winG, k, r0, nr, wg, bins * st.G * sizeof(QWin), nullptr, 0, flags + 2 + passes, st.G, d,
                                        "quantile successor launch"))
        return rc;
      XH_VALUES_LAUNCH(q_finalize, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK(k, "q_finalize launch");
    }
  }
  describe_quantile_radix("quantile", k, r, win0, digit, &winG);
  return XHIST_OK;
}
