// xhist_quantile.hip — exact per-bin quantiles (histogram_quantile): the kernels of xhist_quantile.hip.h, instantiated here and
// nowhere else, the steps between the binning passes, and the driver that orders their launches (the choice and the binning
// geometry: xhist_values.hip.h).
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

struct Pass {
  ValuesChoice c;
  ValuesGeometry g;
  values_fn fn = nullptr;
};

template <class K>
int pick_pass(Pass& ps, const ValuesPlan& pl, size_t slot, const xhist_array* samples, const xhist_array* values, int64_t rows,
              int64_t n_cols, const char* what, char* err, size_t err_cap) {
  const ValuesSlots sl = {{slot, 0}, {slot, 0}, false};
  ps.c = choose_values(pl, sl, samples, values, n_cols);
  ps.fn = pick_values_kernel<K>(ps.c, pl);
  if (!ps.fn) {
    snprintf(err, err_cap, "internal: no quantile %s kernel for this combination", what);
    return XHIST_ERR_HIP;
  }
  ps.g = values_geometry(pl, ps.c, rows, n_cols);
  return allow_values_lds(ps.fn, ps.c.lds_bytes[0], "quantile: setting the dynamic LDS size failed", err, err_cap);
}

// One binning pass over rows [r0, r0 + nr) of a chunk: `recs` the launch's records (Params::out), `tgt` the targets (w2_ptr),
// `flag` its flag word, T records per bin, digits of d bits.
int launch_q_pass(const Pass& ps, const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t r0, int64_t nr,
                  int64_t n_cols, void* recs, size_t rec_row_bytes, const QTgt* tgt, uint32_t* flag, int T, int d, hipStream_t stream,
                  const char* what, char* err, size_t err_cap) {
  for (int64_t k = 0; k < nr; k += ps.g.max_rows) {
    const int64_t n = std::min(ps.g.max_rows, nr - k);
    Params kp = values_params(pl, ps.c, ps.g.segs, samples, values, r0 + k, n, n_cols);
    kp.out = static_cast<char*>(recs) + k * rec_row_bytes;
    kp.w2_ptr = reinterpret_cast<const uint64_t*>(tgt ? tgt + k * pl.n_bins * T : nullptr);
    kp.part_counts = flag;
    kp.n_parts = T;
    kp.part_shift = d;
    XH_VALUES_LAUNCH(ps.fn, dim3((unsigned)(n * ps.g.segs)), dim3(ps.g.block), ps.c.lds_bytes[0], stream, kp);
    XH_VALUES_LAUNCH_CHECK(what);
  }
  return XHIST_OK;
}

}  // namespace

int xhist_quantile_run(const ValuesPlan& pl_in, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                       const double* q, int n_q, int method, double* out, xhist_quantile_alloc_fn alloc, void* alloc_ctx,
                       hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap) {
  ValuesPlan pl = pl_in;
  pl.lds_max -= 64;  // (the launch header q_hdr() is static LDS next to the dynamic slots)
  const int64_t bins = pl.n_bins;
  const int cmp = values_cmp(pl);
  QStep st;
  memset(&st, 0, sizeof st);
  st.bins = bins;
  st.n_rows_total = n_rows;
  st.method = method;
  st.out = out;

  // ---- short rows: one workgroup sorts whole rows in LDS -------------------------------------------------------------------
  if (n_cols <= kQShortCols) {
    const int64_t R = std::max<int64_t>(1, std::min<int64_t>(kQShortCols / std::max<int64_t>(n_cols, 1), (((int64_t)1 << 32) - 2) / bins));
    uint32_t N = 2;
    while (N < (uint32_t)(R * n_cols)) N <<= 1;
    const size_t lds = (size_t)N * 12;
    if (lds > 48 * 1024) return values_error(err, err_cap, XHIST_ERR_HIP, "internal: short-row LDS", hipErrorInvalidValue);
    const int64_t max_wg = ((int64_t)1 << 31) - 1;
    for (int g0 = 0; g0 < n_q; g0 += kQGroup) {
      st.qi0 = g0;
      st.G = std::min(kQGroup, n_q - g0);
      for (int t = 0; t < st.G; ++t) st.q[t] = q[g0 + t];
      for (int64_t r0 = 0; r0 < n_rows; r0 += max_wg * R) {
        const int64_t nr = std::min(max_wg * R, n_rows - r0);
        ValuesChoice c;
        c.tab = &pl.native;
        Params kp = values_params(pl, c, 1, samples, values, r0, nr, n_cols);
        kp.tables_in_lds = 0;  // (the tables are read through L2)
        kp.lane_rows = (int32_t)R;
        kp.slice_n = (int32_t)N;
        const dim3 grid((unsigned)((nr + R - 1) / R));
        if (cmp == 0) XH_VALUES_LAUNCH(q_short<0>, grid, dim3(256), lds, stream, kp, st);
        else if (cmp == 1) XH_VALUES_LAUNCH(q_short<1>, grid, dim3(256), lds, stream, kp, st);
        else XH_VALUES_LAUNCH(q_short<3>, grid, dim3(256), lds, stream, kp, st);
        XH_VALUES_LAUNCH_CHECK("q_short launch");
      }
    }
    if (desc && desc_cap)
      snprintf(desc, desc_cap, "quantile family=short rows_per_wg=%lld pairs=%u lds_bytes=%zu groups=%d block=256 D=%d cmp=%d",
               (long long)R, N, lds, (n_q + kQGroup - 1) / kQGroup, pl.n_dims, cmp);
    return XHIST_OK;
  }

  // ---- long rows: radix select -------------------------------------------------------------------------------------------
  // The group size G and the digit width d: the fewest streaming passes, groups x ceil(64 / d) (ties: the wider d), first
  // over the (G, d) whose digit pass takes at most kQLdsBudget of LDS, then over those that fit LDS at all, both with d >= 4;
  // if none does, counters in global memory, under the scratch cap.
  int G = 0, d = 0;
  int64_t best = INT64_MAX;
  for (int tier = 0; tier < 3 && !G; ++tier) {
    for (int g = std::min(kQGroup, n_q); g >= 1; --g)
      for (int dd = 8; dd >= (tier < 2 ? 4 : 1); --dd) {
        const int64_t cost = (int64_t)((n_q + g - 1) / g) * ((64 + dd - 1) / dd);
        if (cost >= best) continue;
        if (radix_row_bytes(bins, g, dd) > kQScratchCap && !(g == 1 && dd == 1)) continue;
        const ValuesSlots sl = {{digit_bytes(g, dd), 0}, {digit_bytes(g, dd), 0}, false};
        const ValuesChoice c = choose_values(pl, sl, samples, values, n_cols);
        if (c.lds != (tier < 2) || (tier == 0 && c.lds_bytes[0] > kQLdsBudget)) continue;
        best = cost;
        G = g;
        d = dd;
      }
  }
  Pass digit;
  const int passes = (64 + d - 1) / d;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_rows, (int64_t)(kQScratchCap / radix_row_bytes(bins, G, d))));
  Pass win0, winG;
  if (int rc = pick_pass<QDigitKernels>(digit, pl, digit_bytes(G, d), samples, values, chunk, n_cols, "digit", err, err_cap)) return rc;
  if (int rc = pick_pass<QWinKernels>(win0, pl, win_bytes(1), samples, values, chunk, n_cols, "window", err, err_cap)) return rc;
  if (int rc = pick_pass<QWinKernels>(winG, pl, win_bytes(G), samples, values, chunk, n_cols, "window", err, err_cap)) return rc;

  const size_t n_rb = (size_t)chunk * bins;
  QWin* w0 = static_cast<QWin*>(alloc(alloc_ctx, n_rb * sizeof(QWin)));
  QWin* wg = static_cast<QWin*>(alloc(alloc_ctx, n_rb * G * sizeof(QWin)));
  QTgt* tg = static_cast<QTgt*>(alloc(alloc_ctx, n_rb * G * sizeof(QTgt)));
  unsigned long long* cnt = static_cast<unsigned long long*>(alloc(alloc_ctx, (n_rb * G << d) * 8));
  uint32_t* flags = static_cast<uint32_t*>(alloc(alloc_ctx, 8 * ((size_t)passes + 8)));
  if (!w0 || !wg || !tg || !cnt || !flags) {
    snprintf(err, err_cap, "allocation of the quantile scratch (%zu bytes per chunk) failed", radix_row_bytes(bins, G, d) * chunk);
    return XHIST_ERR_NOMEM;
  }
  const int64_t n_flag_words = (3 + passes + 1) / 2;  // flags: [0] pass 0, [1 + j] digit pass j, [2 + passes] the successor
  hipLaunchKernelGGL(zero_words, dim3(2048), dim3(256), 0, stream, cnt, (int64_t)(n_rb * G << d));
  XH_VALUES_LAUNCH_CHECK("quantile zeroing launch");
  st.tgt = tg;
  st.win0 = w0;
  st.win = wg;
  st.cnt = cnt;
  st.flags = flags;
  st.d = d;
  for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
    const int64_t nr = std::min(chunk, n_rows - r0);
    st.rows = nr;
    st.row0 = r0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (nr * bins * G + 255) / 256));
    XH_VALUES_LAUNCH(q_window, dim3(grid), dim3(256), 0, stream, st, 0);
    XH_VALUES_LAUNCH_CHECK("q_window launch");
    if (int rc = launch_q_pass(win0, pl, samples, values, r0, nr, n_cols, w0, bins * sizeof(QWin), nullptr, flags, 1, d, stream,
                               "quantile window launch", err, err_cap))
      return rc;
    for (int g0 = 0; g0 < n_q; g0 += G) {
      st.qi0 = g0;
      st.G = std::min(G, n_q - g0);
      for (int t = 0; t < st.G; ++t) st.q[t] = q[g0 + t];
      // the flags of the digit passes and of the successor start at zero for every group (pass 0 has run: its flag may go too)
      hipLaunchKernelGGL(zero_words, dim3(1), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(flags), n_flag_words);
      XH_VALUES_LAUNCH_CHECK("quantile zeroing launch");
      XH_VALUES_LAUNCH(q_init, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK("q_init launch");
      for (int j = 0; j < passes; ++j) {
        st.pass = j;
        if (int rc = launch_q_pass(digit, pl, samples, values, r0, nr, n_cols, cnt, ((size_t)bins * st.G * 8) << d, tg, flags + 1 + j,
                                   st.G, d, stream, "quantile digit launch", err, err_cap))
          return rc;
        XH_VALUES_LAUNCH(q_select, dim3(grid), dim3(256), 0, stream, st);
        XH_VALUES_LAUNCH_CHECK("q_select launch");
      }
      st.pass = passes;
      XH_VALUES_LAUNCH(q_window, dim3(grid), dim3(256), 0, stream, st, 1);
      XH_VALUES_LAUNCH_CHECK("q_window launch");
      if (int rc = launch_q_pass(winG, pl, samples, values, r0, nr, n_cols, wg, bins * st.G * sizeof(QWin), nullptr, flags + 2 + passes,
                                 st.G, d, stream, "quantile successor launch", err, err_cap))
        return rc;
      XH_VALUES_LAUNCH(q_finalize, dim3(grid), dim3(256), 0, stream, st);
      XH_VALUES_LAUNCH_CHECK("q_finalize launch");
    }
  }
  if (desc && desc_cap) {
    auto fam = [](const Pass& p) { return p.c.fast ? "fast" : "generic"; };
    auto home = [](const Pass& p) { return p.c.lds ? "lds" : "global"; };
    snprintf(desc, desc_cap,
             "quantile family=radix window=%s/%s digits=%s/%s scan=%d/%d d=%d group=%d groups=%d passes=%d chunks=%lld rows_per_chunk=%lld "
             "block=%d segs=%lld lds_bytes=%zu/%zu D=%d cmp=%d",
             fam(win0), home(win0), fam(digit), home(digit), win0.c.scan, digit.c.scan, d, G, (n_q + G - 1) / G, passes,
             (long long)((n_rows + chunk - 1) / chunk), (long long)chunk, digit.g.block, (long long)digit.g.segs, win0.c.lds_bytes[0],
             digit.c.lds_bytes[0], pl.n_dims, cmp);
  }
  return XHIST_OK;
}
