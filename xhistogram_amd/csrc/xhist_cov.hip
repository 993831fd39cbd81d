// xhist_cov.hip — per-bin count, means, variances and covariance of two value arrays (histogram_cov): the kernels of
// xhist_cov.hip.h, instantiated here and nowhere else, the steps between and after the two passes, and the driver (the choice
// and the binning launches themselves: xhist_values.hip.h).
//
// Instantiations (36 binning kernels + 2):
//   cov_sum_fast<ST, D, SCAN>, cov_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   cov_sum_generic<CMP, LDS>, cov_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   cov_mean, cov_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_cov.hip.h"

using namespace xhist;

namespace xhist {

// the sums of pass 1 -> both means, in place: S / n, NaN where no pair arrived; `sum` is [2, n]
__global__ void __launch_bounds__(256) cov_mean(const unsigned long long* cnt, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    sum[i] = c ? sum[i] / (double)c : nan;
    sum[n + i] = c ? sum[n + i] / (double)c : nan;
  }
}

// the sums of pass 2 -> M2_a, C_ab, M2_b, in place in `co` [3, n]; `sd` is [2, n].  The M2 are clamped at 0, the co-moment is
// not; NaN where no pair arrived, and NaN stays NaN
__global__ void __launch_bounds__(256) cov_finalize(const unsigned long long* cnt, const double* sd, double* co, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    if (!c) {
      co[i] = co[n + i] = co[2 * n + i] = nan;
      continue;
    }
    const double sa = sd[i], sb = sd[n + i];
    const double ra = co[i] - sa * sa / (double)c;
    const double rb = co[2 * n + i] - sb * sb / (double)c;
    co[i] = ra <= 0.0 ? 0.0 : ra;
    co[n + i] = co[n + i] - sa * sb / (double)c;
    co[2 * n + i] = rb <= 0.0 ? 0.0 : rb;
  }
}

}  // namespace xhist

typedef void (*cov_fn)(const CovParams);

// the binning kernels of each pass, for pick_values_kernel
struct CovSumKernels {
  template <typename ST, int D, int SCAN>
  static cov_fn fast() { return cov_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_fn generic() { return cov_sum_generic<CMP, LDS>; }
};
struct CovDevKernels {
  template <typename ST, int D, int SCAN>
  static cov_fn fast() { return cov_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static cov_fn generic() { return cov_dev_generic<CMP, LDS>; }
};

// pass 1's count and two sums, pass 2's two means and five sums, whatever the type of the values; pass 2's slot decides for both
static constexpr ValuesSlots kCovSlots = {{sizeof(CovSumSlot), sizeof(CovDevSlot)}, {sizeof(CovSumSlot), sizeof(CovDevSlot)}, true};

// The zeroing and the five launches on `stream` (pass 1, means, pass 2, finalize), as meanvar_run (xhist_meanvar.hip.h) with
// the second value array in the place of the weights and outputs of several planes.
int xhist_cov_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values_a, const xhist_array* values_b,
                  int64_t n_rows, int64_t n_cols, int64_t* out_count, double* out_mean, double* out_comoment, double* sd,
                  hipStream_t stream, char* err, size_t err_cap, char* desc, size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out_count);
  const struct {
    void* p;
    int planes;
  } zero[4] = {{cnt, 1}, {out_mean, 2}, {out_comoment, 3}, {sd, 2}};
  for (const auto& z : zero) {
    hipLaunchKernelGGL(zero_words, dim3(grid_io), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(z.p), z.planes * n_out);
    XH_VALUES_LAUNCH_CHECK("cov zeroing launch");
  }

  ValuesChoice c;
  ValuesGeometry g;
  cov_fn sum = nullptr, dev = nullptr;
  if (n_cols > 0) {
    c = choose_values(pl, kCovSlots, samples, values_a, n_cols, values_b);
    sum = pick_values_kernel<CovSumKernels>(c, pl);
    dev = pick_values_kernel<CovDevKernels>(c, pl);
    if (!sum || !dev) {
      snprintf(err, err_cap, "internal: no cov kernel for this combination");
      return XHIST_ERR_HIP;
    }
    for (int k = 0; k < 2; ++k)
      if (int rc = allow_values_lds(k ? dev : sum, c.lds_bytes[k], "cov: setting the dynamic LDS size failed", err, err_cap)) return rc;
    g = values_geometry(pl, c, n_rows, n_cols);
    if (int rc = launch_values_pass(sum, c.lds_bytes[0], "cov_sum launch", pl, c, g, samples, values_a, n_rows, n_cols, cnt, out_mean,
                                    nullptr, stream, err, err_cap, values_b))
      return rc;
  }
  XH_VALUES_LAUNCH(cov_mean, dim3(grid_io), dim3(256), 0, stream, cnt, out_mean, n_out);
  XH_VALUES_LAUNCH_CHECK("cov_mean launch");
  if (n_cols > 0) {
    if (int rc = launch_values_pass(dev, c.lds_bytes[1], "cov_dev launch", pl, c, g, samples, values_a, n_rows, n_cols, sd, out_comoment,
                                    out_mean, stream, err, err_cap, values_b))
      return rc;
  }
  XH_VALUES_LAUNCH(cov_finalize, dim3(grid_io), dim3(256), 0, stream, cnt, sd, out_comoment, n_out);
  XH_VALUES_LAUNCH_CHECK("cov_finalize launch");
  if (desc && desc_cap) {
    const char* fam = !sum ? "none" : c.fast ? "fast" : "generic";
    const char* home = !sum ? "none" : c.lds ? "lds" : "global";
    snprintf(desc, desc_cap,
             "cov pass1=cov_sum_%s slots=%s pass2=cov_dev_%s slots=%s scan=%d copies=%d block=%d segs=%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d cmp=%d",
             fam, home, fam, home, c.scan, 1 << c.copies_log2, g.block, (long long)g.segs, c.lds_bytes[0], c.lds_bytes[1],
             (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  return XHIST_OK;
}
