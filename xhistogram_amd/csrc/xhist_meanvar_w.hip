// xhist_meanvar_w.hip — per-bin sum of weights, weighted mean and variance (histogram_mean_var with weights): the weighted
// kernels of xhist_meanvar.hip.h, instantiated here and nowhere else, the steps between and after the two passes, and the
// driver that orders their launches (the choice and the binning launches themselves: xhist_values.hip.h).
//
// Instantiations (36 binning kernels + 2):
//   mvw_sum_fast<ST, D, SCAN>, mvw_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mvw_sum_generic<CMP, LDS>, mvw_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   mvw_mean, mvw_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

using namespace xhist;

namespace xhist {

// the weighted sums of pass 1 -> means, in place: S / W, NaN where W == 0 (a NaN W gives NaN)
__global__ void __launch_bounds__(256) mvw_mean(const double* wsum, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    sum[i] = w != 0.0 ? sum[i] / w : nan;
  }
}

// the sums of pass 2 -> M2 = max(0, sum(w*d*d) - sum(w*d)^2 / W), in place; NaN where W == 0, and NaN stays NaN
__global__ void __launch_bounds__(256) mvw_finalize(const double* wsum, const double* sd, double* m2, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = wsum[i];
    if (w == 0.0) {
      m2[i] = nan;
      continue;
    }
    const double s = sd[i];
    const double r = m2[i] - s * s / w;
    m2[i] = r <= 0.0 ? 0.0 : r;
  }
}

}  // namespace xhist

typedef void (*values_w_fn)(const WParams);

// the binning kernels of each weighted pass, for pick_values_kernel
struct MvwSumKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return mvw_sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return mvw_sum_generic<CMP, LDS>; }
};
struct MvwDevKernels {
  template <typename ST, int D, int SCAN>
  static values_w_fn fast() { return mvw_dev_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static values_w_fn generic() { return mvw_dev_generic<CMP, LDS>; }
};

// pass 1's sums of weights and of w*v, pass 2's mean and two sums: the slot sizes of the unweighted passes, so the same choice
static constexpr ValuesSlots kMeanVarWSlots = {{sizeof(MvwSumSlot), sizeof(MvDevSlot)}, {sizeof(MvwSumSlot), sizeof(MvDevSlot)}, true};
static_assert(sizeof(MvwSumSlot) == sizeof(MvSumSlot), "the weighted pass 1 keeps the slot size of the unweighted one");

int xhist_meanvar_w_run(const ValuesPlan& pl, const xhist_array* samples, const xhist_array* values, const xhist_array* weights,
                        int64_t n_rows, int64_t n_cols, double* out_wsum, double* out_mean, double* out_m2, double* sd, hipStream_t stream,
                        char* err, size_t err_cap, char* desc, size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  unsigned long long* zero[4] = {reinterpret_cast<unsigned long long*>(out_wsum), reinterpret_cast<unsigned long long*>(out_mean),
                                 reinterpret_cast<unsigned long long*>(out_m2), reinterpret_cast<unsigned long long*>(sd)};
  for (unsigned long long* z : zero) {
    hipLaunchKernelGGL(zero_words, dim3(grid_io), dim3(256), 0, stream, z, n_out);
    XH_VALUES_LAUNCH_CHECK("mean_var_w zeroing launch");
  }

  ValuesChoice c;
  ValuesGeometry g;
  values_w_fn sum = nullptr, dev = nullptr;
  if (n_cols > 0) {
    c = choose_values(pl, kMeanVarWSlots, samples, values, n_cols, weights);
    sum = pick_values_kernel<MvwSumKernels>(c, pl);
    dev = pick_values_kernel<MvwDevKernels>(c, pl);
    if (!sum || !dev) {
      snprintf(err, err_cap, "internal: no weighted mean_var kernel for this combination");
      return XHIST_ERR_HIP;
    }
    for (int k = 0; k < 2; ++k)
      if (int rc = allow_values_lds(k ? dev : sum, c.lds_bytes[k], "mean_var_w: setting the dynamic LDS size failed", err, err_cap))
        return rc;
    g = values_geometry(pl, c, n_rows, n_cols);
    if (int rc = launch_values_pass(sum, c.lds_bytes[0], "mvw_sum launch", pl, c, g, samples, values, n_rows, n_cols, out_wsum, out_mean,
                                    nullptr, stream, err, err_cap, weights))
      return rc;
  }
  XH_VALUES_LAUNCH(mvw_mean, dim3(grid_io), dim3(256), 0, stream, out_wsum, out_mean, n_out);
  XH_VALUES_LAUNCH_CHECK("mvw_mean launch");
  if (n_cols > 0) {
    if (int rc = launch_values_pass(dev, c.lds_bytes[1], "mvw_dev launch", pl, c, g, samples, values, n_rows, n_cols, sd, out_m2, out_mean,
                                    stream, err, err_cap, weights))
      return rc;
  }
  XH_VALUES_LAUNCH(mvw_finalize, dim3(grid_io), dim3(256), 0, stream, out_wsum, sd, out_m2, n_out);
  XH_VALUES_LAUNCH_CHECK("mvw_finalize launch");
  if (desc && desc_cap) {
    const char* fam = !sum ? "none" : c.fast ? "fast" : "generic";
    const char* home = !sum ? "none" : c.lds ? "lds" : "global";
    snprintf(desc, desc_cap,
             "mean_var_w pass1=mvw_sum_%s slots=%s pass2=mvw_dev_%s slots=%s scan=%d copies=%d block=%d segs=%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d cmp=%d",
             fam, home, fam, home, c.scan, 1 << c.copies_log2, g.block, (long long)g.segs, c.lds_bytes[0], c.lds_bytes[1],
             (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  }
  return XHIST_OK;
}
