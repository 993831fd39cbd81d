// xhist_extrema.hip — per-bin minimum and maximum (histogram_extrema): the kernels of xhist_extrema.hip.h, instantiated here and
// nowhere else, the key conversions before and after them, and the one function that chooses and launches.
//
// Instantiations (18 binning kernels + 2):
//   extrema_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith          12
//   extrema_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or in global memory                6
//   extrema_prepare, extrema_finalize                                                          2
#include "xhist_extrema.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace xhist;

// every binning kernel, prepare and finalize included, goes through the census log of the dispatch surface (XH_LAUNCH_PICKED
// of xhist_host_common.hip.h, whose logger lives in xhist_capi.hip)
#define XH_EXT_LAUNCH(fn, ...)                                  \
  do {                                                          \
    xhist_log_picked_kernel(reinterpret_cast<const void*>(fn)); \
    hipLaunchKernelGGL(fn, __VA_ARGS__);                        \
  } while (0)

namespace xhist {

// The output's doubles -> keys, in place: fresh (the empty markers) or accumulating (NaN = empty, as the result reads).
__global__ void __launch_bounds__(256) extrema_prepare(uint64_t* kmin, uint64_t* kmax, int64_t n, int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!accumulate) {
      kmin[i] = kEmptyMin64;
      kmax[i] = kEmptyMax64;
      continue;
    }
    const double lo = __builtin_bit_cast(double, kmin[i]), hi = __builtin_bit_cast(double, kmax[i]);
    kmin[i] = lo == lo ? extrema_key64(lo) : kEmptyMin64;
    kmax[i] = hi == hi ? extrema_key64(hi) : kEmptyMax64;
  }
}

// ... and back: keys -> doubles, the markers -> NaN
__global__ void __launch_bounds__(256) extrema_finalize(uint64_t* kmin, uint64_t* kmax, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t lo = kmin[i], hi = kmax[i];
    reinterpret_cast<double*>(kmin)[i] = lo == kEmptyMin64 ? nan : extrema_value64(lo);
    reinterpret_cast<double*>(kmax)[i] = hi == kEmptyMax64 ? nan : extrema_value64(hi);
  }
}

}  // namespace xhist

typedef void (*extrema_fn)(const Params);

template <typename ST, int D>
static extrema_fn fast_scan(int scan) {
  if (scan == 1) return extrema_fast<ST, D, 1>;
  if (scan == 2) return extrema_fast<ST, D, 2>;
  if (scan == kScanArith) return extrema_fast<ST, D, kScanArith>;
  return nullptr;
}

static extrema_fn fast_kernel(bool f32, int D, int scan) {
  if (f32) return D == 1 ? fast_scan<float, 1>(scan) : fast_scan<float, 2>(scan);
  return D == 1 ? fast_scan<double, 1>(scan) : fast_scan<double, 2>(scan);
}

static extrema_fn generic_kernel(int cmp, bool lds) {
  // (the domain as the histogram's generic family reads it: exactly float64, exactly int64, else per input)
  if (cmp == XHIST_CMP_F64) return lds ? extrema_generic<0, true> : extrema_generic<0, false>;
  if (cmp == XHIST_CMP_I64) return lds ? extrema_generic<1, true> : extrema_generic<1, false>;
  return lds ? extrema_generic<3, true> : extrema_generic<3, false>;
}

static int error(char* err, size_t cap, int code, const char* what, hipError_t e) {
  snprintf(err, cap, "%s: %s", what, hipGetErrorString(e));
  return code;
}

static int elem_bytes(int dt) {
  return (dt == XHIST_F64 || dt == XHIST_I64 || dt == XHIST_U64) ? 8 : (dt == XHIST_F32 || dt == XHIST_I32 || dt == XHIST_U32) ? 4
       : (dt == XHIST_F16 || dt == XHIST_I16 || dt == XHIST_U16) ? 2 : 1;
}

#define XH_EXT_LAUNCH_CHECK(what)                                    \
  do {                                                               \
    hipError_t e_ = hipGetLastError();                               \
    if (e_ != hipSuccess) return error(err, err_cap, XHIST_ERR_HIP, what, e_); \
  } while (0)

// What the binning launch runs and where its slots live.
struct ExtremaChoice {
  extrema_fn fn = nullptr;
  bool fast = false, lds = false, tables_in_lds = false;
  int scan = 0;
  const ExtremaTables* tab = nullptr;
  int32_t table_words = 0;
  size_t lds_bytes = 0;
};

// fast if eligible, else generic with its slots in LDS, else generic with its keys in global memory
static ExtremaChoice choose(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_cols) {
  ExtremaChoice c;
  const int D = pl.n_dims;
  const int sdt = samples[0].dtype;
  bool fast_ok = pl.cmp == XHIST_CMP_F64 && D <= 2 && (sdt == XHIST_F64 || sdt == XHIST_F32) && values->dtype == sdt &&
                 pl.n_bins < ((int64_t)1 << 24);
  for (int d = 0; d < D && fast_ok; ++d)
    fast_ok = samples[d].dtype == sdt && (samples[d].col_stride == 1 || n_cols == 1) && (uintptr_t)samples[d].data % (size_t)elem_bytes(sdt) == 0;
  if (fast_ok) fast_ok = (values->col_stride == 1 || n_cols == 1) && (uintptr_t)values->data % (size_t)elem_bytes(sdt) == 0;
  if (fast_ok) {
    const size_t slot = sdt == XHIST_F32 ? 8 : 16;
    const size_t slots = (size_t)pl.n_bins * slot;
    const ExtremaTables& fine = sdt == XHIST_F32 ? pl.fine32 : pl.fine64;
    const size_t tbytes = ((size_t)fine.words + 1) / 2 * 16;
    if (fine.blob && fine.max_cnt >= 1 && fine.max_cnt <= 2 && tbytes + slots <= pl.lds_max) {
      c.scan = fine.max_cnt;
      c.tab = &fine;
      c.table_words = fine.words;
      c.lds_bytes = tbytes + slots;
    } else if (pl.arith && slots <= pl.lds_max) {
      c.scan = kScanArith;
      c.tab = &pl.native;  // (the float64-domain DimTable carries e_0, e_last and the step; no table is read)
      c.table_words = 0;
      c.lds_bytes = slots;
    }
    if (c.tab) {
      c.fn = fast_kernel(sdt == XHIST_F32, D, c.scan);
      c.fast = c.lds = c.tables_in_lds = true;
      return c;
    }
  }
  c.tab = &pl.native;
  const size_t tbytes = ((size_t)pl.native.words + 1) / 2 * 16;
  c.tables_in_lds = tbytes + 1024 <= pl.lds_max;
  c.table_words = c.tables_in_lds ? pl.native.words : 0;
  c.lds = c.tables_in_lds && pl.n_bins < ((int64_t)1 << 24) && tbytes + (size_t)pl.n_bins * 16 <= pl.lds_max;
  c.lds_bytes = c.tables_in_lds ? tbytes + (c.lds ? (size_t)pl.n_bins * 16 : 0) : 0;
  c.fn = generic_kernel(pl.cmp, c.lds);
  return c;
}

int xhist_extrema_run(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      double* out_min, double* out_max, int accumulate, hipStream_t stream, char* err, size_t err_cap, char* desc,
                      size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  uint64_t* kmin = reinterpret_cast<uint64_t*>(out_min);
  uint64_t* kmax = reinterpret_cast<uint64_t*>(out_max);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_EXT_LAUNCH(extrema_prepare, dim3(grid_io), dim3(256), 0, stream, kmin, kmax, n_out, accumulate);
  XH_EXT_LAUNCH_CHECK("extrema_prepare launch");

  if (n_cols > 0) {
    const ExtremaChoice c = choose(pl, samples, values, n_cols);
    if (!c.fn) {
      snprintf(err, err_cap, "internal: no extrema kernel for this combination");
      return XHIST_ERR_HIP;
    }
    if (c.lds_bytes > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)c.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_bytes);
      if (e != hipSuccess) return error(err, err_cap, XHIST_ERR_HIP, "extrema: setting the dynamic LDS size failed", e);
    }
    // geometry: every resident workgroup at once, the workgroups of a row walking its tiles interleaved
    const int block = c.fast ? 256 : 512;
    const int vec = samples[0].dtype == XHIST_F32 ? 4 : 2;
    const int64_t per_tile = c.fast ? (int64_t)block * (pl.n_dims == 1 ? 4 * vec : 8) : block;  // (extrema_fast: VEC x UNROLL per lane)
    int bpc = 2048 / block;
    if (c.lds_bytes) bpc = (int)std::max<size_t>(1, std::min<size_t>((size_t)bpc, 160 * 1024 / c.lds_bytes));
    const int64_t target = (int64_t)pl.cus * bpc;
    const int64_t tiles = (n_cols + per_tile - 1) / per_tile;
    const int64_t segs = std::max<int64_t>(1, std::min<int64_t>(tiles, (target + n_rows - 1) / n_rows));
    const int64_t max_rows = (((int64_t)1 << 31) - 1) / segs;
    for (int64_t r0 = 0; r0 < n_rows; r0 += max_rows) {
      const int64_t nr = std::min(max_rows, n_rows - r0);
      Params kp;
      memset(&kp, 0, sizeof kp);
      for (int d = 0; d < pl.n_dims; ++d) {
        kp.s_ptr[d] = samples[d].data;
        kp.s_rs[d] = samples[d].row_stride;
        kp.s_cs[d] = samples[d].col_stride;
        kp.s_ir[d] = samples[d].inner_rows;
        kp.s_os[d] = samples[d].outer_stride;
        kp.s_dt[d] = samples[d].dtype;
        kp.dim[d] = c.tab->dim[d];
      }
      kp.w_ptr = values->data;
      kp.w_rs = values->row_stride;
      kp.w_cs = values->col_stride;
      kp.w_ir = values->inner_rows;
      kp.w_os = values->outer_stride;
      kp.w_dt = values->dtype;
      kp.row0 = r0;
      kp.n_dims = pl.n_dims;
      kp.tables = c.tab->blob;
      kp.table_words = c.table_words;
      kp.tables_in_lds = c.tables_in_lds ? 1 : 0;
      kp.n_rows = nr;
      kp.n_cols = n_cols;
      kp.n_bins = pl.n_bins;
      kp.out = kmin + r0 * pl.n_bins;
      kp.out2 = kmax + r0 * pl.n_bins;
      kp.segs = (int32_t)segs;
      XH_EXT_LAUNCH(c.fn, dim3((unsigned)(nr * segs)), dim3(block), c.lds_bytes, stream, kp);
      XH_EXT_LAUNCH_CHECK("extrema launch");
    }
    if (desc && desc_cap)
      snprintf(desc, desc_cap, "extrema family=%s slots=%s scan=%d block=%d segs=%lld lds_bytes=%zu tables_in_lds=%d D=%d",
               c.fast ? "fast" : "generic", c.lds ? "lds" : "global", c.scan, block, (long long)segs, c.lds_bytes, (int)c.tables_in_lds,
               pl.n_dims);
  }
  XH_EXT_LAUNCH(extrema_finalize, dim3(grid_io), dim3(256), 0, stream, kmin, kmax, n_out);
  XH_EXT_LAUNCH_CHECK("extrema_finalize launch");
  return XHIST_OK;
}
