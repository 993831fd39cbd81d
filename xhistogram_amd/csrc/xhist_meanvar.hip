// xhist_meanvar.hip — per-bin count, mean and variance (histogram_mean_var): the kernels of xhist_meanvar.hip.h, instantiated
// here and nowhere else, the steps between and after the two passes, and the one function that chooses and launches.
//
// Instantiations (36 binning kernels + 2):
//   mv_sum_fast<ST, D, SCAN>, mv_dev_fast<ST, D, SCAN>    ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     12 + 12
//   mv_sum_generic<CMP, LDS>, mv_dev_generic<CMP, LDS>    CMP 0 / 1 / 3, slots in LDS or sums in global memory       6 + 6
//   mv_mean, mv_finalize                                                                                              2
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_meanvar.hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace xhist;

// every kernel but the zeroing goes through the census log of the dispatch surface, as in xhist_extrema.hip
#define XH_MV_LAUNCH(fn, ...)                                   \
  do {                                                          \
    xhist_log_picked_kernel(reinterpret_cast<const void*>(fn)); \
    hipLaunchKernelGGL(fn, __VA_ARGS__);                        \
  } while (0)

namespace xhist {

// the sums of pass 1 -> means, in place: S / n, NaN where no value arrived
__global__ void __launch_bounds__(256) mv_mean(const unsigned long long* cnt, double* sum, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    sum[i] = c ? sum[i] / (double)c : nan;
  }
}

// the sums of pass 2 -> M2 = max(0, sum(d*d) - sum(d)^2 / n), in place; NaN where no value arrived, and NaN stays NaN
__global__ void __launch_bounds__(256) mv_finalize(const unsigned long long* cnt, const double* sd, double* m2, int64_t n) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long c = cnt[i];
    if (!c) {
      m2[i] = nan;
      continue;
    }
    const double s = sd[i];
    const double r = m2[i] - s * s / (double)c;
    m2[i] = r <= 0.0 ? 0.0 : r;
  }
}

}  // namespace xhist

typedef void (*mv_fn)(const Params);

template <int PASS, typename ST, int D>
static mv_fn fast_scan(int scan) {
  if (scan == 1) return PASS == 1 ? mv_sum_fast<ST, D, 1> : mv_dev_fast<ST, D, 1>;
  if (scan == 2) return PASS == 1 ? mv_sum_fast<ST, D, 2> : mv_dev_fast<ST, D, 2>;
  if (scan == kScanArith) return PASS == 1 ? mv_sum_fast<ST, D, kScanArith> : mv_dev_fast<ST, D, kScanArith>;
  return nullptr;
}

template <int PASS>
static mv_fn fast_kernel(bool f32, int D, int scan) {
  if (f32) return D == 1 ? fast_scan<PASS, float, 1>(scan) : fast_scan<PASS, float, 2>(scan);
  return D == 1 ? fast_scan<PASS, double, 1>(scan) : fast_scan<PASS, double, 2>(scan);
}

template <int CMP>
static mv_fn generic_cmp(int pass, bool lds) {
  if (pass == 1) return lds ? mv_sum_generic<CMP, true> : mv_sum_generic<CMP, false>;
  return lds ? mv_dev_generic<CMP, true> : mv_dev_generic<CMP, false>;
}

static mv_fn generic_kernel(int pass, int cmp, bool lds) {
  // (the domain as the histogram's generic family reads it: exactly float64, exactly int64, else per input)
  if (cmp == XHIST_CMP_F64) return generic_cmp<0>(pass, lds);
  if (cmp == XHIST_CMP_I64) return generic_cmp<1>(pass, lds);
  return generic_cmp<3>(pass, lds);
}

static int error(char* err, size_t cap, int code, const char* what, hipError_t e) {
  snprintf(err, cap, "%s: %s", what, hipGetErrorString(e));
  return code;
}

static int elem_bytes(int dt) {
  return (dt == XHIST_F64 || dt == XHIST_I64 || dt == XHIST_U64) ? 8 : (dt == XHIST_F32 || dt == XHIST_I32 || dt == XHIST_U32) ? 4
       : (dt == XHIST_F16 || dt == XHIST_I16 || dt == XHIST_U16) ? 2 : 1;
}

#define XH_MV_LAUNCH_CHECK(what)                                     \
  do {                                                               \
    hipError_t e_ = hipGetLastError();                               \
    if (e_ != hipSuccess) return error(err, err_cap, XHIST_ERR_HIP, what, e_); \
  } while (0)

// The largest LDS slot of the two passes: pass 2's mean and two sums.  Both passes take the family and home chosen for it.
constexpr size_t kSlotBytes = sizeof(MvDevSlot);
static_assert(sizeof(MvSumSlot) <= kSlotBytes, "pass 1's slot fits where pass 2's does");

// What the two binning launches run and where their slots live.
struct MvChoice {
  mv_fn sum = nullptr, dev = nullptr;
  bool fast = false, lds = false, tables_in_lds = false;
  int scan = 0, copies_log2 = 0;
  const ExtremaTables* tab = nullptr;
  int32_t table_words = 0;
  size_t lds_bytes[2] = {0, 0};  // pass 1, pass 2
};

// Copies of the fast family's slots: the most (up to 16) whose pass-2 slots stay within 24 KiB, so that a CU still holds
// several workgroups.  C2's 100 bins get 8, C4's 50 get 16; above 1024 bins there is one.
static int fast_copies_log2(int64_t n_bins, size_t tbytes, size_t lds_max) {
  int cl = 0;
  while (cl < 4 && ((size_t)n_bins * kSlotBytes << (cl + 1)) <= 24 * 1024 && tbytes + ((size_t)n_bins * kSlotBytes << (cl + 1)) <= lds_max) ++cl;
  return cl;
}

// fast if eligible, else generic with its slots in LDS, else generic with its sums in global memory (the rule of
// xhist_extrema.hip's choose(), with 24-byte slots)
static MvChoice choose(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_cols) {
  MvChoice c;
  const int D = pl.n_dims;
  const int sdt = samples[0].dtype;
  bool fast_ok = pl.cmp == XHIST_CMP_F64 && D <= 2 && (sdt == XHIST_F64 || sdt == XHIST_F32) && values->dtype == sdt &&
                 pl.n_bins < ((int64_t)1 << 24);
  for (int d = 0; d < D && fast_ok; ++d)
    fast_ok = samples[d].dtype == sdt && (samples[d].col_stride == 1 || n_cols == 1) && (uintptr_t)samples[d].data % (size_t)elem_bytes(sdt) == 0;
  if (fast_ok) fast_ok = (values->col_stride == 1 || n_cols == 1) && (uintptr_t)values->data % (size_t)elem_bytes(sdt) == 0;
  const size_t slots1 = (size_t)pl.n_bins * sizeof(MvSumSlot), slots2 = (size_t)pl.n_bins * kSlotBytes;
  if (fast_ok) {
    const ExtremaTables& fine = sdt == XHIST_F32 ? pl.fine32 : pl.fine64;
    const size_t tbytes = ((size_t)fine.words + 1) / 2 * 16;
    if (fine.blob && fine.max_cnt >= 1 && fine.max_cnt <= 2 && tbytes + slots2 <= pl.lds_max) {
      c.scan = fine.max_cnt;
      c.tab = &fine;
      c.table_words = fine.words;
      c.copies_log2 = fast_copies_log2(pl.n_bins, tbytes, pl.lds_max);
      c.lds_bytes[0] = tbytes + (slots1 << c.copies_log2);
      c.lds_bytes[1] = tbytes + (slots2 << c.copies_log2);
    } else if (pl.arith && slots2 <= pl.lds_max) {
      c.scan = kScanArith;
      c.tab = &pl.native;  // (the float64-domain DimTable carries e_0, e_last and the step; no table is read)
      c.table_words = 0;
      c.copies_log2 = fast_copies_log2(pl.n_bins, 0, pl.lds_max);
      c.lds_bytes[0] = slots1 << c.copies_log2;
      c.lds_bytes[1] = slots2 << c.copies_log2;
    }
    if (c.tab) {
      c.sum = fast_kernel<1>(sdt == XHIST_F32, D, c.scan);
      c.dev = fast_kernel<2>(sdt == XHIST_F32, D, c.scan);
      c.fast = c.lds = c.tables_in_lds = true;
      return c;
    }
  }
  c.tab = &pl.native;
  const size_t tbytes = ((size_t)pl.native.words + 1) / 2 * 16;
  c.tables_in_lds = tbytes + 1024 <= pl.lds_max;
  c.table_words = c.tables_in_lds ? pl.native.words : 0;
  c.lds = c.tables_in_lds && pl.n_bins < ((int64_t)1 << 24) && tbytes + slots2 <= pl.lds_max;
  for (int k = 0; k < 2; ++k) c.lds_bytes[k] = c.tables_in_lds ? tbytes + (c.lds ? (k ? slots2 : slots1) : 0) : 0;
  c.sum = generic_kernel(1, pl.cmp, c.lds);
  c.dev = generic_kernel(2, pl.cmp, c.lds);
  return c;
}

int xhist_meanvar_run(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      int64_t* out_count, double* out_mean, double* out_m2, double* sd, hipStream_t stream, char* err, size_t err_cap,
                      char* desc, size_t desc_cap) {
  const int64_t n_out = n_rows * pl.n_bins;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out_count);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  unsigned long long* zero[4] = {cnt, reinterpret_cast<unsigned long long*>(out_mean), reinterpret_cast<unsigned long long*>(out_m2),
                                 reinterpret_cast<unsigned long long*>(sd)};
  for (unsigned long long* z : zero) {
    hipLaunchKernelGGL(zero_words, dim3(grid_io), dim3(256), 0, stream, z, n_out);
    XH_MV_LAUNCH_CHECK("mean_var zeroing launch");
  }

  MvChoice c;
  int block = 0;
  int64_t segs = 0;
  if (n_cols > 0) {
    c = choose(pl, samples, values, n_cols);
    if (!c.sum || !c.dev) {
      snprintf(err, err_cap, "internal: no mean_var kernel for this combination");
      return XHIST_ERR_HIP;
    }
    for (int k = 0; k < 2; ++k) {
      if (c.lds_bytes[k] > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)(k ? c.dev : c.sum), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_bytes[k]);
        if (e != hipSuccess) return error(err, err_cap, XHIST_ERR_HIP, "mean_var: setting the dynamic LDS size failed", e);
      }
    }
    // geometry (both passes): every resident workgroup at once, the workgroups of a row walking its tiles interleaved; pass 2's
    // LDS footprint sets the residency.  A workgroup sees fewer than 2^31 samples, so its uint32 counts cannot wrap.
    block = c.fast ? 256 : 512;
    const int vec = samples[0].dtype == XHIST_F32 ? 4 : 2;
    const int64_t per_tile = c.fast ? (int64_t)block * (pl.n_dims == 1 ? 4 * vec : 8) : block;  // (mv_*_fast: VEC x UNROLL per lane)
    int bpc = 2048 / block;
    if (c.lds_bytes[1]) bpc = (int)std::max<size_t>(1, std::min<size_t>((size_t)bpc, 160 * 1024 / c.lds_bytes[1]));
    const int64_t target = (int64_t)pl.cus * bpc;
    const int64_t tiles = (n_cols + per_tile - 1) / per_tile;
    segs = std::max<int64_t>(1, std::min<int64_t>(tiles, (target + n_rows - 1) / n_rows));
    segs = std::max<int64_t>(segs, (tiles * per_tile + ((int64_t)1 << 31) - 1) >> 31);
    const int64_t max_rows = (((int64_t)1 << 31) - 1) / segs;
    for (int pass = 1; pass <= 2; ++pass) {
      if (pass == 2) {
        XH_MV_LAUNCH(mv_mean, dim3(grid_io), dim3(256), 0, stream, cnt, out_mean, n_out);
        XH_MV_LAUNCH_CHECK("mv_mean launch");
      }
      const mv_fn fn = pass == 1 ? c.sum : c.dev;
      const size_t lds = c.lds_bytes[pass - 1];
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
        if (pass == 1) {
          kp.out = cnt + r0 * pl.n_bins;
          kp.out2 = out_mean + r0 * pl.n_bins;
        } else {
          kp.w2_ptr = out_mean + r0 * pl.n_bins;
          kp.out = sd + r0 * pl.n_bins;
          kp.out2 = out_m2 + r0 * pl.n_bins;
        }
        kp.segs = (int32_t)segs;
        kp.copies_log2 = c.copies_log2;
        XH_MV_LAUNCH(fn, dim3((unsigned)(nr * segs)), dim3(block), lds, stream, kp);
        XH_MV_LAUNCH_CHECK(pass == 1 ? "mv_sum launch" : "mv_dev launch");
      }
    }
  } else {
    XH_MV_LAUNCH(mv_mean, dim3(grid_io), dim3(256), 0, stream, cnt, out_mean, n_out);
    XH_MV_LAUNCH_CHECK("mv_mean launch");
  }
  XH_MV_LAUNCH(mv_finalize, dim3(grid_io), dim3(256), 0, stream, cnt, sd, out_m2, n_out);
  XH_MV_LAUNCH_CHECK("mv_finalize launch");
  if (desc && desc_cap) {
    const char* fam = !c.sum ? "none" : c.fast ? "fast" : "generic";
    const char* home = !c.sum ? "none" : c.lds ? "lds" : "global";
    snprintf(desc, desc_cap,
             "mean_var pass1=mv_sum_%s slots=%s pass2=mv_dev_%s slots=%s scan=%d copies=%d block=%d segs=%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d",
             fam, home, fam, home, c.scan, 1 << c.copies_log2, block, (long long)segs, c.lds_bytes[0], c.lds_bytes[1], (int)c.tables_in_lds,
             pl.n_dims);
  }
  return XHIST_OK;
}
