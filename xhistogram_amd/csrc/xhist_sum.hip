// xhist_sum.hip — per-bin sums that do not depend on the order of arrival (histogram_sum): the kernels of xhist_sum.hip.h,
// instantiated here and nowhere else, the finalize after them, and the driver that orders the launches (pass 1 is
// histogram_extrema's, launched by xhist_extrema.hip; the choice and the launches themselves: xhist_values.hip.h).
//
// Instantiations (18 binning kernels + 1):
//   sum_fast<ST, D, SCAN>     ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith          12
//   sum_generic<CMP, LDS>     CMP 0 / 1 / 3, slots in LDS or in global memory                6
//   sum_finalize                                                                            1
// (and zero_words of xhist_kernels.hip.h, which is not dispatched)
#include "xhist_sum.hip.h"

using namespace xhist;

namespace xhist {

// the keys and the limb planes -> the totals; the counts are already what they are
__global__ void __launch_bounds__(256) sum_finalize(const uint64_t* kmin, const uint64_t* kmax, const int64_t* limbs, const uint64_t* count,
                                                    double* total, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    total[i] = sum_total(count[i], kmin[i], kmax[i], limbs[i], limbs[n + i], limbs[2 * n + i]);
}

}  // namespace xhist

// pass 2's binning kernels, for pick_values_kernel
struct SumKernels {
  template <typename ST, int D, int SCAN>
  static auto fast() -> void (*)(const CovParams) { return sum_fast<ST, D, SCAN>; }
  template <int CMP, bool LDS>
  static auto generic() -> void (*)(const CovParams) { return sum_generic<CMP, LDS>; }
};

// pass 1: a bin's two keys; pass 2: the three accumulators, the count and the unit, the same 30 bytes for float32 values, in
// copies.  The larger pass decides family, home and copies for both.  The slots come in groups of four (SumGroup), so pass 2's
// LDS is rounded up to whole groups: at most 90 bytes more than the rule counted.  Where that crosses the LDS a workgroup may
// take, the rule is asked again with 32 bytes a slot, which covers the groups of any count above 45.
static constexpr ValuesSlots kSumSlots = {{16, 30}, {8, 30}, true};
static constexpr ValuesSlots kSumSlotsRounded = {{16, 32}, {8, 32}, true};

// Pass 2's LDS bytes of a choice made with `declared` bytes a slot, in whole groups; false: beyond the LDS of a workgroup.
// The fast family gives up copies until eight workgroups share a CU's 160 KiB where it can: the integer adds queue less than the
// float64 ones (C4's 50 bins cost the same with 8 copies as with 16), and the residency is worth more than the copies (C2's 100
// bins: 8 copies leave six workgroups on a CU and cost a tenth more than 4 copies and eight of them).
static bool sum_whole_groups(ValuesChoice& c, const ValuesPlan& pl, size_t declared) {
  if (!c.lds) return true;
  const size_t own = c.fast && c.f32 ? kSumSlots.fast32[0] : kSumSlots.bytes[0];
  const size_t tbytes = c.lds_bytes[1] - ((size_t)pl.n_bins * declared << c.copies_log2);
  auto need = [&](int cl) { return tbytes + (((size_t)pl.n_bins << cl) + 3) / 4 * sizeof(SumGroup); };
  while (c.copies_log2 > 0 && need(c.copies_log2) > 160 * 1024 / 8) --c.copies_log2;
  if (need(c.copies_log2) > pl.lds_max) return false;
  c.lds_bytes[0] = tbytes + ((size_t)pl.n_bins * own << c.copies_log2);  // (as choose_values states pass 1: xhist_extrema_pass1 takes the copies off)
  c.lds_bytes[1] = need(c.copies_log2);
  return true;
}

int xhist_sum_run(const ValuesCall& k, int64_t* out_count, double* out_total) {
  const ValuesPlan& pl = k.pl;
  if (k.n_cols >= ((int64_t)1 << 31))
    return k.fail(XHIST_ERR_UNSUPPORTED, "histogram_sum takes fewer than 2^31 samples per output row (the int64 accumulators of a bin "
                                         "hold that many 32-bit limbs), got %lld", (long long)k.n_cols);
  const int64_t n_out = k.n_rows * pl.n_bins;
  // the call's scratch: pass 1's two key planes, then the three limb planes; the counts gather in out_count itself
  uint64_t* const kmin = static_cast<uint64_t*>(k.scratch((size_t)(5 * n_out) * sizeof(uint64_t)));
  if (!kmin) return k.fail(XHIST_ERR_NOMEM, "allocation of the sum scratch blocks failed");
  uint64_t* const kmax = kmin + n_out;
  int64_t* const limbs = reinterpret_cast<int64_t*>(kmin + 2 * n_out);
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(grid_io), dim3(256), 0, k.stream, reinterpret_cast<unsigned long long*>(limbs), 3 * n_out);
  XH_VALUES_LAUNCH_CHECK(k, "sum zeroing launch");
  XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(grid_io), dim3(256), 0, k.stream, reinterpret_cast<unsigned long long*>(out_count), n_out);
  XH_VALUES_LAUNCH_CHECK(k, "sum zeroing launch");

  ValuesChoice c;
  ValuesGeometry g;
  int64_t segs1 = 0;
  size_t lds1 = 0;
  void (*pass2)(const CovParams) = nullptr;
  if (k.n_cols > 0) {
    c = choose_values(k, kSumSlots);
    if (!sum_whole_groups(c, pl, kSumSlots.bytes[1])) {
      c = choose_values(k, kSumSlotsRounded);
      if (!sum_whole_groups(c, pl, kSumSlotsRounded.bytes[1])) return k.fail(XHIST_ERR_HIP, "internal: the sum slots do not fit the LDS they were chosen for");
    }
    pass2 = pick_values_kernel<SumKernels>(c, pl);
    if (!pass2) return k.fail(XHIST_ERR_HIP, "internal: no sum kernel for this combination");
    if (int rc = allow_values_lds(k, pass2, c.lds_bytes[1], "sum: setting the dynamic LDS size failed")) return rc;
    g = values_geometry(pl, c, k.n_rows, k.n_cols);
  }
  // pass 1 with the residency of its own slots, one copy of 16 (8) bytes a bin: its size is not pass 2's
  if (int rc = xhist_extrema_pass1(k, c, kmin, kmax, &segs1, &lds1)) return rc;
  if (pass2) {
    if (int rc = launch_values_pass(pass2, c.lds_bytes[1], "sum launch", k, c, g, limbs, out_count, kmin)) return rc;
  }
  XH_VALUES_LAUNCH(sum_finalize, dim3(grid_io), dim3(256), 0, k.stream, kmin, kmax, limbs, reinterpret_cast<const uint64_t*>(out_count),
                   out_total, n_out);
  XH_VALUES_LAUNCH_CHECK(k, "sum_finalize launch");
  const bool ran = k.n_cols > 0;
  const char* fam = !ran ? "none" : c.fast ? "fast" : "generic";
  const char* home = !ran ? "none" : c.lds ? "lds" : "global";
  k.describe("sum pass1=extrema_%s slots=%s pass2=sum_%s slots=%s scan=%d copies=%d block=%d segs=%lld/%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d cmp=%d",
             fam, home, fam, home, c.scan, 1 << c.copies_log2, g.block, (long long)segs1, (long long)g.segs, lds1,
             c.lds_bytes[1], (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  return XHIST_OK;
}

// Test support: the host side of xhist_sum.hip.h over one bin, with no device: the `n` values as histogram_sum takes them (NaN
// ignored) through the keys, sum_unit, sum_limbs and sum_total, the accumulators plain int64 additions.
extern "C" int xhist_debug_sum_host(const double* values, int64_t n, int64_t* out_count, double* out_total) {
  if (n < 0 || (n > 0 && !values) || !out_count || !out_total || n >= ((int64_t)1 << 31)) return XHIST_ERR_INVALID;
  uint64_t kmin = kEmptyMin64, kmax = kEmptyMax64, count = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (values[i] != values[i]) continue;
    const uint64_t key = extrema_key64(values[i]);
    kmin = std::min(kmin, key);
    kmax = std::max(kmax, key);
    ++count;
  }
  const int32_t U = sum_unit(kmin, kmax);
  uint64_t L[3] = {0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const double v = values[i];
    if (v != v) continue;
    if (U == kSumUnitInf) {
      if (v == __builtin_inf()) ++L[0];
      if (v == -__builtin_inf()) ++L[1];
      continue;
    }
    uint32_t limb[3];
    const bool neg = sum_limbs(v, U, limb);
    for (int j = 0; j < 3; ++j) L[j] += neg ? 0ull - (uint64_t)limb[j] : (uint64_t)limb[j];
  }
  *out_count = (int64_t)count;
  *out_total = sum_total(count, kmin, kmax, (int64_t)L[0], (int64_t)L[1], (int64_t)L[2]);
  return XHIST_OK;
}

// ... and the one rounding alone, for accumulators no short list of values reaches: RN_even((L0 + L1 * 2^32 + L2 * 2^64) * 2^U)
extern "C" int xhist_debug_sum_round(int64_t L0, int64_t L1, int64_t L2, int U, double* out) {
  if (!out || U < kSumUnitMin || U > 1023) return XHIST_ERR_INVALID;
  *out = sum_round(L0, L1, L2, U);
  return XHIST_OK;
}
