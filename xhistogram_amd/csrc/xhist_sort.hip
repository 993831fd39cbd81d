// xhist_sort.hip — bin_sort, the samples grouped by bin and sorted by value inside each bin: the kernels of xhist_sort.hip.h,
// instantiated here and nowhere else, the constants of their launch geometry (runs_geometry's) and the driver that orders them.
//
// Instantiations (5): sort_keys, sort_gather, sort_count, sort_scatter, sort_offsets.  sort_count and sort_scatter are the count
// and scatter bodies of xhist_runs.hip.h on SortParams; the scan between them is xhist_runs_scan, whose three kernels
// xhist_group.hip defines.  Whether a scatter writes keys, uint32 positions or the int64 order is a kernel-uniform parameter,
// not a template axis.
//
// Step 0 is bin_index itself: xhist_map_run(k, XHIST_MAP_INDEX) writes the int64 bin keys of the call into a scratch block, so
// every dtype, layout, compare domain and input count of bin_index is bin_sort's.  Phase A sorts (value key, position) by the
// value key, least significant digit first, and launches no digit the dtype of the values makes constant (sort_value_shift).
// Phase B gathers the bin key of every sorted position and sorts by it in ceil(log2(B + 1) / 8) passes; the sort is stable, so
// the value order survives inside each bin.  The last pass of the call stores int64 positions straight into out_order and the
// sorted bin keys beside them, from which sort_offsets writes the offsets (one way for every B: the last pass's totals would
// serve only up to 255 bins).
//
// Scratch of a call, from k.scratch, per sample: 8 bytes of bin keys + 2 * 8 bytes of keys + 2 * 4 bytes of positions = 32 bytes
// (24 for a plan without bins); per launch 1 KiB of counters per (row, chunk) and per (row, slice of 64 chunks), at most
// kSortCounterBytes: a chunk is never shorter than 512 positions unless the row is, so the counters of rows of 512 samples or
// more stay below a sixteenth of the records' bytes.  Rows shorter than that still pay 1 KiB each, in launches of fewer rows.
#include "xhist_sort.hip.h"

#include <cstring>

using namespace xhist;

namespace {

constexpr int64_t kSortPerCu = 32;                   // waves the geometry wants on a CU
constexpr int64_t kSortMinChunk = 512;               // positions of a chunk, unless the row is shorter
constexpr int64_t kSortCounterBytes = 256ll << 20;   // counters of one launch's rows
constexpr int64_t kSortFlatGrid = 8192;              // workgroups of the grid-strided kernels over all samples

// The low bits of a value key that every value of the dtype shares up to the sign: a value of the dtype, taken as float64, has
// that many zero bits at the bottom of its mantissa, so a key's low bits are all zeros (value >= +0.0 ascending) or all ones,
// and a NaN's key, all ones, shares its high digits with no other key.  The digits inside them order nothing the digits above
// do not: phase A starts at digit shift / 8.
//   float32 as float64: 52 - 23 = 29; float16: 52 - 10 = 42; an integer below 2^L in magnitude: 53 - L
static int sort_value_shift(int dt) {
  switch (dt) {
    case XHIST_F32: return 29;
    case XHIST_F16: return 42;
    case XHIST_I32: case XHIST_U32: return 21;
    case XHIST_I16: case XHIST_U16: return 37;
    case XHIST_I8: case XHIST_U8: return 45;
    case XHIST_BOOL: return 52;
    default: return 0;  // float64, and 64-bit integers: they round to any float64
  }
}

static const char* sort_dtype_name(int dt) {
  static const char* const names[] = {"f64", "f32", "f16", "i64", "i32", "i16", "i8", "u64", "u32", "u16", "u8", "bool"};
  return dt >= 0 && dt < 12 ? names[dt] : "?";
}

}  // namespace

// The driver.  `hand` (nullptr: nobody asks) receives what bin_rank builds on: the sorted bin keys the last pass of a call with
// bins wrote beside the order (scratch of the call, alive until the call returns) and the rows of a launch.
int xhist_sort_run(const ValuesCall& k, int descending, int64_t* out_order, int64_t* out_offsets, SortHandover* hand) {
  const ValuesPlan& pl = k.pl;
  const int64_t nb = pl.n_bins, nb1 = nb + 1;  // (n_cols < 2^31 and nb1 <= 2^32: the front has refused the rest)
  const int vdt = k.values->dtype;
  int bin_bits = 0;
  while (((int64_t)1 << bin_bits) < nb1) ++bin_bits;
  const int bin_passes = (bin_bits + 7) / 8, first_digit = sort_value_shift(vdt) / 8, value_passes = 8 - first_digit;
  if (k.n_cols == 0 || nb == 0) {
    if (hipMemsetAsync(out_offsets, 0, (size_t)(k.n_rows * nb1) * 8, k.stream) != hipSuccess)
      return k.fail(XHIST_ERR_HIP, "sort: zeroing the offsets failed");
    if (k.n_cols == 0) {
      k.describe("sort keys=none value_passes=0 bin_passes=0 waves=0 block=0 chunks=0 chunk=0 slices=0 rows_per_launch=0 D=%d cmp=%d vdtype=%s",
                 pl.n_dims, values_cmp(pl), sort_dtype_name(vdt));
      return XHIST_OK;
    }
  }
  // (n_cols > 0.  Rows shorter than kSortMinChunk are one chunk; the counters of one launch stay within kSortCounterBytes.)
  const RunsGeometry g = runs_geometry(pl.cus, kSortPerCu, kSortMinChunk, kSortWaves, kSortCounterBytes, kSortDigits, k.n_rows, k.n_cols);
  const int64_t n = k.n_rows * k.n_cols, launch_rows = std::min(g.max_rows, k.n_rows);
  int64_t* const binkeys = nb > 0 ? static_cast<int64_t*>(k.scratch((size_t)n * 8)) : nullptr;
  uint64_t* kbuf[2] = {static_cast<uint64_t*>(k.scratch((size_t)n * 8)), static_cast<uint64_t*>(k.scratch((size_t)n * 8))};
  uint32_t* pbuf[2] = {static_cast<uint32_t*>(k.scratch((size_t)n * 4)), static_cast<uint32_t*>(k.scratch((size_t)n * 4))};
  uint32_t* const cnt = static_cast<uint32_t*>(k.scratch((size_t)(launch_rows * g.chunks * kSortDigits) * 4));
  uint32_t* const part = g.chunks == 1 ? cnt : static_cast<uint32_t*>(k.scratch((size_t)(launch_rows * g.slices * kSortDigits) * 4));
  if ((nb > 0 && !binkeys) || !kbuf[0] || !kbuf[1] || !pbuf[0] || !pbuf[1] || !cnt || !part)
    return k.fail(XHIST_ERR_NOMEM, "allocation of the sort scratch blocks failed");

  // step 0: the bin keys, by bin_index's own driver on the samples alone.  Its line about the launch is overwritten below: the
  // family is all that is quoted.
  const char* family = "none";
  if (nb > 0) {
    ValuesCall k0 = k;
    k0.values = nullptr;
    if (int rc = xhist_map_run(k0, XHIST_MAP_INDEX, nullptr, nullptr, binkeys)) return rc;
    family = strstr(k.desc, "family=fast") ? "fast" : "generic";
  }

  const unsigned flat_grid = (unsigned)std::min<int64_t>(kSortFlatGrid, (n + 255) / 256);
  const SortKeyParams sp = {values_read(*k.values, 0), descending ? 1 : 0, kbuf[0], pbuf[0], k.n_rows, k.n_cols};
  XH_VALUES_LAUNCH(sort_keys, dim3(flat_grid), dim3(256), 0, k.stream, sp);
  XH_VALUES_LAUNCH_CHECK(k, "sort_keys launch");

  const int block = kRunsStep * kSortWaves;
  const size_t lds = (size_t)kSortWaves * kSortDigits * 4;
  for (int64_t r0 = 0; r0 < k.n_rows; r0 += g.max_rows) {
    const int64_t nr = std::min(g.max_rows, k.n_rows - r0), at = r0 * k.n_cols;
    const unsigned batch_grid = (unsigned)std::min<int64_t>(kSortFlatGrid, (nr * (k.n_cols + 1) + 255) / 256);
    int cur = 0;  // the buffers that hold the records
    for (int pass = 0; pass < value_passes + bin_passes; ++pass) {
      const bool phase_b = pass >= value_passes;
      const bool last_of_a = pass == value_passes - 1, last = pass == value_passes + bin_passes - 1;
      if (phase_b && pass == value_passes) {
        // the bin key of every sorted position, into the key buffer beside the positions (the value keys are done with)
        XH_VALUES_LAUNCH(sort_gather, dim3(batch_grid), dim3(256), 0, k.stream, (const int64_t*)(binkeys + at), (const uint32_t*)(pbuf[cur] + at),
                         kbuf[cur] + at, k.n_cols, nr * k.n_cols, nb);
        XH_VALUES_LAUNCH_CHECK(k, "sort_gather launch");
      }
      SortParams kp;
      kp.runs = {cnt, part, nullptr, nr, k.n_cols, g.chunk, (int32_t)g.chunks, (int32_t)g.slices, kSortDigits};
      kp.kin = kbuf[cur] + at;
      kp.pin = pbuf[cur] + at;
      kp.kout = (last ? bin_passes > 0 : !last_of_a) ? kbuf[cur ^ 1] + at : nullptr;
      kp.pout = last ? nullptr : pbuf[cur ^ 1] + at;
      kp.order = last ? out_order + at : nullptr;
      kp.shift = 8 * (phase_b ? pass - value_passes : first_digit + pass);
      if (int rc = runs_pass(k, sort_count, sort_scatter, kSortWaves, lds, kp, "sort")) return rc;
      cur ^= 1;
    }
    if (bin_passes > 0) {
      XH_VALUES_LAUNCH(sort_offsets, dim3(batch_grid), dim3(256), 0, k.stream, (const uint64_t*)(kbuf[cur] + at), out_offsets + r0 * nb1, nr,
                       k.n_cols, nb);
      XH_VALUES_LAUNCH_CHECK(k, "sort_offsets launch");
    }
  }
  if (hand) {
    hand->keys = bin_passes > 0 ? kbuf[(value_passes + bin_passes) & 1] : nullptr;  // (every batch of rows ends in the same buffer)
    hand->rows_per_launch = g.max_rows;
  }
  k.describe("sort keys=%s value_passes=%d bin_passes=%d waves=%d block=%d chunks=%lld chunk=%lld slices=%lld rows_per_launch=%lld D=%d cmp=%d "
             "vdtype=%s", family, value_passes, bin_passes, kSortWaves, block, (long long)g.chunks, (long long)g.chunk, (long long)g.slices,
             (long long)g.max_rows, pl.n_dims, values_cmp(pl), sort_dtype_name(vdt));
  return XHIST_OK;
}
