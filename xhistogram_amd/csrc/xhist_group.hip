// xhist_group.hip — bin_order, the stable group-by of the samples by bin: the kernels of xhist_group.hip.h, instantiated here and
// nowhere else, the geometry of their launches and the driver that orders them.
//
// Instantiations (10):
//   group_count<W>, group_scatter<W>                        W 1 / 2 / 4 waves per workgroup     6
//   group_totals, group_scan, group_bases, group_identity                                       4
//
// Step 0 is bin_index itself: xhist_map_run(k, XHIST_MAP_INDEX) writes the int64 keys of the call into a scratch block, so every
// dtype, layout, compare domain and input count of bin_index is bin_order's.  Steps 1 to 3 (xhist_group.hip.h) read that block.
//
// Scratch of a call, from k.scratch:  n_rows * n_cols * 8 bytes of keys  +  n_rows * chunks * (B + 1) * 4 bytes of counters  +,
// where a row is cut, n_rows * ceil(chunks / 64) * (B + 1) * 4 bytes of slice totals.
// The geometry keeps the counters at no more than a quarter of the keys' bytes (chunk >= 2 * (B + 1) positions wherever a row is
// cut at all): 10^9 samples of one row take 8 GB of keys and, with 100 bins on 256 CUs, 3.3 MB of counters.
#include "xhist_group.hip.h"

#include <cstring>

using namespace xhist;

namespace {

struct GroupGeometry {
  int waves = 1, bits = 0;
  int64_t chunks = 0, chunk = 0, slices = 0, max_rows = 0;
  size_t lds_bytes = 0;
};

// The launch geometry of a call, n_cols > 0 and (B + 1) * 4 <= pl.lds_max:
//   waves     the most of 4 / 2 / 1 waves per workgroup whose counters fit the LDS a workgroup may take
//   chunks    (a) rows that fill the device alone get one chunk each; (b) fewer rows are cut until cus * per_cu waves exist,
//             per_cu = what a CU's 160 KiB hold of them, at most 32; (c) never so far that a chunk is shorter than 2 * (B + 1)
//             positions: the counter table then stays at or below a quarter of the key block's bytes, and zeroing, writing and
//             scanning a chunk's counters stays below the work of its samples; (d) a chunk is whole steps of 64 positions, so a
//             row of a few thousand samples in few bins is already cut
//   max_rows  rows per launch: workgroups below 2^31 and lanes below 2^32, for the (row, chunk) grid and for group_scan's rows
static GroupGeometry group_geometry(const ValuesPlan& pl, int64_t n_rows, int64_t n_cols) {
  GroupGeometry g;
  const int64_t nb1 = pl.n_bins + 1;
  const size_t wave_lds = (size_t)nb1 * 4;
  g.waves = 4 * wave_lds <= pl.lds_max ? 4 : 2 * wave_lds <= pl.lds_max ? 2 : 1;
  g.lds_bytes = g.waves * wave_lds;
  while (((int64_t)1 << g.bits) < nb1) ++g.bits;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(32, (int64_t)(160 * 1024 / wave_lds)));
  const int64_t target = (int64_t)pl.cus * per_cu;
  const int64_t steps = (n_cols + kGroupStep - 1) / kGroupStep;
  int64_t want = std::min<int64_t>(steps, (target + n_rows - 1) / n_rows);
  want = std::max<int64_t>(1, std::min<int64_t>(want, n_cols / (2 * nb1)));
  g.chunk = ((n_cols + want - 1) / want + kGroupStep - 1) / kGroupStep * kGroupStep;
  g.chunks = (n_cols + g.chunk - 1) / g.chunk;
  g.slices = g.chunks == 1 ? 1 : (g.chunks + kGroupSlice - 1) / kGroupSlice;
  const int64_t max_units = (((int64_t)1 << 32) - 1) / (kGroupStep * g.waves) * g.waves;
  g.max_rows = std::max<int64_t>(1, std::min<int64_t>(max_units / g.chunks, (((int64_t)1 << 32) - 1) / 256));
  return g;
}

constexpr int64_t kSliceGrid = 4096;  // workgroups of group_totals / group_bases, 16 to a CU of 256: they walk their units grid-strided

typedef void (*group_fn)(const GroupParams);
static group_fn count_kernel(int w) { return w == 4 ? group_count<4> : w == 2 ? group_count<2> : group_count<1>; }
static group_fn scatter_kernel(int w) { return w == 4 ? group_scatter<4> : w == 2 ? group_scatter<2> : group_scatter<1>; }

}  // namespace

int xhist_group_run(const ValuesCall& k, int64_t* out_order, int64_t* out_offsets) {
  const ValuesPlan& pl = k.pl;
  const int64_t nb1 = pl.n_bins + 1;
  if (k.n_cols >= ((int64_t)1 << 31))
    return k.fail(XHIST_ERR_UNSUPPORTED, "bin_order takes fewer than 2^31 samples per output row (a row's offsets are held in 32 bits), "
                                         "got %lld", (long long)k.n_cols);
  if ((size_t)nb1 * 4 > pl.lds_max)
    return k.fail(XHIST_ERR_UNSUPPORTED, "bin_order takes at most %lld bins (a wave keeps one 4-byte counter per bin and one more in the "
                                         "%zu bytes of LDS of a workgroup), got %lld",
                  (long long)(pl.lds_max / 4 - 1), pl.lds_max, (long long)pl.n_bins);
  if (k.n_cols == 0) {
    if (hipMemsetAsync(out_offsets, 0, (size_t)(k.n_rows * nb1) * 8, k.stream) != hipSuccess)
      return k.fail(XHIST_ERR_HIP, "group: zeroing the offsets failed");
    k.describe("group keys=none bits=0 waves=0 block=0 chunks=0 chunk=0 lds_bytes=0 rows_per_launch=0 D=%d cmp=%d", pl.n_dims, values_cmp(pl));
    return XHIST_OK;
  }
  const GroupGeometry g = group_geometry(pl, k.n_rows, k.n_cols);
  int64_t* const keys = static_cast<int64_t*>(k.scratch((size_t)(k.n_rows * k.n_cols) * 8));
  uint32_t* const cnt = static_cast<uint32_t*>(k.scratch((size_t)(k.n_rows * g.chunks * nb1) * 4));
  uint32_t* const part = g.chunks == 1 ? cnt : static_cast<uint32_t*>(k.scratch((size_t)(k.n_rows * g.slices * nb1) * 4));
  if (!keys || !cnt || !part) return k.fail(XHIST_ERR_NOMEM, "allocation of the group scratch blocks failed");

  // step 0: the keys.  Its line about the launch is overwritten below: the family is all that is quoted.
  if (int rc = xhist_map_run(k, XHIST_MAP_INDEX, nullptr, nullptr, keys)) return rc;
  const char* family = strstr(k.desc, "family=fast") ? "fast" : "generic";

  const group_fn count = count_kernel(g.waves), scatter = scatter_kernel(g.waves);
  if (int rc = allow_values_lds(k, count, g.lds_bytes, "group: setting the dynamic LDS size failed")) return rc;
  if (int rc = allow_values_lds(k, scatter, g.lds_bytes, "group: setting the dynamic LDS size failed")) return rc;
  const int block = kGroupStep * g.waves;
  const int scan_block = nb1 <= 64 ? 64 : 256;
  for (int64_t r0 = 0; r0 < k.n_rows; r0 += g.max_rows) {
    const int64_t nr = std::min(g.max_rows, k.n_rows - r0);
    GroupParams kp;
    kp.keys = keys + r0 * k.n_cols;
    kp.cnt = cnt + r0 * g.chunks * nb1;
    kp.part = part + r0 * g.slices * nb1;
    kp.order = out_order + r0 * k.n_cols;
    kp.offsets = out_offsets + r0 * nb1;
    kp.n_rows = nr;
    kp.n_cols = k.n_cols;
    kp.chunk = g.chunk;
    kp.chunks = (int32_t)g.chunks;
    kp.slices = (int32_t)g.slices;
    kp.nb1 = (int32_t)nb1;
    kp.bits = g.bits;
    const unsigned grid = (unsigned)((nr * g.chunks + g.waves - 1) / g.waves);
    XH_VALUES_LAUNCH(count, dim3(grid), dim3(block), g.lds_bytes, k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, "group_count launch");
    // the slices' workgroups: a unit per (row, tile of bins, slice), at most kSliceGrid workgroups walking them
    const int64_t units = nr * ((nb1 + scan_block - 1) / scan_block) * g.slices;
    const unsigned slice_grid = (unsigned)std::min<int64_t>(units, kSliceGrid);
    if (g.chunks > 1) {
      XH_VALUES_LAUNCH(group_totals, dim3(slice_grid), dim3(scan_block), 0, k.stream, kp);
      XH_VALUES_LAUNCH_CHECK(k, "group_totals launch");
    }
    XH_VALUES_LAUNCH(group_scan, dim3((unsigned)nr), dim3(scan_block), 0, k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, "group_scan launch");
    if (g.chunks > 1) {
      XH_VALUES_LAUNCH(group_bases, dim3(slice_grid), dim3(scan_block), 0, k.stream, kp);
      XH_VALUES_LAUNCH_CHECK(k, "group_bases launch");
    }
    XH_VALUES_LAUNCH(scatter, dim3(grid), dim3(block), g.lds_bytes, k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, "group_scatter launch");
  }
  k.describe("group keys=%s bits=%d waves=%d block=%d chunks=%lld chunk=%lld lds_bytes=%zu rows_per_launch=%lld D=%d cmp=%d", family,
             g.bits, g.waves, block, (long long)g.chunks, (long long)g.chunk, g.lds_bytes, (long long)g.max_rows, pl.n_dims, values_cmp(pl));
  return XHIST_OK;
}

int xhist_group_no_bins(int64_t n_rows, int64_t n_cols, int64_t* out_order, int64_t* out_offsets, hipStream_t stream) {
  if (hipMemsetAsync(out_offsets, 0, (size_t)n_rows * 8, stream) != hipSuccess) return XHIST_ERR_HIP;
  const int64_t n = n_rows * n_cols;
  if (n > 0) {
    const int grid = (int)std::min<int64_t>(2048, (n + 255) / 256);
    XH_VALUES_LAUNCH(group_identity, dim3(grid), dim3(256), 0, stream, out_order, n_cols, n);
    if (hipGetLastError() != hipSuccess) return XHIST_ERR_HIP;
  }
  return XHIST_OK;
}
