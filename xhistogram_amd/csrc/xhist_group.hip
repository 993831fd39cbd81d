// xhist_group.hip — bin_order, the stable group-by of the samples by bin: the kernels of xhist_group.hip.h, instantiated here and
// nowhere else, the geometry of their launches and the driver that orders them; and the three kernels of the engine's scan
// (xhist_runs.hip.h), which bin_sort's passes reach through xhist_runs_scan.
//
// Instantiations (13):
//   group_count<W>, group_scatter<W>                        W 1 / 2 / 4 waves per workgroup     6
//   group_totals<WIDTH>, group_scan<WIDTH>, group_bases<WIDTH>   WIDTH 0 / 256 (bin_sort's passes)      6
//   group_identity                                                                              1
//
// Step 0 is bin_index itself: xhist_map_run(k, XHIST_MAP_INDEX) writes the int64 keys of the call into a scratch block, so every
// dtype, layout, compare domain and input count of bin_index is bin_order's.  The engine reads that block.  A call without columns
// and a plan without bins run neither: the driver zeroes the offsets, and where there are columns group_identity writes every
// row's positions as its order.
//
// Scratch of a call, from k.scratch:  n_rows * n_cols * 8 bytes of keys  +  n_rows * chunks * (B + 1) * 4 bytes of counters  +,
// where a row is cut, n_rows * ceil(chunks / 64) * (B + 1) * 4 bytes of slice totals.
// The geometry keeps the counters at no more than a quarter of the keys' bytes (chunk >= 2 * (B + 1) positions wherever a row is
// cut at all): 10^9 samples of one row take 8 GB of keys and, with 100 bins on 256 CUs, 3.3 MB of counters.
#include "xhist_group.hip.h"

#include <cstring>

namespace xhist {

// the engine's scan, for bin_order and for every pass of bin_sort: WIDTH 0 reads the width from the parameters, WIDTH 256 is
// the radix pass's (and bin_order's with 255 bins), whose index arithmetic then folds as it did in the sort's own kernels
template <int WIDTH>
__global__ void __launch_bounds__(256) group_totals(const RunsParams p) {
  runs_slices_body<false, WIDTH>(p);
}
template <int WIDTH>
__global__ void __launch_bounds__(256) group_scan(const RunsParams p) {
  runs_scan_body<WIDTH>(p);
}
template <int WIDTH>
__global__ void __launch_bounds__(256) group_bases(const RunsParams p) {
  runs_slices_body<true, WIDTH>(p);
}

}  // namespace xhist

using namespace xhist;

namespace {

// The launch geometry of a call, n_cols > 0 and (B + 1) * 4 <= pl.lds_max (runs_geometry's, with):
//   waves     the most of 4 / 2 / 1 waves per workgroup whose counters fit the LDS a workgroup may take
//   per_cu    what a CU's 160 KiB hold of such waves, at most 32
//   a chunk of at least 2 * (B + 1) positions: the counter table then stays at or below a quarter of the key block's bytes, and
//   zeroing, writing and scanning a chunk's counters stays below the work of its samples; a chunk is whole steps of 64
//   positions, so a row of a few thousand samples in few bins is already cut
struct GroupGeometry : RunsGeometry {
  int waves, bits;
  size_t lds_bytes;
};

static GroupGeometry group_geometry(const ValuesPlan& pl, int64_t n_rows, int64_t n_cols) {
  const int64_t nb1 = pl.n_bins + 1;
  const size_t wave_lds = (size_t)nb1 * 4;
  const int waves = 4 * wave_lds <= pl.lds_max ? 4 : 2 * wave_lds <= pl.lds_max ? 2 : 1;
  int bits = 0;
  while (((int64_t)1 << bits) < nb1) ++bits;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(32, (int64_t)(160 * 1024 / wave_lds)));
  return GroupGeometry{runs_geometry(pl.cus, per_cu, 2 * nb1, waves, 0, nb1, n_rows, n_cols), waves, bits, waves * wave_lds};
}

typedef void (*group_fn)(const GroupParams);
static group_fn count_kernel(int w) { return w == 4 ? group_count<4> : w == 2 ? group_count<2> : group_count<1>; }
static group_fn scatter_kernel(int w) { return w == 4 ? group_scatter<4> : w == 2 ? group_scatter<2> : group_scatter<1>; }

}  // namespace

int xhist_runs_scan(const ValuesCall& k, const RunsParams& p, const char* who) {
  // the slices' workgroups: a unit per (row, tile of slots, slice), at most kRunsSliceGrid workgroups walking them
  const int block = runs_scan_block(p.width);
  const int64_t units = p.n_rows * ((p.width + block - 1) / block) * p.slices;
  const unsigned slice_grid = (unsigned)std::min<int64_t>(units, kRunsSliceGrid);
  typedef void (*scan_fn)(const RunsParams);
  const bool fixed = p.width == 256;
  const scan_fn totals = fixed ? group_totals<256> : group_totals<0>, scan = fixed ? group_scan<256> : group_scan<0>,
                bases = fixed ? group_bases<256> : group_bases<0>;
  char what[48];  // "<who>_<step> launch": only XH_VALUES_LAUNCH_CHECK reads it, after a failed launch
  auto step = [&](const char* name) {
    snprintf(what, sizeof what, "%s_%s launch", who, name);
    return what;
  };
  if (p.chunks > 1) {
    XH_VALUES_LAUNCH(totals, dim3(slice_grid), dim3(block), 0, k.stream, p);
    XH_VALUES_LAUNCH_CHECK(k, step("totals"));
  }
  XH_VALUES_LAUNCH(scan, dim3((unsigned)p.n_rows), dim3(block), 0, k.stream, p);
  XH_VALUES_LAUNCH_CHECK(k, step("scan"));
  if (p.chunks > 1) {
    XH_VALUES_LAUNCH(bases, dim3(slice_grid), dim3(block), 0, k.stream, p);
    XH_VALUES_LAUNCH_CHECK(k, step("bases"));
  }
  return XHIST_OK;
}

int xhist_group_run(const ValuesCall& k, int64_t* out_order, int64_t* out_offsets) {
  const ValuesPlan& pl = k.pl;
  const int64_t nb1 = pl.n_bins + 1;
  if ((size_t)nb1 * 4 > pl.lds_max)
    return k.fail(XHIST_ERR_UNSUPPORTED, "bin_order takes at most %lld bins (a wave keeps one 4-byte counter per bin and one more in the "
                                         "%zu bytes of LDS of a workgroup), got %lld",
                  (long long)(pl.lds_max / 4 - 1), pl.lds_max, (long long)pl.n_bins);
  if (k.n_cols == 0 || pl.n_bins == 0) {
    if (hipMemsetAsync(out_offsets, 0, (size_t)(k.n_rows * nb1) * 8, k.stream) != hipSuccess)
      return k.fail(XHIST_ERR_HIP, "group: zeroing the offsets failed");
    if (const int64_t n = k.n_rows * k.n_cols) {  // a plan without bins drops every sample: every row's order is its positions
      const int grid = (int)std::min<int64_t>(2048, (n + 255) / 256);
      XH_VALUES_LAUNCH(group_identity, dim3(grid), dim3(256), 0, k.stream, out_order, k.n_cols, n);
      XH_VALUES_LAUNCH_CHECK(k, "group_identity launch");
    }
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
  const int block = kRunsStep * g.waves;
  for (int64_t r0 = 0; r0 < k.n_rows; r0 += g.max_rows) {
    GroupParams kp;
    kp.runs = {cnt + r0 * g.chunks * nb1, part + r0 * g.slices * nb1, out_offsets + r0 * nb1, std::min(g.max_rows, k.n_rows - r0),
               k.n_cols, g.chunk, (int32_t)g.chunks, (int32_t)g.slices, (int32_t)nb1};
    kp.keys = keys + r0 * k.n_cols;
    kp.order = out_order + r0 * k.n_cols;
    kp.bits = g.bits;
    if (int rc = runs_pass(k, count, scatter, g.waves, g.lds_bytes, kp, "group")) return rc;
  }
  k.describe("group keys=%s bits=%d waves=%d block=%d chunks=%lld chunk=%lld lds_bytes=%zu rows_per_launch=%lld D=%d cmp=%d", family,
             g.bits, g.waves, block, (long long)g.chunks, (long long)g.chunk, g.lds_bytes, (long long)g.max_rows, pl.n_dims, values_cmp(pl));
  return XHIST_OK;
}
