// xhist_map.hip — the per-sample maps (bin_index, histogram_lookup, histogram_anomaly): the kernels of xhist_map.hip.h,
// instantiated here and nowhere else, and the driver that chooses and launches them (the family rule, the geometry and the
// Params of a launch: xhist_values.hip.h, with a call that may have no values).
//
// Instantiations (51):
//   map_fast<OP, ST, D, SCAN>      OP index / take / anomaly, ST float / double, D 1 / 2, SCAN 1 / 2 / kScanArith     36
//   map_generic<OP, CMP, TLDS>     OP take / anomaly, CMP 0 / 1 / 3, the table row in LDS or in global memory         12
//   map_generic<index, CMP, false> CMP 0 / 1 / 3 (no table)                                                            3
#include "xhist_map.hip.h"

using namespace xhist;

typedef void (*map_fn)(const MapParams);

// the kernels of one op, for pick_values_kernel (whose `LDS` is the table row's home here)
template <int OP>
struct MapKernels {
  template <typename ST, int D, int SCAN>
  static map_fn fast() { return map_fast<OP, ST, D, SCAN>; }
  template <int CMP, bool TLDS>
  static map_fn generic() { return map_generic<OP, CMP, (OP != kMapIndex) && TLDS>; }
};

static const char* map_op_name(int op) { return op == kMapIndex ? "index" : op == kMapTake ? "take" : "anomaly"; }

int xhist_map_run(const ValuesCall& k, int op, const double* centre, const double* scale, void* out) {
  const ValuesPlan& pl = k.pl;
  if (k.n_cols == 0 || pl.n_bins == 0) {
    // a plan without bins counts no sample: -1 for XHIST_MAP_INDEX and NaN for the others.  Bytes of all ones are both.
    if (k.n_cols > 0 && hipMemsetAsync(out, 0xff, (size_t)(k.n_rows * k.n_cols) * 8, k.stream) != hipSuccess)
      return k.fail(XHIST_ERR_HIP, "map: filling out failed");
    k.describe("map op=%s family=none table=none scan=0 cmp=%d segs=0 block=0 lds_bytes=0 tables_in_lds=0 scale=%d D=%d", map_op_name(op),
               values_cmp(pl), scale ? 1 : 0, pl.n_dims);
    return XHIST_OK;
  }
  // The "slot" of the family rule is what a bin keeps in LDS: its centre, and its scale where one is given; bin_index keeps
  // nothing.  The table is float64 whatever the samples are, and there are no copies.
  const size_t slot = op == kMapIndex ? 0 : scale ? 16 : 8;
  const ValuesSlots sl = {{slot, 0}, {slot, 0}, false};
  ValuesChoice c = choose_values(k, sl);
  // (choose_values leaves the LDS bytes of a pass without slots at 0: bin_index still stages its digitize tables)
  const size_t tbytes = c.tables_in_lds ? ((size_t)c.table_words + 1) / 2 * 16 : 0;
  c.lds_bytes[0] = tbytes + (c.lds ? (size_t)pl.n_bins * slot : 0);
  c.lds_bytes[1] = 0;
  const map_fn fn = op == kMapIndex  ? pick_values_kernel<MapKernels<kMapIndex>>(c, pl)
                    : op == kMapTake ? pick_values_kernel<MapKernels<kMapTake>>(c, pl)
                                     : pick_values_kernel<MapKernels<kMapAnomaly>>(c, pl);
  if (!fn) return k.fail(XHIST_ERR_HIP, "internal: no map kernel for this combination");
  if (int rc = allow_values_lds(k, fn, c.lds_bytes[0], "map: setting the dynamic LDS size failed")) return rc;
  const ValuesGeometry g = values_geometry(pl, c, k.n_rows, k.n_cols);
  for (int64_t r0 = 0; r0 < k.n_rows; r0 += g.max_rows) {
    const int64_t nr = std::min(g.max_rows, k.n_rows - r0);
    MapParams kp;
    static_cast<Params&>(kp) = values_params(k, c, g.segs, r0, nr);
    kp.centre = centre ? centre + r0 * pl.n_bins : nullptr;
    kp.scale = scale ? scale + r0 * pl.n_bins : nullptr;
    kp.out = static_cast<uint64_t*>(out) + r0 * k.n_cols;
    XH_VALUES_LAUNCH(fn, dim3((unsigned)(nr * g.segs)), dim3(g.block), c.lds_bytes[0], k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, "map launch");
  }
  k.describe("map op=%s family=%s table=%s scan=%d cmp=%d segs=%lld block=%d lds_bytes=%zu tables_in_lds=%d scale=%d D=%d",
             map_op_name(op), c.fast ? "fast" : "generic", op == kMapIndex ? "none" : c.lds ? "lds" : "global", c.scan, values_cmp(pl),
             (long long)g.segs, g.block, c.lds_bytes[0], (int)c.tables_in_lds, scale ? 1 : 0, pl.n_dims);
  return XHIST_OK;
}
