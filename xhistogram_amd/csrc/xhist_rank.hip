// xhist_rank.hip — bin_rank, the rank of every sample's value among the non-NaN values of its bin: the kernels of
// xhist_rank.hip.h, instantiated here and nowhere else, and the driver that orders them behind the sort.
//
// Instantiations (6): rank_heads, rank_totals, rank_scan, rank_words, rank_bins, rank_apply.  The method and whether the call is
// pct are kernel-uniform parameters, not template axes; rank_bins is launched only for pct.
//
// The driver runs bin_sort's own driver (xhist_sort_run) into scratch order and offsets blocks and takes over the sorted bin
// keys its last pass wrote.  Then, per batch of the sort's rows_per_launch rows, a chain of plain launches: rank_heads,
// rank_totals, rank_scan, rank_words, rank_bins (pct), rank_apply.  A call without columns or a plan without bins fills out with
// NaN (bytes of all ones) and launches nothing.
//
// Scratch of a call, from k.scratch, on top of the sort's 32 bytes per sample: 8 bytes per sample of order, n_rows * (B + 1) * 8
// bytes of offsets, per 64 samples of a row 28 bytes (the head word, the NaN word, and before / last / next), per 65536 samples
// of a row 12 bytes more (a tile's three scalars), and n_rows * B * 8 bytes of divisors when pct.
#include "xhist_rank.hip.h"

using namespace xhist;

namespace {

constexpr int64_t kRankFlatGrid = 1 << 16;  // workgroups of the grid-strided kernels

static const char* rank_method_name(int method) {
  static const char* const names[] = {"average", "min", "max", "dense", "ordinal"};
  return method >= XHIST_RANK_AVERAGE && method <= XHIST_RANK_ORDINAL ? names[method] : "?";
}

}  // namespace

int xhist_rank_run(const ValuesCall& k, int method, int descending, int pct, double* out) {
  const ValuesPlan& pl = k.pl;
  const int64_t nb = pl.n_bins, nb1 = nb + 1;
  if (method < XHIST_RANK_AVERAGE || method > XHIST_RANK_ORDINAL) return k.fail(XHIST_ERR_INVALID, "unknown rank method %d", method);
  if (k.n_cols >= ((int64_t)1 << 31))
    return k.fail(XHIST_ERR_UNSUPPORTED, "bin_rank takes fewer than 2^31 samples per output row (a row's positions are held in 32 bits), "
                                         "got %lld", (long long)k.n_cols);
  if (nb1 > ((int64_t)1 << 32))
    return k.fail(XHIST_ERR_UNSUPPORTED, "bin_rank takes at most 2^32 - 1 bins (a bin key is sorted in four 8-bit digits), got %lld",
                  (long long)nb);
  const int64_t n = k.n_rows * k.n_cols;
  if (k.n_cols == 0 || nb == 0) {
    if (n > 0 && hipMemsetAsync(out, 0xff, (size_t)n * 8, k.stream) != hipSuccess) return k.fail(XHIST_ERR_HIP, "rank: filling out with NaN failed");
    k.describe("rank method=%s pct=%d descending=%d words=0 rows_per_launch=0 | none", rank_method_name(method), pct ? 1 : 0,
               descending ? 1 : 0);
    return XHIST_OK;
  }
  const int64_t words = (k.n_cols + 63) / 64, nw = k.n_rows * words, tiles = (words + kRankTile - 1) / kRankTile;
  // one block for all of it (a call's scope holds few blocks, and the sort takes seven): the 8-byte parts first
  const size_t n_off = (size_t)(k.n_rows * nb1), n_div = pct ? (size_t)(k.n_rows * nb) : 0, n_part = (size_t)(k.n_rows * tiles) * 3;
  char* const block = static_cast<char*>(k.scratch(((size_t)n + n_off + 2 * (size_t)nw + n_div) * 8 + ((size_t)nw * 3 + n_part) * 4));
  if (!block) return k.fail(XHIST_ERR_NOMEM, "allocation of the rank scratch block failed");
  int64_t* const order = reinterpret_cast<int64_t*>(block);
  int64_t* const offsets = order + n;
  uint64_t* const headw = reinterpret_cast<uint64_t*>(offsets + n_off);
  uint64_t* const nanw = headw + nw;
  double* const div = pct ? reinterpret_cast<double*>(nanw + nw) : nullptr;
  uint32_t* const scalars = reinterpret_cast<uint32_t*>(nanw + nw + n_div);
  uint32_t* const part = scalars + 3 * nw;  // (every batch of rows uses its head)

  SortHandover hand = {nullptr, 0};
  if (int rc = xhist_sort_run(k, descending, order, offsets, &hand)) return rc;
  if (!hand.keys || hand.rows_per_launch < 1) return k.fail(XHIST_ERR_HIP, "internal: the sort handed over no bin keys");
  char sort_line[384];
  snprintf(sort_line, sizeof sort_line, "%s", k.desc);

  for (int64_t r0 = 0; r0 < k.n_rows; r0 += hand.rows_per_launch) {
    const int64_t nr = std::min(hand.rows_per_launch, k.n_rows - r0);
    RankParams rp;
    rp.v = values_read(*k.values, r0);
    rp.method = method;
    rp.order = order + r0 * k.n_cols;
    rp.keys = hand.keys + r0 * k.n_cols;
    rp.offsets = offsets + r0 * nb1;
    rp.headw = headw + r0 * words;
    rp.nanw = nanw + r0 * words;
    rp.before = scalars + r0 * words;
    rp.last = scalars + nw + r0 * words;
    rp.next = scalars + 2 * nw + r0 * words;
    rp.div = pct ? div + r0 * nb : nullptr;
    rp.out = out + r0 * k.n_cols;
    rp.n_rows = nr;
    rp.n_cols = k.n_cols;
    rp.words = words;
    rp.tiles = tiles;
    rp.part = part;
    rp.nb = nb;
    const unsigned word_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (nr * words + kRankWaves - 1) / kRankWaves);
    XH_VALUES_LAUNCH(rank_heads, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_heads launch");
    const unsigned tile_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, nr * tiles);
    XH_VALUES_LAUNCH(rank_totals, dim3(tile_grid), dim3(256), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_totals launch");
    XH_VALUES_LAUNCH(rank_scan, dim3((unsigned)nr), dim3(256), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_scan launch");
    XH_VALUES_LAUNCH(rank_words, dim3(tile_grid), dim3(256), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_words launch");
    if (pct) {
      const unsigned bin_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (nr * nb + 255) / 256);
      XH_VALUES_LAUNCH(rank_bins, dim3(bin_grid), dim3(256), 0, k.stream, rp);
      XH_VALUES_LAUNCH_CHECK(k, "rank_bins launch");
    }
    XH_VALUES_LAUNCH(rank_apply, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_apply launch");
  }
  k.describe("rank method=%s pct=%d descending=%d words=%lld rows_per_launch=%lld | %s", rank_method_name(method), pct ? 1 : 0,
             descending ? 1 : 0, (long long)words, (long long)hand.rows_per_launch, sort_line);
  return XHIST_OK;
}
