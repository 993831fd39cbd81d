// xhist_rank.hip — bin_rank, the rank of every sample's value among the non-NaN values of its bin, histogram_mode, each bin's
// most frequent value, bin_unique, each bin's distinct values and their counts, and the weighted twins of the last two,
// bin_weighted_unique and histogram_weighted_mode: the kernels of xhist_rank.hip.h, xhist_mode.hip.h, xhist_unique.hip.h and
// xhist_wruns.hip.h, instantiated here and nowhere else, and the five drivers that order them behind the sort.
//
// Instantiations (21): rank_heads, rank_totals, rank_scan, rank_words, rank_bins, rank_apply, mode_runs, mode_finish, unique_bins,
// unique_scan, unique_runs, unique_pad, unique_inverse, wruns_words, wruns_totals, wruns_scan, wruns_close, wruns_pad, wmode_max,
// wmode_pos, wmode_finish.  The method, whether the call is pct and where a run's sum is stored are kernel-uniform parameters,
// not template axes (wmode_max and wmode_pos are the two instantiations of one walk); rank_bins is launched only for pct,
// unique_inverse only for a call with an inverse, the wruns kernels of bin_weighted_unique only for a width above 0.
//
// Both drivers run bin_sort's own driver (xhist_sort_run) into scratch order and offsets blocks and take over the sorted bin
// keys its last pass wrote.  Then, per batch of the sort's rows_per_launch rows, a chain of plain launches: rank_heads,
// rank_totals, rank_scan, rank_words (sorted_domain_run, which both share), and then rank_bins (pct), rank_apply for bin_rank, a
// fill of the slots with 0, mode_runs, mode_finish for histogram_mode.  A bin_rank call without columns or a plan without bins
// fills out with NaN (bytes of all ones) and launches nothing; a histogram_mode call without columns launches mode_finish alone.
// bin_unique's tail is unique_bins, unique_scan, unique_runs, unique_pad (a width above 0) and unique_inverse (an inverse); a call
// without columns or a plan without bins zeroes the offsets and launches unique_pad alone.  Each of these empty cases is its
// driver's own branch and leaves its own "none" line; the C ABI's front has refused the sorted order's two limits, an unknown
// method and a negative size before a driver runs.
//
// Scratch of a call, from k.scratch, on top of the sort's 32 bytes per sample: 8 bytes per sample of order, n_rows * (B + 1) * 8
// bytes of offsets, per 64 samples of a row 28 bytes (the head word, the NaN word, and before / last / next), per 65536 samples
// of a row 12 bytes more (a tile's three scalars), and n_rows * B * 8 bytes of divisors when pct.  histogram_mode takes the same
// without the divisors and nothing more: its slots are the out_mode_count block.  bin_unique takes the same again: its distinct
// counts and their scan live in out_offsets.  The weighted twins add, in the same block: 16 bytes per 64 samples of a row (a word's
// lead and tail sums) and 16 bytes per 65536 samples of a row (a tile's element), and histogram_weighted_mode 8 bytes per sample
// more (every run's sum at its first position) with its distinct-value scan left out; bin_weighted_unique's tail is bin_unique's,
// then (a width above 0) wruns_words, wruns_totals, wruns_scan, wruns_close and wruns_pad; histogram_weighted_mode's is two fills
// of the slots, the same four wruns kernels, wmode_max, wmode_pos and wmode_finish (alone for a call without columns).
#include "xhist_mode.hip.h"
#include "xhist_unique.hip.h"
#include "xhist_wruns.hip.h"

using namespace xhist;

namespace {

constexpr int64_t kRankFlatGrid = 1 << 16;  // workgroups of the grid-strided kernels

static const char* rank_method_name(int method) {
  static const char* const names[] = {"average", "min", "max", "dense", "ordinal"};
  return method >= XHIST_RANK_AVERAGE && method <= XHIST_RANK_ORDINAL ? names[method] : "?";
}

// what sorted_domain_run tells its caller about the call: the words of a row, the rows of one launch, the sort's describe() line
struct SortedDomain {
  int64_t words, rows_per_launch;
  char sort_line[384];
  size_t extra_bytes = 0;  // in: bytes (a multiple of 8) the caller wants at the head of the scratch block
  char* extra = nullptr;   // out: where they are
};

// What bin_rank and histogram_mode share, for a call with columns and bins: one scratch block for all of it (a call's scope
// holds few blocks, and the sort takes seven; the 8-byte parts first, `pct`: with the block of divisors), the sort into it, and
// per batch of the sort's rows_per_launch rows the four launches that build the sorted domain; then tail(rp, r0, nr, word_grid),
// the caller's own launches over that batch, which returns a status.
template <class Tail>
static int sorted_domain_run(const ValuesCall& k, const char* who, int method, int descending, bool pct, double* out, SortedDomain& dom,
                             Tail tail) {
  const int64_t nb = k.pl.n_bins, nb1 = nb + 1, n = k.n_rows * k.n_cols;
  const int64_t words = (k.n_cols + 63) / 64, nw = k.n_rows * words, tiles = (words + kRankTile - 1) / kRankTile;
  const size_t n_off = (size_t)(k.n_rows * nb1), n_div = pct ? (size_t)(k.n_rows * nb) : 0, n_part = (size_t)(k.n_rows * tiles) * 3;
  char* const block =
      static_cast<char*>(k.scratch(dom.extra_bytes + ((size_t)n + n_off + 2 * (size_t)nw + n_div) * 8 + ((size_t)nw * 3 + n_part) * 4));
  if (!block) return k.fail(XHIST_ERR_NOMEM, "allocation of the %s scratch block failed", who);
  dom.extra = block;
  int64_t* const order = reinterpret_cast<int64_t*>(block + dom.extra_bytes);
  int64_t* const offsets = order + n;
  uint64_t* const headw = reinterpret_cast<uint64_t*>(offsets + n_off);
  uint64_t* const nanw = headw + nw;
  double* const div = pct ? reinterpret_cast<double*>(nanw + nw) : nullptr;
  uint32_t* const scalars = reinterpret_cast<uint32_t*>(nanw + nw + n_div);
  uint32_t* const part = scalars + 3 * nw;  // (every batch of rows uses its head)

  SortHandover hand = {nullptr, 0};
  ValuesCall sort_call = k;  // (the sort reads samples and values alone: weights must not move its choice of key kernels)
  sort_call.third = sort_call.fourth = nullptr;
  if (int rc = xhist_sort_run(sort_call, descending, order, offsets, &hand)) return rc;
  if (!hand.keys || hand.rows_per_launch < 1) return k.fail(XHIST_ERR_HIP, "internal: the sort handed over no bin keys");
  snprintf(dom.sort_line, sizeof dom.sort_line, "%s", k.desc);
  dom.words = words;
  dom.rows_per_launch = hand.rows_per_launch;

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
    rp.out = out ? out + r0 * k.n_cols : nullptr;
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
    if (int rc = tail(rp, r0, nr, word_grid)) return rc;
  }
  return XHIST_OK;
}

}  // namespace

int xhist_rank_run(const ValuesCall& k, int method, int descending, int pct, double* out) {
  const ValuesPlan& pl = k.pl;
  const int64_t nb = pl.n_bins;
  const int64_t n = k.n_rows * k.n_cols;
  if (k.n_cols == 0 || nb == 0) {
    if (n > 0 && hipMemsetAsync(out, 0xff, (size_t)n * 8, k.stream) != hipSuccess) return k.fail(XHIST_ERR_HIP, "rank: filling out with NaN failed");
    k.describe("rank method=%s pct=%d descending=%d words=0 rows_per_launch=0 | none", rank_method_name(method), pct ? 1 : 0,
               descending ? 1 : 0);
    return XHIST_OK;
  }
  SortedDomain dom;
  const int rc = sorted_domain_run(k, "rank", method, descending, pct != 0, out, dom, [&](const RankParams& rp, int64_t, int64_t nr, unsigned word_grid) {
    if (pct) {
      const unsigned bin_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (nr * nb + 255) / 256);
      XH_VALUES_LAUNCH(rank_bins, dim3(bin_grid), dim3(256), 0, k.stream, rp);
      XH_VALUES_LAUNCH_CHECK(k, "rank_bins launch");
    }
    XH_VALUES_LAUNCH(rank_apply, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, rp);
    XH_VALUES_LAUNCH_CHECK(k, "rank_apply launch");
    return (int)XHIST_OK;
  });
  if (rc != XHIST_OK) return rc;
  k.describe("rank method=%s pct=%d descending=%d words=%lld rows_per_launch=%lld | %s", rank_method_name(method), pct ? 1 : 0,
             descending ? 1 : 0, (long long)dom.words, (long long)dom.rows_per_launch, dom.sort_line);
  return XHIST_OK;
}

int xhist_mode_run(const ValuesCall& k, int64_t* out_count, int64_t* out_nunique, double* out_mode, int64_t* out_mode_count) {
  const int64_t nb = k.pl.n_bins;
  auto params = [&](const RankParams& rp, int64_t r0) {
    ModeParams mp;
    mp.r = rp;
    mp.slots = reinterpret_cast<uint64_t*>(out_mode_count + r0 * nb);
    mp.out_count = out_count + r0 * nb;
    mp.out_nunique = out_nunique + r0 * nb;
    mp.out_mode = out_mode + r0 * nb;
    mp.out_mode_count = out_mode_count + r0 * nb;
    return mp;
  };
  auto finish = [&](const ModeParams& mp) {
    const unsigned bin_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (mp.r.n_rows * nb + 255) / 256);
    XH_VALUES_LAUNCH(mode_finish, dim3(bin_grid), dim3(256), 0, k.stream, mp);
    XH_VALUES_LAUNCH_CHECK(k, "mode_finish launch");
    return (int)XHIST_OK;
  };
  if (k.n_cols == 0) {  // every bin is empty: mode_finish reads nothing but the shape
    RankParams rp = {};
    rp.n_rows = k.n_rows;
    rp.nb = nb;
    if (int rc = finish(params(rp, 0))) return rc;
    k.describe("mode words=0 rows_per_launch=0 | none");
    return XHIST_OK;
  }
  SortedDomain dom;
  const int rc = sorted_domain_run(k, "mode", XHIST_RANK_MIN, 0, false, nullptr, dom, [&](const RankParams& rp, int64_t r0, int64_t nr, unsigned word_grid) {
    const ModeParams mp = params(rp, r0);
    if (hipMemsetAsync(mp.slots, 0, (size_t)(nr * nb) * 8, k.stream) != hipSuccess) return k.fail(XHIST_ERR_HIP, "mode: zeroing the slots failed");
    XH_VALUES_LAUNCH(mode_runs, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, mp);
    XH_VALUES_LAUNCH_CHECK(k, "mode_runs launch");
    return finish(mp);
  });
  if (rc != XHIST_OK) return rc;
  k.describe("mode words=%lld rows_per_launch=%lld | %s", (long long)dom.words, (long long)dom.rows_per_launch, dom.sort_line);
  return XHIST_OK;
}

// a call without columns, or a plan without bins: no entry and no counted sample.  Offsets of 0, padding over the whole width,
// an inverse of -1 (bytes of all ones).
static int unique_nothing(int64_t n_rows, int64_t n_cols, int64_t nb, int64_t size, double* out_uniques, int64_t* out_counts,
                          int64_t* out_offsets, int64_t* out_inverse, hipStream_t stream) {
  if (hipMemsetAsync(out_offsets, 0, (size_t)(n_rows * (nb + 1)) * 8, stream) != hipSuccess) return XHIST_ERR_HIP;
  if (size > 0) {
    UniqueParams up = {};
    up.r.n_rows = n_rows;
    up.r.nb = nb;
    up.out_offsets = out_offsets;
    up.out_uniques = out_uniques;
    up.out_counts = out_counts;
    up.width = size;
    const int64_t chunks = (size + kUniquePadChunk - 1) / kUniquePadChunk;
    XH_VALUES_LAUNCH(unique_pad, dim3((unsigned)std::min<int64_t>(kRankFlatGrid, n_rows * chunks)), dim3(256), 0, stream, up);
    if (hipGetLastError() != hipSuccess) return XHIST_ERR_HIP;
  }
  if (out_inverse && n_rows * n_cols > 0 && hipMemsetAsync(out_inverse, 0xff, (size_t)(n_rows * n_cols) * 8, stream) != hipSuccess)
    return XHIST_ERR_HIP;
  return XHIST_OK;
}

// The scratch of the run sums behind the sorted domain's own: per word lead and tail, per tile its element (sum and flag), and,
// `by_position`, one float64 per sample.  wruns_scratch() is its size, wruns_params() cuts it for one batch of rows.
static size_t wruns_scratch(const ValuesCall& k, bool by_position) {
  const int64_t words = (k.n_cols + 63) / 64, tiles = (words + kRankTile - 1) / kRankTile;
  return ((size_t)(k.n_rows * words) * 2 + (size_t)(k.n_rows * tiles) * 2 + (by_position ? (size_t)(k.n_rows * k.n_cols) : 0)) * 8;
}

static WrunsParams wruns_params(const ValuesCall& k, const RankParams& rp, int64_t r0, char* extra, bool by_position) {
  const int64_t nw = k.n_rows * rp.words, nt = k.n_rows * rp.tiles;
  double* const base = reinterpret_cast<double*>(extra);
  WrunsParams wp = {};
  wp.r = rp;
  wp.w = values_read(*k.third, r0);
  wp.lead = base + r0 * rp.words;
  wp.tail = base + nw + r0 * rp.words;
  wp.tsum = base + 2 * nw;  // (every batch of rows uses the head of the tiles' two arrays)
  wp.tflag = reinterpret_cast<uint64_t*>(base + 2 * nw + nt);
  if (by_position) {
    wp.out = base + 2 * nw + 2 * nt + r0 * k.n_cols;
    wp.width = k.n_cols;
  }
  return wp;
}

// the four launches that leave every run's sum at its slot
static int wruns_launch(const ValuesCall& k, const WrunsParams& wp, unsigned word_grid) {
  const unsigned tile_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, wp.r.n_rows * wp.r.tiles);
  XH_VALUES_LAUNCH(wruns_words, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, wp);
  XH_VALUES_LAUNCH_CHECK(k, "wruns_words launch");
  XH_VALUES_LAUNCH(wruns_totals, dim3(tile_grid), dim3(256), 0, k.stream, wp);
  XH_VALUES_LAUNCH_CHECK(k, "wruns_totals launch");
  XH_VALUES_LAUNCH(wruns_scan, dim3((unsigned)wp.r.n_rows), dim3(256), 0, k.stream, wp);
  XH_VALUES_LAUNCH_CHECK(k, "wruns_scan launch");
  XH_VALUES_LAUNCH(wruns_close, dim3(tile_grid), dim3(256), 0, k.stream, wp);
  XH_VALUES_LAUNCH_CHECK(k, "wruns_close launch");
  return XHIST_OK;
}

int xhist_mode_w_run(const ValuesCall& k, int64_t* out_count, int64_t* out_nunique, double* out_mode, double* out_mode_weight) {
  const int64_t nb = k.pl.n_bins;
  auto slots = [&](WrunsParams& wp, int64_t r0) {
    wp.kslot = reinterpret_cast<uint64_t*>(out_mode_weight + r0 * nb);
    wp.pslot = reinterpret_cast<uint64_t*>(out_mode + r0 * nb);
    wp.out_count = out_count + r0 * nb;
    wp.out_nunique = out_nunique + r0 * nb;
  };
  auto finish = [&](const WrunsParams& wp) {
    const unsigned bin_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (wp.r.n_rows * nb + 255) / 256);
    XH_VALUES_LAUNCH(wmode_finish, dim3(bin_grid), dim3(256), 0, k.stream, wp);
    XH_VALUES_LAUNCH_CHECK(k, "wmode_finish launch");
    return (int)XHIST_OK;
  };
  if (k.n_cols == 0) {  // every bin is empty: wmode_finish reads nothing but the shape
    WrunsParams wp = {};
    wp.r.n_rows = k.n_rows;
    wp.r.nb = nb;
    slots(wp, 0);
    if (int rc = finish(wp)) return rc;
    k.describe("wmode words=0 rows_per_launch=0 | none");
    return XHIST_OK;
  }
  SortedDomain dom;
  dom.extra_bytes = wruns_scratch(k, true);
  const int rc = sorted_domain_run(k, "wmode", XHIST_RANK_MIN, 0, false, nullptr, dom, [&](const RankParams& rp, int64_t r0, int64_t nr, unsigned word_grid) {
    WrunsParams wp = wruns_params(k, rp, r0, dom.extra, true);
    slots(wp, r0);
    if (hipMemsetAsync(wp.kslot, 0, (size_t)(nr * nb) * 8, k.stream) != hipSuccess ||
        hipMemsetAsync(wp.pslot, 0xff, (size_t)(nr * nb) * 8, k.stream) != hipSuccess)
      return k.fail(XHIST_ERR_HIP, "wmode: filling the slots failed");
    if (int rc2 = wruns_launch(k, wp, word_grid)) return rc2;
    XH_VALUES_LAUNCH(wmode_max, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, wp);
    XH_VALUES_LAUNCH_CHECK(k, "wmode_max launch");
    XH_VALUES_LAUNCH(wmode_pos, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, wp);
    XH_VALUES_LAUNCH_CHECK(k, "wmode_pos launch");
    return finish(wp);
  });
  if (rc != XHIST_OK) return rc;
  k.describe("wmode words=%lld rows_per_launch=%lld | %s", (long long)dom.words, (long long)dom.rows_per_launch, dom.sort_line);
  return XHIST_OK;
}

// bin_unique and, `weighted`, bin_weighted_unique (k.third the weights; out_weight_sums is read only then, and only for a width
// above 0): `who` is the name in the describe() line and the messages
static int unique_run(const ValuesCall& k, const char* who, bool weighted, int64_t size, double* out_uniques, int64_t* out_counts,
                      double* out_weight_sums, int64_t* out_offsets, int64_t* out_inverse) {
  const int64_t nb = k.pl.n_bins, nb1 = nb + 1;
  if (k.n_cols == 0 || nb == 0) {
    if (unique_nothing(k.n_rows, k.n_cols, nb, size, out_uniques, out_counts, out_offsets, out_inverse, k.stream) != XHIST_OK ||
        (weighted && size > 0 && hipMemsetAsync(out_weight_sums, 0, (size_t)(k.n_rows * size) * 8, k.stream) != hipSuccess))
      return k.fail(XHIST_ERR_HIP, "%s: writing the outputs of a call without columns or bins failed", who);
    k.describe("%s size=%lld inverse=%d words=0 rows_per_launch=0 | none", who, (long long)size, out_inverse ? 1 : 0);
    return XHIST_OK;
  }
  SortedDomain dom;
  if (weighted && size > 0) dom.extra_bytes = wruns_scratch(k, false);
  const int rc = sorted_domain_run(k, who, XHIST_RANK_DENSE, 0, false, nullptr, dom, [&](const RankParams& rp, int64_t r0, int64_t nr, unsigned word_grid) {
    UniqueParams up;
    up.r = rp;
    up.out_offsets = out_offsets + r0 * nb1;
    up.out_uniques = out_uniques ? out_uniques + r0 * size : nullptr;
    up.out_counts = out_counts ? out_counts + r0 * size : nullptr;
    up.out_inverse = out_inverse ? out_inverse + r0 * k.n_cols : nullptr;
    up.width = size;
    const unsigned bin_grid = (unsigned)std::min<int64_t>(kRankFlatGrid, (nr * nb + 255) / 256);
    XH_VALUES_LAUNCH(unique_bins, dim3(bin_grid), dim3(256), 0, k.stream, up);
    XH_VALUES_LAUNCH_CHECK(k, "unique_bins launch");
    XH_VALUES_LAUNCH(unique_scan, dim3((unsigned)nr), dim3(256), 0, k.stream, up);
    XH_VALUES_LAUNCH_CHECK(k, "unique_scan launch");
    if (size > 0) {
      XH_VALUES_LAUNCH(unique_runs, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, up);
      XH_VALUES_LAUNCH_CHECK(k, "unique_runs launch");
      const int64_t chunks = (size + kUniquePadChunk - 1) / kUniquePadChunk;
      XH_VALUES_LAUNCH(unique_pad, dim3((unsigned)std::min<int64_t>(kRankFlatGrid, nr * chunks)), dim3(256), 0, k.stream, up);
      XH_VALUES_LAUNCH_CHECK(k, "unique_pad launch");
    }
    if (out_inverse) {
      XH_VALUES_LAUNCH(unique_inverse, dim3(word_grid), dim3(64 * kRankWaves), 0, k.stream, up);
      XH_VALUES_LAUNCH_CHECK(k, "unique_inverse launch");
    }
    if (weighted && size > 0) {  // (a width of 0 stores no sum)
      WrunsParams wp = wruns_params(k, rp, r0, dom.extra, false);
      wp.uoff = up.out_offsets;
      wp.out = out_weight_sums + r0 * size;
      wp.width = size;
      if (int rc2 = wruns_launch(k, wp, word_grid)) return rc2;
      const int64_t chunks = (size + kWrunsPadChunk - 1) / kWrunsPadChunk;
      XH_VALUES_LAUNCH(wruns_pad, dim3((unsigned)std::min<int64_t>(kRankFlatGrid, nr * chunks)), dim3(256), 0, k.stream, wp);
      XH_VALUES_LAUNCH_CHECK(k, "wruns_pad launch");
    }
    return (int)XHIST_OK;
  });
  if (rc != XHIST_OK) return rc;
  k.describe("%s size=%lld inverse=%d words=%lld rows_per_launch=%lld | %s", who, (long long)size, out_inverse ? 1 : 0,
             (long long)dom.words, (long long)dom.rows_per_launch, dom.sort_line);
  return XHIST_OK;
}

int xhist_unique_run(const ValuesCall& k, int64_t size, double* out_uniques, int64_t* out_counts, int64_t* out_offsets,
                     int64_t* out_inverse) {
  return unique_run(k, "unique", false, size, out_uniques, out_counts, nullptr, out_offsets, out_inverse);
}

int xhist_unique_w_run(const ValuesCall& k, int64_t size, double* out_uniques, int64_t* out_counts, double* out_weight_sums,
                       int64_t* out_offsets, int64_t* out_inverse) {
  return unique_run(k, "wunique", true, size, out_uniques, out_counts, out_weight_sums, out_offsets, out_inverse);
}
