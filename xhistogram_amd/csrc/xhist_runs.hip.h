// xhist_runs.hip.h — the count / scan / scatter engine of bin_order (xhist_group.hip.h) and of every pass of bin_sort
// (xhist_sort.hip.h): a stable counting sort of a row's records by a small key, the *slot* of a record in [0, width).
//   count<W, P>    a row is cut into `chunks` contiguous chunks of `chunk` positions (a multiple of 64).  One wave64 owns one
//                  (row, chunk): it counts the slots of the chunk's records into its own `width` uint32 counters in LDS and
//                  writes them to cnt[row][chunk][width].  Counts do not depend on the order of the additions, so plain LDS adds
//                  without a return value do.
//   scan           cnt[row][chunk][slot] becomes where the (chunk, slot) run starts in the row: the exclusive prefix over slots
//                  of the totals over chunks (written to `offsets` where the caller wants it), plus the counts of the earlier
//                  chunks.  Everything of a row is below 2^31, so uint32 holds it.  A row cut into thousands of chunks is too
//                  much for the one workgroup that scans a row's slots, so the chunks go in slices of 64:
//                    totals  a workgroup per (row, tile of slots, slice), a thread per slot: part[row][slice][slot] = the
//                            slice's total
//                    scan    one workgroup per row, the slots in tiles of the block with the running sum carried from tile to
//                            tile: offsets, and part becomes the base of each (slice, slot)
//                    bases   as totals: from its slice's base, a thread rewrites the slice's 64 counters of its slot
//                  A row of one chunk is its own slice: scan runs on cnt itself and the other two are not launched.
//   scatter<W, P>  the same (row, chunk) -> wave assignment.  The wave loads its bases into its LDS counters and walks its
//                  chunk 64 consecutive records at a step.  In a step the lanes that hold the same slot find each other by one
//                  __ballot per bit of the slot; a lane's rank is the number of its peers below it; every lane reads its
//                  slot's counter, and then the lowest lane of each group adds the group's size to it.  Distinct groups hold
//                  distinct slots, so no two lanes write one counter, and no atomic is involved: the place of a record is
//                  base + rank, a function of the keys alone, and records of equal slots keep their order (the sort is stable).
// One wave owns one chunk, so the streaming loops have no workgroup barrier, and a wave's LDS operations complete in the order
// they were issued: a fence at wavefront scope (runs_wave_sync) is all that separates the counter reads of a step from its
// writes.
//
// What a record is belongs to the caller, a compile-time policy P that is also the kernel's argument:
//   P::runs                    the RunsParams of the launch
//   P::kWidth, P::kBits        the counters of a wave and the ballots of a step where the caller fixes them; 0: runs.width, and
//                              p.bits with 2^bits >= width
//   P::Key, P::Rest            a record's key, all the count reads of it, and what the scatter carries beside the key (an empty
//                              struct: nothing); a lane past the chunk's end holds key 0, whose slot is 0, and Rest{}
//   p.key(at), p.rest(at)      the two parts of the record at `at` = row * n_cols + position.  They are loaded by separate
//                              statements, each under its own test of the chunk's end, as the hand-written kernels did (why:
//                              profiles/runs_engine_resources.txt, the wait sequence of sort_scatter)
//   p.slot(key, width)         its counter
//   p.store(to, key, rest, pos)  the record from position `pos` of its row, placed at `to` = row * n_cols + place
// The bodies (runs_count_body<W>, runs_scatter_body<W>) never ask which caller they serve.  A caller's count and scatter kernels
// call them with W waves of 64 lanes per workgroup and W * width * 4 bytes of dynamic LDS.
//
// Templates and inline functions only: both units include this header.  The kernels of totals / scan / bases serve both callers,
// so one unit instantiates them (xhist_group.hip: width read from the parameters, and width 256), and the other reaches them
// through xhist_runs_scan (xhist_values_api.h).
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

constexpr int kRunsStep = 64;         // positions of one step of a wave; chunks are whole steps
constexpr int kRunsUnroll = 4;        // record loads a lane keeps in flight
constexpr int kRunsSlice = 64;        // chunks of one slice of the scan
constexpr int64_t kRunsSliceGrid = 4096;  // workgroups of totals / bases, 16 to a CU of 256: they walk their units grid-strided

// one launch over rows [r0, r0 + n_rows) of the call: every pointer is pre-advanced to r0
struct RunsParams {
  uint32_t* cnt;     // [n_rows, chunks, width]
  uint32_t* part;    // [n_rows, slices, width]; cnt itself where a row is one chunk
  int64_t* offsets;  // [n_rows, width] the exclusive prefix of a row's totals; nullptr: nowhere
  int64_t n_rows, n_cols, chunk;
  int32_t chunks, slices, width;  // width counters per wave; slices of kRunsSlice chunks
};

// threads of a workgroup of totals / scan / bases: a thread per slot of a tile
__host__ __device__ constexpr int runs_scan_block(int width) { return width <= 64 ? 64 : 256; }

// between the LDS accesses of a wave's lanes to each other's words: the hardware runs a wave's LDS operations in order, this
// keeps the compiler from moving them
__device__ __forceinline__ void runs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int W, class P>
__device__ __forceinline__ void runs_count_body(const P& __restrict__ p) {
  const RunsParams& r = p.runs;
  const int32_t width = P::kWidth ? P::kWidth : r.width;
  const int wave = threadIdx.x / kRunsStep, lane = threadIdx.x % kRunsStep;
  const int64_t unit = (int64_t)blockIdx.x * W + wave;  // (row, chunk)
  if (unit >= r.n_rows * r.chunks) return;              // (whole waves leave: nothing below waits for another wave)
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * width;
  for (int32_t b = lane; b < width; b += kRunsStep) my[b] = 0;
  runs_wave_sync();
  const int64_t row = unit / r.chunks, begin = (unit % r.chunks) * r.chunk;
  const int64_t end = begin + r.chunk < r.n_cols ? begin + r.chunk : r.n_cols;
  const int64_t r0 = row * r.n_cols;
  for (int64_t i = begin + lane; i < end + lane; i += kRunsStep * kRunsUnroll) {  // (i - lane < end: uniform)
    typename P::Key k[kRunsUnroll];
#pragma unroll
    for (int u = 0; u < kRunsUnroll; ++u) k[u] = i + u * kRunsStep < end ? p.key(r0 + i + u * kRunsStep) : 0;
#pragma unroll
    for (int u = 0; u < kRunsUnroll; ++u)
      if (i + u * kRunsStep < end) atomicAdd(&my[p.slot(k[u], width)], 1u);
  }
  runs_wave_sync();
  uint32_t* out = r.cnt + unit * width;
  for (int32_t b = lane; b < width; b += kRunsStep) out[b] = my[b];
}

// A slice's counters of one slot, per thread; the workgroups walk the (row, tile of slots, slice) units grid-strided.
// BASES false: part = their total.  BASES true: each becomes the running sum from part, the slice's base.
// WIDTH: the counters of a wave where the caller fixes them (the sort's 256), 0: p.width.  The workgroup is runs_scan_block.
template <bool BASES, int WIDTH>
__device__ __forceinline__ void runs_slices_body(const RunsParams& __restrict__ p) {
  const int32_t width = WIDTH ? WIDTH : p.width;
  const int64_t nt = WIDTH ? runs_scan_block(WIDTH) : blockDim.x, tiles = (width + nt - 1) / nt;
  const int64_t units = p.n_rows * tiles * p.slices;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u / (tiles * p.slices), b = (u / p.slices) % tiles * nt + threadIdx.x;
    const int32_t slice = (int32_t)(u % p.slices);
    if (b >= width) continue;
    const int32_t c0 = slice * kRunsSlice, c1 = c0 + kRunsSlice < p.chunks ? c0 + kRunsSlice : p.chunks;
    uint32_t* cnt = p.cnt + row * p.chunks * width + b;
    uint32_t* part = p.part + (row * p.slices + slice) * width + b;
    if constexpr (!BASES) {
      uint32_t total = 0;
      for (int32_t c = c0; c < c1; ++c) total += cnt[(int64_t)c * width];
      *part = total;
    } else {
      uint32_t run = *part;
      for (int32_t c = c0; c < c1; ++c) {
        const uint32_t t = cnt[(int64_t)c * width];
        cnt[(int64_t)c * width] = run;
        run += t;
      }
    }
  }
}

// One workgroup per row, a thread per slot, the slots in tiles of the block with the running sum carried from tile to tile.
template <int WIDTH>
__device__ __forceinline__ void runs_scan_body(const RunsParams& __restrict__ p) {
  __shared__ uint32_t s[256];
  const int32_t width = WIDTH ? WIDTH : p.width;
  const int tid = threadIdx.x, nt = WIDTH ? runs_scan_block(WIDTH) : blockDim.x;
  const int64_t row = blockIdx.x;
  uint32_t* part = p.part + row * p.slices * width;
  uint32_t carry = 0;
  for (int32_t b0 = 0; b0 < width; b0 += nt) {
    const int32_t b = b0 + tid;
    uint32_t total = 0;
    if (b < width)
      for (int32_t c = 0; c < p.slices; ++c) total += part[(int64_t)c * width + b];
    s[tid] = total;
    __syncthreads();
    for (int d = 1; d < nt; d <<= 1) {  // inclusive scan of the tile's totals
      const uint32_t t = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    const uint32_t incl = s[tid], tile = s[nt - 1];
    __syncthreads();
    if (b < width) {
      uint32_t run = carry + incl - total;
      if (p.offsets) p.offsets[row * width + b] = (int64_t)run;
      for (int32_t c = 0; c < p.slices; ++c) {
        const uint32_t t = part[(int64_t)c * width + b];
        part[(int64_t)c * width + b] = run;
        run += t;
      }
    }
    carry += tile;
  }
}

template <int W, class P>
__device__ __forceinline__ void runs_scatter_body(const P& __restrict__ p) {
  const RunsParams& r = p.runs;
  const int32_t width = P::kWidth ? P::kWidth : r.width;
  int bits = P::kBits;
  if constexpr (!P::kBits) bits = p.bits;
  const int wave = threadIdx.x / kRunsStep, lane = threadIdx.x % kRunsStep;
  const int64_t unit = (int64_t)blockIdx.x * W + wave;
  if (unit >= r.n_rows * r.chunks) return;
  uint32_t* my = reinterpret_cast<uint32_t*>(xhist_smem) + (size_t)wave * width;
  const uint32_t* base = r.cnt + unit * width;
  for (int32_t b = lane; b < width; b += kRunsStep) my[b] = base[b];
  runs_wave_sync();
  const int64_t row = unit / r.chunks, begin = (unit % r.chunks) * r.chunk;
  const int64_t end = begin + r.chunk < r.n_cols ? begin + r.chunk : r.n_cols;
  const int64_t r0 = row * r.n_cols;
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t i = begin + lane; i < end + lane; i += kRunsStep * kRunsUnroll) {
    typename P::Key k[kRunsUnroll];
    typename P::Rest q[kRunsUnroll];
#pragma unroll
    for (int u = 0; u < kRunsUnroll; ++u) {
      const bool in = i + u * kRunsStep < end;
      k[u] = in ? p.key(r0 + i + u * kRunsStep) : 0;
      q[u] = in ? p.rest(r0 + i + u * kRunsStep) : typename P::Rest{};
    }
#pragma unroll
    for (int u = 0; u < kRunsUnroll; ++u) {
      const int64_t pos = i + u * kRunsStep;
      if (pos - lane >= end) break;  // (uniform: the step lies past the chunk)
      const bool in = pos < end;
      const uint32_t slot = p.slot(k[u], width);
      uint64_t peers = __ballot(in);
      for (int bit = 0; bit < bits; ++bit) {
        const bool one = (slot >> bit) & 1u;
        const uint64_t m = __ballot(one);
        peers &= one ? m : ~m;
      }
      const uint32_t at = my[slot];  // (every lane of a group reads the same word, before its lowest lane moves it on)
      const uint32_t rank = (uint32_t)__popcll(peers & below);
      runs_wave_sync();
      if (in && rank == 0) my[slot] = at + (uint32_t)__popcll(peers);
      runs_wave_sync();
      if (in) p.store(r0 + (int64_t)at + rank, k[u], q[u], pos);
    }
  }
}

struct RunsGeometry {
  int64_t chunks = 0, chunk = 0, slices = 0, max_rows = 0;
};

// The launch geometry of a call of n_rows rows of n_cols > 0 positions on `cus` CUs, for a caller that wants `per_cu` waves on
// a CU, no chunk shorter than `min_chunk` positions unless the row is, `waves` waves in a workgroup, and at most `cap_bytes` of
// `width` counters per (row, chunk) in one launch (0: no cap):
//   chunks    rows that fill the device alone get one chunk each; fewer rows are cut until cus * per_cu waves exist, never
//             into chunks shorter than min_chunk; a chunk is whole steps of 64 positions
//   max_rows  rows per launch: workgroups below 2^31 and lanes below 2^32, for the (row, chunk) grid and for the scan's rows,
//             and the counters within the cap
static inline RunsGeometry runs_geometry(int cus, int64_t per_cu, int64_t min_chunk, int waves, int64_t cap_bytes, int64_t width,
                                         int64_t n_rows, int64_t n_cols) {
  RunsGeometry g;
  const int64_t target = (int64_t)cus * per_cu;
  const int64_t steps = (n_cols + kRunsStep - 1) / kRunsStep;
  int64_t want = std::min<int64_t>(steps, (target + n_rows - 1) / n_rows);
  want = std::max<int64_t>(1, std::min<int64_t>(want, n_cols / min_chunk));
  g.chunk = ((n_cols + want - 1) / want + kRunsStep - 1) / kRunsStep * kRunsStep;
  g.chunks = (n_cols + g.chunk - 1) / g.chunk;
  g.slices = g.chunks == 1 ? 1 : (g.chunks + kRunsSlice - 1) / kRunsSlice;
  const int64_t max_units = (((int64_t)1 << 32) - 1) / (kRunsStep * waves) * waves;
  g.max_rows = std::min<int64_t>(max_units / g.chunks, (((int64_t)1 << 32) - 1) / 256);
  if (cap_bytes) g.max_rows = std::min<int64_t>(g.max_rows, cap_bytes / (g.chunks * width * 4));
  g.max_rows = std::max<int64_t>(1, g.max_rows);
  return g;
}

// One counting sort of a batch of rows, `waves` waves to a workgroup: the caller's count kernel, the scan of its counters, the
// caller's scatter kernel.  `who` ("group", "sort") names the caller in the message of a failed launch: "<who>_count launch",
// "<who>_totals launch", ... as before the kernels were shared.
template <class P>
static int runs_pass(const ValuesCall& k, void (*count)(const P), void (*scatter)(const P), int waves, size_t lds_bytes, const P& p,
                     const char* who) {
  char what[48];  // (only XH_VALUES_LAUNCH_CHECK reads it, after a failed launch)
  const unsigned grid = (unsigned)((p.runs.n_rows * p.runs.chunks + waves - 1) / waves);
  XH_VALUES_LAUNCH(count, dim3(grid), dim3(kRunsStep * waves), lds_bytes, k.stream, p);
  XH_VALUES_LAUNCH_CHECK(k, (snprintf(what, sizeof what, "%s_count launch", who), what));
  if (int rc = xhist_runs_scan(k, p.runs, who)) return rc;
  XH_VALUES_LAUNCH(scatter, dim3(grid), dim3(kRunsStep * waves), lds_bytes, k.stream, p);
  XH_VALUES_LAUNCH_CHECK(k, (snprintf(what, sizeof what, "%s_scatter launch", who), what));
  return XHIST_OK;
}

}  // namespace xhist
