// xhist_exec_device.hip.h — host side: execution on device-resident arrays — partitioned mode, row-per-lane mode, streaming kernels
// Part of the single translation unit xhist_capi.hip (included there, in order).
#pragma once

// ------------------------------------------------------------------------------------------
// device-resident execute
// ------------------------------------------------------------------------------------------
// `out_checked`: the caller answers for its outputs itself (they are no [n_rows, n_bins] planes), and `out` is not looked at
static int validate_arrays(const xhist_plan* p, const xhist_array* samples, const xhist_array* weights, int64_t n_rows,
                           int64_t n_cols, const void* out, int out_dtype, bool out_checked = false) {
  if (!p) return fail(XHIST_ERR_INVALID, "plan is NULL");
  if (!samples) return fail(XHIST_ERR_INVALID, "samples is NULL");
  if (n_rows < 0 || n_cols < 0) return fail(XHIST_ERR_INVALID, "negative shape");
  const bool empty = n_rows == 0 || n_cols == 0;
  for (int d = 0; d < p->n_dims; ++d) {
    if (!empty && !samples[d].data) return fail(XHIST_ERR_INVALID, "samples[%d].data is NULL", d);
    if (!dtype_size(samples[d].dtype)) return fail(XHIST_ERR_INVALID, "samples[%d] has unknown dtype tag %d", d, samples[d].dtype);
    if (samples[d].row_stride < 0 || samples[d].col_stride < 0 || samples[d].inner_rows < 0 || samples[d].outer_stride < 0)
      return fail(XHIST_ERR_UNSUPPORTED, "negative strides are not supported; pass a contiguous copy");
    const bool int_dim = p->cmp == XHIST_CMP_I64 || ((p->cmp & ~0xff) == XHIST_CMP_PER_DIM && ((p->cmp >> d) & 1));
    const int sdt_d = samples[d].dtype;
    const bool unsigned_dt = sdt_d == XHIST_U64 || sdt_d == XHIST_U32 || sdt_d == XHIST_U16 || sdt_d == XHIST_U8 || sdt_d == XHIST_BOOL;
    if (int_dim && p->uns && !unsigned_dt)
      return fail(XHIST_ERR_UNSUPPORTED, "unsigned int64 compare domain needs unsigned integer samples (got dtype tag %d)", sdt_d);
    if (int_dim && !p->uns && (!dtype_is_int(sdt_d) || sdt_d == XHIST_U64))
      return fail(XHIST_ERR_UNSUPPORTED, "int64 compare domain needs signed/small integer samples (got dtype tag %d)", sdt_d);
  }
  if (weights) {
    if (!empty && !weights->data) return fail(XHIST_ERR_INVALID, "weights.data is NULL");
    if (!dtype_size(weights->dtype)) return fail(XHIST_ERR_INVALID, "weights has unknown dtype tag %d", weights->dtype);
    if (weights->row_stride < 0 || weights->col_stride < 0 || weights->inner_rows < 0 || weights->outer_stride < 0)
      return fail(XHIST_ERR_UNSUPPORTED, "negative strides are not supported; pass a contiguous copy");
    if (out_dtype != XHIST_F64) return fail(XHIST_ERR_INVALID, "weighted histograms are float64 (out_dtype XHIST_F64)");
  } else if (out_dtype != XHIST_I64) {
    return fail(XHIST_ERR_INVALID, "unweighted histograms are int64 (out_dtype XHIST_I64)");
  }
  if (!out_checked && !out && n_rows * p->n_bins > 0) return fail(XHIST_ERR_INVALID, "out is NULL");
  return XHIST_OK;
}

// zero n 8-byte output words on `stream` (see zero_words)
static int zero_output(void* out, int64_t n_words, hipStream_t stream) {
  if (n_words <= 0) return XHIST_OK;
  const int grid = (int)std::min<int64_t>(2048, (n_words + 255) / 256);
  HIPC((hipError_t)xhist_hot_zero_words(static_cast<unsigned long long*>(out), n_words, grid, stream));  // (the kernel lives in the small hot code object)
  return XHIST_OK;
}

static const void* advance(const void* base, int dt, int64_t elems) {
  return static_cast<const char*>(base) + elems * dtype_size(dt);
}

// The arrays a call reads, in order: samples[0 .. D), then the weights (index D) when there are any.
static int n_arrays(int D, const xhist_array* weights) { return weights ? D + 1 : D; }
static const xhist_array& array_at(const xhist_array* samples, const xhist_array* weights, int D, int d) {
  return d < D ? samples[d] : *weights;
}

// A Params with the arrays of a call (samples[0 .. D), then the weights when there are any) as they are, their tables and
// shape, and the histogram; every other field zero.  Each launch adds its own.
static Params fill_params(const xhist_array* samples, const xhist_array* weights, int D, const TableSet& tset, int32_t table_words,
                          int64_t n_rows, int64_t n_cols, int64_t n_bins, void* out) {
  Params kp;
  memset(&kp, 0, sizeof kp);
  for (int d = 0; d < D; ++d) {
    const xhist_array& a = samples[d];
    kp.s_ptr[d] = a.data;
    kp.s_rs[d] = a.row_stride;
    kp.s_cs[d] = a.col_stride;
    kp.s_ir[d] = a.inner_rows;
    kp.s_os[d] = a.outer_stride;
    kp.s_dt[d] = a.dtype;
    kp.dim[d] = tset.dim[d];
  }
  if (weights) {
    kp.w_ptr = weights->data;
    kp.w_rs = weights->row_stride;
    kp.w_cs = weights->col_stride;
    kp.w_ir = weights->inner_rows;
    kp.w_os = weights->outer_stride;
    kp.w_dt = weights->dtype;
  }
  kp.n_dims = D;
  kp.tables = tset.blob;
  kp.table_words = table_words;
  kp.tables_in_lds = 1;
  kp.n_rows = n_rows;
  kp.n_cols = n_cols;
  kp.n_bins = n_bins;
  kp.out = out;
  return kp;
}

// The exchange mode's kernel wants every compute unit for itself (256 persistent workgroups that wait for one another): two
// of them running on two streams of one GPU would each hold part of the chip and wait for the rest until their deadlines.
// So a call whose stream is not the one the last exchange kernel of this device went to looks at that kernel's event first
// and takes the classic passes when it has not finished.  (Other people's kernels on other streams can still hold compute
// units back; that costs the deadline once and takes the plan off the mode — exchange_bookkeeping.)
struct ExchInFlight {
  std::mutex mu;
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;
  bool armed = false;
};
static ExchInFlight& exch_in_flight(int device) {
  static ExchInFlight slots[64];
  return slots[device & 63];
}
// fl.mu held: the last exchange kernel of this device went to another stream and may still be running
static bool exchange_running_elsewhere(ExchInFlight& fl, hipStream_t stream) {
  const bool busy = fl.armed && fl.stream != stream && hipEventQuery(fl.ev) == hipErrorNotReady;
  (void)hipGetLastError();
  return busy;
}

static bool exact_records_env() {
  static const bool v = [] { const char* e = getenv("XHIST_AMD_EXACT_RECORDS"); return e && *e && *e != '0'; }();
  return v;
}

static kernel_fn_route route_kernel(int sdt, int wdt, int D, int scan, bool multi, int block, int spl = 4) {
  if (block != 1024) return nullptr;
  if (spl == 8) return sdt == XHIST_F64 ? xhist_pick_route_f64_b1024s8(wdt, D, scan, multi) : sdt == XHIST_F32 ? xhist_pick_route_f32_b1024s8(wdt, D, scan, multi) : nullptr;
  if (spl != 4) return nullptr;
  return sdt == XHIST_F64 ? xhist_pick_route_f64_b1024(wdt, D, scan, multi) : sdt == XHIST_F32 ? xhist_pick_route_f32_b1024(wdt, D, scan, multi) : nullptr;
}

// Geometry of the routing pass: 1024-thread workgroups, 4 or 8 samples per lane and tile ("route_spl" override).
// Long tiles — 1024 threads x 8 samples, 64 KB read per input and tile — are what the mixed read/write traffic of the pass
// wants (tools/ubench/mixbw `mb`: 24 B read : 8 B written per sample runs at 4.8-5.6 TB/s with 32 KB bursts per workgroup and
// at 5.7-6.0 with 64 KB and more), as long as the tile's samples and weights fit the 128 registers a lane of a 1024-thread
// workgroup has: 2 x (bytes of one sample of every input + bytes of its weight) registers hold the tile, and up to 32 of
// them leave room for the rest (24 with table lookups, which take more registers than the arithmetic digitize).
// Measured over 5*10^8 samples, ms per call, 1024 x 4 -> 1024 x 8 | 2 x 512 x 4 (profiles/r03_s8_route_geometry.txt):
//   counts:  f64 pair 2.58 -> 2.40;  f64, 10^6 bins 1.82 -> 1.58;  f32 pair 1.98 -> 1.60 | 1.96;  f32 triple (3*10^8) 1.39 -> 1.20
//            | 1.57;  f64 triple (48 registers) 2.13 -> 2.19 (stays at 4)
//   f32 weights:  f32 pair 2.92 -> 2.64 | 3.62;  f32, 10^6 bins 2.47 -> 2.26 | 3.21;  f64, 10^6 bins 2.78 -> 2.55 | 3.33;
//            f64 pair (40 registers) 3.51 -> 3.49 | 4.12;  32 rows of 3*10^7 f32 pairs, 400 x 400 bins 5.42 -> 4.44 | 5.88
//   f64 weights, packed records:  f32 pair 3.20 -> 3.03 | 3.32;  f32, 10^6 bins 3.02 -> 2.77 | 3.00;
//            f32 triple (40 registers) 2.16 -> 2.47 | 2.26
//   f64 samples AND f64 weights are the exception to the register count: the long tile loses (C5 4.13 -> 4.52, it spills;
//   10^6 bins 3.36 -> 3.57) and they keep 1024 x 4.
// Two 512-thread workgroups per CU (VERDICT r2 "next" #1b: one's loads and stores under the other's arithmetic) beat one of
// 1024 by 2-3 % on C5 while the pass loaded its weights with the samples (3.43-3.48 -> 3.35-3.37 ms,
// profiles/r03_c5_blocks.txt); with the weights loaded a tile later and the arithmetic digitize they lose everywhere
// (C5 3.94 | 4.11, uniform 3.93 | 4.12, 10^6 bins 3.28 | 3.32, 8 rows x 512 x 512 bins 3.82 | 3.89; exact float64 records
// 4.21 | 4.32): the 512-thread instantiations were removed in round 5.
struct RouteGeom {
  int block, spl;
};
// Table lookups (edges that are not arithmetic) take more registers than the arithmetic digitize: 24 there.
static RouteGeom route_geom_for(const PlanKnobs& kn, int sdt, int wdt /* -1: counts */, int D, int scan) {
  RouteGeom g;
  g.block = 1024;
  // (route_long_tile_ok, xhist_pick.hip.h: the same rule decides which long-tile kernels exist; a forced 8 without one falls to 4)
  const bool long_ok = route_long_tile_ok(sdt == XHIST_F64 ? 8 : 4, wdt == XHIST_F64 ? 8 : wdt == XHIST_F32 ? 4 : 0, D, scan == kScanArith);
  g.spl = kn.route_spl == 4 ? 4 : (long_ok ? 8 : 4);
  return g;
}

// The digitize and geometry of the partitioned mode's one routing pass (route_digitize).
struct RouteDigitize {
  int scan;
  const TableSet* tset;
  bool f32;
  RouteGeom geom;
};

// What execute_partitioned_rows hands, unchanged, to every execute_partitioned and execute_partitioned_fused call of an execute.
struct PartCall {
  int sdt, wdt;  // wdt: -1 without weights
  int64_t n_cols;
  int shift, parts_per_row;
  int scan;  // count + prefix + scatter: the streaming choice's digitize
  bool use_f32;
  const TableSet* tset;
  RouteDigitize route;  // the one routing pass: its own digitize
  LaunchRecord* rec;    // one timing record per execute: opened before the first row's kernels, closed after the last row's
};

// The Params fields both forms of the partitioned mode share: the row views (unit column stride: the vector family, see
// execute_partitioned_rows; one row or rows at one stride, no groups: row_views), the tables, the histogram and its
// partitions.  Each caller adds its own: segs, and the record streams or parts_per_row.
static Params partitioned_params(const xhist_plan* p, const PartCall& pc, const xhist_array* samples, const xhist_array* weights,
                                 void* out, const TableSet& tset, int32_t table_words, int64_t rows, int n_parts) {
  Params kp = fill_params(samples, weights, p->n_dims, tset, table_words, rows, pc.n_cols, p->n_bins, out);
  kp.part_shift = pc.shift;
  kp.n_parts = n_parts;
  return kp;
}

// Partitioned mode (xhist_partition.hip.h): count -> prefix -> scatter -> accumulate, all on
// `stream`, scratch from the stream-ordered allocator (so concurrent callers never share it).
static int execute_partitioned(xhist_plan* p, const PlanKnobs& kn, const PartCall& pc, const xhist_array* samples,
                               const xhist_array* weights, void* out, hipStream_t stream, bool first, bool last) {
  const int D = p->n_dims;
  const bool weighted = weights != nullptr;
  const int64_t n_cols = pc.n_cols;
  const int sdt = pc.sdt, wdt = pc.wdt, scan = pc.scan, shift = pc.shift, n_parts = pc.parts_per_row;
  if (n_cols >= ((int64_t)1 << 40)) return XHIST_ERR_UNSUPPORTED;
  int vec = 1;
  kernel_fn_count k_count = (kernel_fn_count)fast_kernel(sdt, wdt, D, scan, kHistPartCount, &vec);
  if (!k_count) return XHIST_ERR_UNSUPPORTED;
  // records leave part_scatter in aligned groups: 8 (one 16-byte code store) while the carried
  // records of all partitions fit LDS next to the tile, else 4
  const int grp = n_parts <= 128 ? 8 : 4;
  kernel_fn_scatter k_scatter;
  if (grp == 8)
    k_scatter = wdt < 0 ? (kernel_fn_scatter)part_scatter<NoWeight, 8>
                        : (wdt == XHIST_F64 ? (kernel_fn_scatter)part_scatter<double, 8> : (kernel_fn_scatter)part_scatter<float, 8>);
  else
    k_scatter = wdt < 0 ? (kernel_fn_scatter)part_scatter<NoWeight, 4>
                        : (wdt == XHIST_F64 ? (kernel_fn_scatter)part_scatter<double, 4> : (kernel_fn_scatter)part_scatter<float, 4>);
  const int32_t table_words = scan == kScanArith ? 0 : pc.tset->words;  // arithmetic edges: no tables
  const size_t table_bytes = (size_t)table_words * 8;
  const size_t lds_count = table_bytes + (size_t)(n_parts + 1) * 32 * 4;
  const size_t lds_scatter = part_scatter_lds(n_parts, grp, weighted);
  const size_t lds_acc = (size_t)((1u << shift) + 1) * (weighted ? 8 : 4);  // + the trash slot of padding records
  if (lds_count > p->lds_max || lds_scatter > p->lds_max || lds_acc > p->lds_max) return XHIST_ERR_UNSUPPORTED;
  const int per_cu = std::max<int>(1, std::min<int>(4, (int)(160 * 1024 / std::max(lds_count, lds_scatter))));
  const int64_t n_tiles = (n_cols + kPartTile - 1) / kPartTile;
  const int G = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)p->cus * per_cu, n_tiles));
  const int Gb = (int)std::max<int64_t>(1, std::min<int64_t>(p->cus, (n_cols + 65535) / 65536));

  ScratchScope scratch(stream);
  uint32_t* d_counts = nullptr;
  uint64_t *d_base = nullptr, *d_offsets = nullptr;
  uint16_t* d_codes = nullptr;
  void* d_w = nullptr;  // record weights: float64, or float32 when the caller's weights are
  uint32_t* d_flat = nullptr;
  HIPC(scratch.alloc((void**)&d_counts, (size_t)G * n_parts * 4));
  HIPC(scratch.alloc((void**)&d_base, (size_t)G * n_parts * 8));
  HIPC(scratch.alloc((void**)&d_offsets, (size_t)(n_parts + 1) * 8));
  HIPC(scratch.alloc((void**)&d_flat, (size_t)n_tiles * kPartTile * 4));
  const size_t n_rec = (size_t)n_cols + (size_t)G * n_parts * grp;  // every slice rounded up to whole groups
  HIPC(scratch.alloc((void**)&d_codes, n_rec * 2 + 16));
  const bool rec_f32 = wdt == XHIST_F32;
  if (weighted) HIPC(scratch.alloc(&d_w, n_rec * (rec_f32 ? 4 : 8) + 16));

  Params kp = partitioned_params(p, pc, samples, weights, out, *pc.tset, table_words, 1, n_parts);
  kp.segs = G;
  kp.part_counts = d_counts;
  kp.part_base = d_base;
  kp.part_codes = d_codes;
  kp.part_w = static_cast<double*>(d_w);

  HIPC(set_dynamic_lds((const void*)k_count, lds_count));
  HIPC(set_dynamic_lds((const void*)k_scatter, lds_scatter));
  kernel_fn_acc k_acc = weighted ? (rec_f32 ? (kernel_fn_acc)part_accumulate<true, float> : (kernel_fn_acc)part_accumulate<true, double>)
                                 : (kernel_fn_acc)part_accumulate<false, double>;
  HIPC(set_dynamic_lds((const void*)k_acc, lds_acc));

  if (first)
    if (int rrc = pc.rec->begin(kn.profile)) return rrc;
  XH_LAUNCH_PICKED(k_count, dim3(G), dim3(kPartBlock), lds_count, stream, kp, d_flat);
  HIPC(hipGetLastError());
  XH_LAUNCH_PICKED_LOCAL(part_prefix, dim3(1), dim3(1024), 0, stream, (const uint32_t*)d_counts, G, n_parts, grp, d_offsets, d_base);
  HIPC(hipGetLastError());
  XH_LAUNCH_PICKED(k_scatter, dim3(G), dim3(kPartBlock), lds_scatter, stream, (const uint32_t*)d_flat,
                     weighted ? weights->data : nullptr, n_cols, (const uint64_t*)d_base, d_codes, d_w, shift, n_parts);
  HIPC(hipGetLastError());
  XH_LAUNCH_PICKED(k_acc, dim3(Gb), dim3(1024), lds_acc, stream, (const uint16_t*)d_codes, (const void*)d_w,
                     (const uint64_t*)d_offsets, out, p->n_bins, shift, n_parts);
  HIPC(hipGetLastError());
  if (!last) return XHIST_OK;
  char desc[384];
  snprintf(desc, sizeof desc,
           "family=fast hist=partitioned parts=%d bins_per_part=%d group=%d vec=%d tile=%d block=%d grid=%d acc_grid=%d "
           "lds_count=%zu lds_scatter=%zu lds_acc=%zu scan=%d weighted=%d D=%d cmp=%s",
           n_parts, 1 << shift, grp, vec, kPartTile, kPartBlock, G, Gb, lds_count, lds_scatter, lds_acc, scan, (int)weighted, D,
           pc.use_f32 ? "f32thr" : "f64");
  return pc.rec->end(desc);
}

// ---- execute_partitioned_fused and its steps ----------------------------------------------------------------------------

// The pinned host words the GPU writes for a plan: [0] a call met weights of both signs, [1] a chunk pool ran dry, [2..5] the
// exchange mode's notes (ExchArgs::note).
static void ensure_mixed_hint(xhist_plan* p) {
  if (p->mixed_hint) return;
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->mixed_hint) return;
  uint32_t* h = nullptr;
  if (hipHostMalloc((void**)&h, 64, hipHostMallocDefault) == hipSuccess) { memset(h, 0, 64); p->mixed_hint = h; }
  else (void)hipGetLastError();
}

// An exchange kernel of an earlier call gave up IN FLIGHT (a wait that outlived its deadline, a placement other than 32
// workgroups per XCD) and the classic passes took that call: the plan stays away from the mode for its next 16 eligible
// calls, twice as many after every further abort (a second hang would cost its deadline again), and is admitted again after
// that; a clean call resets the count.  (Workgroups that were not all resident at the START cost arrive_ticks, not the
// deadline, and do not count: note[5].)  "exchange" set again forgets all of it.  Returns the calls still to skip.
static int exchange_bookkeeping(xhist_plan* p) {
  std::lock_guard<std::mutex> lk(p->mu);
  ExchangeState& xs = p->exch;
  if (p->mixed_hint) {
    if (p->mixed_hint[2] != xs.aborts_seen) {
      xs.aborts_seen = p->mixed_hint[2];
      xs.skip = xs.backoff;
      xs.backoff = std::min(xs.backoff * 2, 4096);
    } else if (xs.skip > 0) {
      xs.skip -= 1;
    } else if (xs.ran_last) {
      xs.backoff = 16;
    }
    xs.ran_last = false;
  }
  return xs.skip;
}

// The routing and adding-up passes of one call: kernels, records, LDS, grids and the chunk pool.
struct RoutePlan {
  kernel_fn_route k_route = nullptr, k_route48 = nullptr;  // (k_route48: packed records only)
  kernel_fn_acc_chunks k_acc = nullptr, k_acc48 = nullptr;
  bool pack = false;  // packed 8-byte records first (float64 weights), exact ones only if both signs turn up
  int block = 0, tile = 0;
  int32_t table_words = 0;
  size_t lds_route = 0, lds_acc = 0;
  int G = 0, Gb = 0;  // workgroups of the routing / adding-up pass
  int lg = 0;         // log2 of the records per chunk
  int64_t pool_chunks = 0, ctr_words = 0;
};

// Decided before anything is allocated or launched: XHIST_ERR_UNSUPPORTED where the LDS or the chunk pool does not fit.
static int plan_route(const xhist_plan* p, const PlanKnobs& kn, kernel_fn_route k_route, int sdt, int wdt, bool weighted, int scan,
                      const TableSet& tset, int shift, int n_parts, int rows, int64_t n_cols, RouteGeom geom, RoutePlan& rp) {
  const int D = p->n_dims;
  const int block = geom.block, spl = geom.spl;
  rp.k_route = k_route;
  rp.block = block;
  rp.pack = weighted && wdt == XHIST_F64 && kn.records48_pref >= 0 && !exact_records_env();
  if (rp.pack && (!p->mixed_hint || *p->mixed_hint != 0u)) rp.pack = false;  // (earlier calls met both signs: straight to exact records)
  rp.k_route48 = rp.pack ? route_kernel(sdt, kWdtPacked48, D, scan, rows > 1, block, spl) : nullptr;
  if (rp.pack && !rp.k_route48) rp.pack = false;
  const bool rec_f32 = wdt == XHIST_F32;
  rp.k_acc = weighted ? (rec_f32 ? (kernel_fn_acc_chunks)part_accumulate_chunks<true, float>
                                 : (kernel_fn_acc_chunks)part_accumulate_chunks<true, double>)
                      : (kernel_fn_acc_chunks)part_accumulate_chunks<false, double>;
  rp.k_acc48 = (kernel_fn_acc_chunks)part_accumulate_chunks<true, double, true>;
  rp.table_words = scan == kScanArith ? 0 : tset.words;  // arithmetic edges: no tables
  const int tile = rp.tile = route_tile(block, spl);
  rp.lds_route = part_route_lds((size_t)rp.table_words * 8, n_parts, weighted, tile, block);
  const size_t hist_bytes = (size_t)((1u << shift) + 1) * (weighted ? 8 : 4);
  rp.lds_acc = ((hist_bytes + 15) & ~(size_t)15) + (size_t)kAccBatch * 8 + (size_t)(n_parts + 1) * 4 + 16;
  if (rp.lds_route > p->lds_max || rp.lds_acc > p->lds_max) return XHIST_ERR_UNSUPPORTED;
  // (Round 4 also ran the adding-up pass of sample sub-batch k on a second stream under the routing pass of sub-batch k + 1:
  // 25-60 % slower, both passes scale with the compute units they get — DESIGN_HISTORY 4.2b, profiles/r04_b_*; removed in
  // round 5.)
  const int64_t n_piece = n_cols * rows;  // samples one routing pass sees
  const int64_t n_tiles = ((n_cols + tile - 1) / tile) * rows;
  // workgroups resident per CU: by LDS — and by registers: the routing pass is held to 128 per lane (waves_per_eu 4), so a
  // CU holds 1024 of its threads.  (Sized by LDS alone, a 77 KB workgroup of 1024 threads got a grid of 2 per CU, ran it
  // in two rounds, and 10^7 float64 pairs + weights into 512 x 512 bins took 0.233 ms against 0.170 for the three-pass route.)
  const int per_cu = std::max<int>(1, std::min<int>(std::min<int>(4, 1024 / block), (int)((size_t)160 * 1024 / rp.lds_route)));
  rp.G = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)p->cus * per_cu, n_tiles));
  rp.Gb = (int)std::max<int64_t>(1, std::min<int64_t>(p->cus, (n_piece + 65535) / 65536));
  if (kn.route_grid) rp.G = (int)std::min<int64_t>(kn.route_grid, n_tiles);
  if (kn.acc_grid) rp.Gb = kn.acc_grid;
  // chunk size: a workgroup files at most kRouteListCap chunks (its list lives in LDS), 2^10 .. 2^14 records each
  int lg = 10;
  while (lg < 14 && (((n_piece / rp.G) + tile) >> lg) + n_parts + 16 > route_list_cap(block)) ++lg;
  rp.lg = lg;
  const int64_t GP = (int64_t)rp.G * n_parts;
  // Chunks that hold records: every chunk but the one in use by its (workgroup, partition) owner is full, and at most 7
  // padding records are added per owner.  Ids taken from the pool but never used: a workgroup's stock drops fewer ids than
  // its largest request whenever a range of `batch` ids runs out (batch >= 8 x that request: < 1/7 of the ids it served),
  // and ends with at most two ranges in hand.
  const int64_t used = ((n_piece + 7 * GP) >> lg) + GP;
  rp.pool_chunks = used + used / 6 + (int64_t)rp.G * (2 * route_batch(n_parts, lg, tile) + 2 * route_max_need(lg, tile)) + 64;
  // "route_pool_pct" < 100 (tests): a pool too small on purpose — what finds no chunk goes straight into the output
  if (kn.route_pool_pct > 0 && kn.route_pool_pct < 100) rp.pool_chunks = std::max<int64_t>(1, rp.pool_chunks * kn.route_pool_pct / 100);
  if (rp.pool_chunks >= ((int64_t)1 << 31) || (rp.pool_chunks << lg) >= ((int64_t)1 << 44)) return XHIST_ERR_UNSUPPORTED;
  rp.ctr_words = (2 + n_parts + 1) / 2 + 1;  // [0] pool, [1] signs seen, [2 .. 2 + P) chunks filed per partition; two sets (packed + exact)
  return XHIST_OK;
}

// The exchange mode (xhist_exchange.hip.h): packed records that never go through HBM — one persistent workgroup per compute
// unit keeps rows of a WINDOW of the histogram in LDS, records travel through rings inside each XCD.  Offered for float64
// samples + float64 weights on arithmetic edges, one row, on the 8 x 32-CU chip; whether a call takes it is decided on the
// GPU by the probe (the window must hold >= 88 % of the samples) — the classic packed kernels are queued all the same
// and return at once when it does.  "exchange" = -1 / 1: never / whenever it can run (any size, any coverage: tests).
struct ExchPlan {
  bool on = false;     // eligible: the exchange kernels are launched unless their occupancy or another stream's exchange kernel says no
  bool exact = false;  // full float64 records: 12 bytes through two rings
  kernel_fn_exch k_xch = nullptr, k_xprobe = nullptr;
  size_t lds = 0;
  // one block for everything that is zeroed per call (one launch): control words | window, cold arguments, probe counts | side copy | rings
  size_t ctl_bytes = 0, words_bytes = 0, side_bytes = 0, rings_bytes = 0;
  ExchArgs xa;  // everything but the scratch pointers and the sign word
};

static ExchPlan plan_exchange(const xhist_plan* p, const PlanKnobs& kn, const xhist_array* samples, const xhist_array* weights,
                              int64_t n_cols, int rows, int sdt, int wdt, bool pack, int exch_skip) {
  const int D = p->n_dims;
  ExchPlan xp;
  memset(&xp.xa, 0, sizeof xp.xa);
  // float64 weights that travel as FULL float64 records ("records48" = -1, XHIST_AMD_EXACT_RECORDS, or a plan that has met weights of
  // both signs): the exchange mode takes these too, with 12-byte records through two rings (part_exchange<D, true>, round 6)
  // (by default for joint histograms only: measured over the shape matrix of tools/exchange_cliffs.py with exact records,
  //  3*10^8 samples, 2-3 inputs read 0.93-1.03 of the classic exact passes — whose own time moves by 10 % from process to process
  //  and size to size with the placement of their five streams, while this form does not: C5 4.14-4.18 ms in every process against
  //  4.09 | 4.50-4.53 — and ONE input reads 1.08-1.11: profiles/r06_e_*)
  const bool xexact = weights && wdt == XHIST_F64 && !pack && rows == 1 && (D >= 2 || kn.exchange_pref > 0);
  if (!((pack || xexact) && rows == 1 && kn.exchange_pref >= 0 && (exch_skip == 0 || kn.exchange_pref > 0) && sdt == XHIST_F64 && p->arith &&
        kn.arith_pref >= 0 && D <= 3 && p->cus == kExchXcds * kExchRings &&
        p->n_bins <= ((int64_t)1 << 23) /* (the side copy is zeroed per call) */ && (kn.exchange_pref > 0 || n_cols >= ((int64_t)1 << 25))))
    return xp;
  const int64_t L = D >= 2 ? (int64_t)p->ts[0][0].dim[D - 1].nb : 256;
  const int64_t hist_rows = D >= 2 ? p->n_bins / L : (p->n_bins + 255) / 256;
  const int64_t units = (hist_rows + kExchUnitRows - 1) / kExchUnitRows;
  const int64_t max_local = xexact ? kExchMaxLocalExact : kExchMaxLocal;
  const int64_t rows_per = L <= max_local ? std::min<int64_t>(max_local / L, units) : 0;
  xp.k_xch = xhist_pick_exchange(D, xexact);
  xp.k_xprobe = xhist_pick_exchange_probe(D);
  xp.lds = rows_per >= 1 ? exchange_lds((int)(rows_per * L), xexact) : 0;
  if (!(rows_per >= 1 && units <= 4096 && xp.k_xch && xp.k_xprobe && xp.lds <= p->lds_max)) return xp;
  xp.on = true;
  xp.exact = xexact;
  ExchArgs& xa = xp.xa;
  xa.row_len = L;
  xa.n_hist_rows = hist_rows;
  xa.rows_per = (int32_t)rows_per;
  xa.local_bins = (int32_t)(rows_per * L);
  xa.n_units = (int32_t)units;
  xa.force = kn.exchange_pref > 0 ? 1 : 0;
  { int64_t p2 = 1; while (p2 * 2 <= L) p2 *= 2; xa.side_rot_mask = (int32_t)(p2 - 1); }
  xa.min_ppm = kn.exchange_min_pct > 0 ? kn.exchange_min_pct * 10000 : kExchMinPpm;
  xa.max_uneven_ppm = 1250000;
  xa.budget_ticks = kn.exchange_budget_ms < 0 ? 0 : (long long)(kn.exchange_budget_ms ? kn.exchange_budget_ms : 500) * 100000;
  xa.arrive_ticks = (long long)(kn.exchange_arrive_us > 0 ? kn.exchange_arrive_us : 200) * 100;  // 200 us: the launch of 256 workgroups on a free chip takes a few
  for (int d = 0; d < D; ++d) {  // (the arithmetic-edge constants of the float64 table set, whatever the classic routing pass digitizes with)
    const DimTable& t = p->ts[0][0].dim[d];
    xa.s_ptr[d] = static_cast<const double*>(samples[d].data);
    xa.dim[d].e0 = t.e0_f;
    xa.dim[d].eL = t.eL_f;
    xa.dim[d].step = t.step;
    xa.dim[d].inv_step = t.inv_step;
    xa.dim[d].arith_h = t.arith_h;
    xa.dim[d].nb = t.nb;
  }
  xa.w_ptr = static_cast<const double*>(weights->data);
  xa.n = n_cols;
  xa.note = p->mixed_hint;
  xp.words_bytes = ((size_t)(units + kExchRings + 8 + 32) * 4 + 7) & ~(size_t)7;  // win[8], the cold arguments (32 words), the probe's counts (units, then owners)
  xp.ctl_bytes = sizeof(ExchCtl) * kExchXcds;
  xp.side_bytes = (size_t)(hist_rows * L) * 8;  // (whole rows: exch_side_index rotates inside a row)
  xp.rings_bytes = (size_t)kExchXcds * kExchRings * kExchRings * kExchCap * (xexact ? 12 : 8);  // (exact records: the ring of low bits behind the ring of packed words)
  static_assert(sizeof(ExchCtl) % 8 == 0, "the block's parts stay 8-byte aligned");
  return xp;
}

// Every workgroup of the exchange kernel must be resident (they wait for one another): one per compute unit is what its LDS
// and registers must allow.  Asked once per plan, kernel and LDS size (a kernel of the host's that holds compute units at run
// time is the deadline's business).
static bool exchange_fits(xhist_plan* p, kernel_fn_exch k, size_t lds) {
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->exch.occ_fn == (const void*)k && p->exch.occ_lds == lds) return p->exch.occ_ok;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k, kExchBlock, lds) != hipSuccess) { per_cu = 0; (void)hipGetLastError(); }
  std::lock_guard<std::mutex> lk(p->mu);
  p->exch.occ_fn = (const void*)k;
  p->exch.occ_lds = lds;
  p->exch.occ_ok = per_cu >= 1;
  return p->exch.occ_ok;
}

// The call's scratch: the chunk pool and its counters (returned as the RouteArgs of the first counter set), and the exchange
// mode's blocks when it is on.  Ends with the kernels' LDS limits raised; clears xp.on when the exchange kernel cannot be resident.
static int alloc_fused(ScratchScope& scratch, xhist_plan* p, const RoutePlan& rp, int n_parts, bool weighted, bool rec_f32,
                       ExchPlan& xp, RouteArgs& ra) {
  const size_t plist_elems = (size_t)n_parts * rp.pool_chunks, pool_recs = ((size_t)rp.pool_chunks << rp.lg);
  memset(&ra, 0, sizeof ra);
  HIPC(scratch.alloc((void**)&ra.pool, (size_t)rp.ctr_words * 8 * 2));  // (two counter sets of ctr_words 8-byte words each)
  HIPC(scratch.alloc((void**)&ra.plist, plist_elems * 4));
  HIPC(scratch.alloc((void**)&ra.cmeta, (size_t)rp.pool_chunks * 4));
  HIPC(scratch.alloc((void**)&ra.codes, pool_recs * 2));
  if (weighted) HIPC(scratch.alloc(&ra.wrec, pool_recs * (rec_f32 ? 4 : 8)));
  ra.pcount = ra.pool + 2;
  ra.list_cap = (uint32_t)rp.pool_chunks;
  ra.chunk_log2 = rp.lg;
  ra.flags = ra.pool + 1;
  ra.dry = p->mixed_hint ? p->mixed_hint + 1 : nullptr;

  if (xp.on) {
    void *x_ctl = nullptr, *x_part = nullptr;
    ExchArgs& xa = xp.xa;
    HIPC(scratch.alloc(&x_ctl, xp.ctl_bytes + xp.words_bytes + xp.side_bytes + xp.rings_bytes));
    HIPC(scratch.alloc(&x_part, (size_t)kExchXcds * kExchRings * (size_t)xa.local_bins * 8));
    char* const base = static_cast<char*>(x_ctl);
    xa.ctl = static_cast<ExchCtl*>(x_ctl);
    xa.win = reinterpret_cast<uint32_t*>(base + xp.ctl_bytes);
    xa.side = reinterpret_cast<double*>(base + xp.ctl_bytes + xp.words_bytes);
    xa.rings = reinterpret_cast<uint64_t*>(base + xp.ctl_bytes + xp.words_bytes + xp.side_bytes);
    xa.rings_lo = xp.exact ? reinterpret_cast<uint32_t*>(xa.rings + (size_t)kExchXcds * kExchRings * kExchRings * kExchCap) : nullptr;
    xa.part = static_cast<double*>(x_part);
    xa.cold = reinterpret_cast<ExchCold*>(xa.win + 8);
    static_assert(sizeof(ExchCold) <= 32 * 4, "the cold arguments fit their 32 words");
    xa.counts = xa.win + 8 + 32;
    xa.flags = ra.pool + 1;
    HIPC(set_dynamic_lds((const void*)xp.k_xch, xp.lds));
    if (!exchange_fits(p, xp.k_xch, xp.lds)) xp.on = false;
  }

  HIPC(set_dynamic_lds((const void*)rp.k_route, rp.lds_route));
  HIPC(set_dynamic_lds((const void*)rp.k_acc, rp.lds_acc));
  if (rp.pack) {
    HIPC(set_dynamic_lds((const void*)rp.k_route48, rp.lds_route));
    HIPC(set_dynamic_lds((const void*)rp.k_acc48, rp.lds_acc));
  }
  return XHIST_OK;
}

// The exchange kernels of one call: zero their block, probe, pick, exchange.  Clears xp.on (and launches nothing) while an
// exchange kernel of another stream may still be running on this device.
static int launch_exchange(xhist_plan* p, hipStream_t stream, ExchPlan& xp) {
  // Invariant: at most one exchange kernel per device is in flight at a time, so two of them never each hold part of the chip
  // and wait for the rest.  The lock is held from the look at the last exchange kernel's event to the record of this call's, so
  // two host threads that both see "idle" can never both launch one.
  ExchInFlight& fl = exch_in_flight(p->device);
  std::lock_guard<std::mutex> lk(fl.mu);
  if (exchange_running_elsewhere(fl, stream)) {
    xp.on = false;
    return XHIST_OK;
  }
  const ExchArgs& xa = xp.xa;
  if (int zrc = zero_output(xa.ctl, (int64_t)((xp.ctl_bytes + xp.words_bytes + xp.side_bytes + xp.rings_bytes) / 8), stream)) return zrc;
  // (the probe always runs: a histogram that fits the window has nothing outside it, but its owners' loads must be even too)
  XH_LAUNCH_PICKED(xp.k_xprobe, dim3(256), dim3(256), 0, stream, xa);
  HIPC(hipGetLastError());
  XH_LAUNCH_PICKED(xhist_pick_exchange_pick(), dim3(1), dim3(64), 0, stream, xa);
  HIPC(hipGetLastError());
  XH_LAUNCH_PICKED(xp.k_xch, dim3(kExchXcds * kExchRings), dim3(kExchBlock), xp.lds, stream, xa);
  HIPC(hipGetLastError());
  if (!fl.ev && hipEventCreateWithFlags(&fl.ev, hipEventDisableTiming) != hipSuccess) { fl.ev = nullptr; (void)hipGetLastError(); }
  if (fl.ev && hipEventRecord(fl.ev, stream) == hipSuccess) { fl.stream = stream; fl.armed = true; }
  else { fl.armed = false; (void)hipGetLastError(); }
  return XHIST_OK;
}

// Zero the counters, the exchange kernels when the mode is on, then the routing and adding-up passes (packed, then exact, when
// packing) and the exchange mode's merge.  `ra`: the first counter set (alloc_fused); kp's part fields describe the pass.
static int launch_fused(xhist_plan* p, hipStream_t stream, const Params& kp, const RoutePlan& rp, RouteArgs ra, ExchPlan& xp) {
  uint32_t* const ctr = ra.pool;
  void* const out = kp.out;
  const int shift = kp.part_shift, n_parts = kp.n_parts, rows = (int)kp.n_rows, parts_per_row = kp.parts_per_row;
  if (int zrc = zero_output(ctr, rp.ctr_words * 2, stream)) return zrc;
  if (xp.on)
    if (int xrc = launch_exchange(p, stream, xp)) return xrc;
  if (xp.on) {
    std::lock_guard<std::mutex> lk(p->mu);
    p->exch.ran_last = true;
    ra.xgate = xp.xa.win + 1;  // the classic packed kernels below return at once when the mode took the call
  }
  RouteArgs ra48 = ra;
  if (rp.pack) {
    XH_LAUNCH_PICKED(rp.k_route48, dim3(rp.G), dim3(rp.block), rp.lds_route, stream, kp, ra);  // packed records, notes the signs
    HIPC(hipGetLastError());
    ra48.gate = ctr + 1;
    ra48.gate_mode = 1;  // one sign: add the packed records up
    // both signs: the exact pass below runs (its own counters: the second set), otherwise its kernels return at once
    ra.pool = ctr + 2 * rp.ctr_words;
    ra.pcount = ra.pool + 2;
    ra.flags = ra.pool + 1;
    ra.gate = ctr + 1;
    ra.gate_mode = 2;
    ra.hint = p->mixed_hint;
    ra.xgate = nullptr;  // (the exact passes redo the call whenever the sign word says so, exchange mode or not)
  }
  XH_LAUNCH_PICKED(rp.k_route, dim3(rp.G), dim3(rp.block), rp.lds_route, stream, kp, ra);
  HIPC(hipGetLastError());
  if (rp.pack) {
    XH_LAUNCH_PICKED(rp.k_acc48, dim3(rp.Gb), dim3(1024), rp.lds_acc, stream, ra48, out, p->n_bins, shift, n_parts, rows > 1 ? parts_per_row : 0);
    HIPC(hipGetLastError());
  }
  XH_LAUNCH_PICKED(rp.k_acc, dim3(rp.Gb), dim3(1024), rp.lds_acc, stream, ra, out, p->n_bins, shift, n_parts, rows > 1 ? parts_per_row : 0);
  HIPC(hipGetLastError());
  if (xp.on) {  // (runs when the mode was on and the weights had one sign: exactly when none of the four kernels above did)
    XH_LAUNCH_PICKED(xhist_pick_exchange_merge(), dim3((unsigned)((p->n_bins + 255) / 256)), dim3(256), 0, stream, xp.xa, static_cast<double*>(out), p->n_bins);
    HIPC(hipGetLastError());
  }
  return XHIST_OK;
}

// Partitioned mode in one routing pass (xhist_route.hip.h): zero the chunk counters -> part_route ->
// part_accumulate_chunks, all on `stream`.  Returns XHIST_ERR_UNSUPPORTED (nothing launched) for what only
// the multi-pass form takes: more than 128 partitions, tables that do not fit LDS next to the sort buffers,
// in-bucket scans of 3 or 4 edges, integer samples.
//
// Packed records (float64 weights).  A record is normally a 16-bit bin code plus the float64 weight: 10 bytes in two streams.
// Rounding the weight to 36 mantissa bits makes room for the code in its low 16 bits: ONE 8-byte record, 40 instead of 44
// bytes of traffic per C5 sample.  The rounding is 2^-37 = 7.3e-12 relative per weight, so a bin's sum is off by at most
// 7.3e-12 x sum|w| — five orders inside the 1e-6 contract as long as sum|w| is comparable to |sum w|, i.e. as long as the
// weights of a bin do not cancel.  That is guaranteed when all weights have one sign, which the routing pass learns for free
// while it reads them.  So: route with packed records and note the signs seen (on the GPU); the packed adding-up pass runs only
// if one sign was seen; if both were, an exact routing + adding-up pass — queued behind, and returning at once otherwise —
// redoes the work with full float64 records.  Every decision is taken on the GPU (no host synchronisation: the call stays
// asynchronous); the plan remembers mixed signs through a pinned host word the exact pass sets, and later calls skip the
// packed attempt.  "records48" = -1 or XHIST_AMD_EXACT_RECORDS=1 turn packing off.
//
// `rows` > 1: that many rows (uniform row strides) in ONE pass — the routing pass treats (row, partition) as the partition, so
// a few time steps of a big joint histogram cost one launch pair instead of one per row; rows * parts_per_row <= 128.
static int execute_partitioned_fused(xhist_plan* p, const PlanKnobs& kn, const PartCall& pc, const xhist_array* samples,
                                     const xhist_array* weights, void* out, hipStream_t stream, bool first, bool last, int rows = 1) {
  const bool weighted = weights != nullptr;
  const int64_t n_cols = pc.n_cols;
  const int sdt = pc.sdt, wdt = pc.wdt, scan = pc.route.scan, shift = pc.shift, parts_per_row = pc.parts_per_row;
  const RouteGeom geom = pc.route.geom;
  const int n_parts = parts_per_row * rows;
  if (n_cols * rows >= ((int64_t)1 << 40) || n_cols < 4 || n_parts > 128) return XHIST_ERR_UNSUPPORTED;
  kernel_fn_route k_route = route_kernel(sdt, wdt, p->n_dims, scan, rows > 1, geom.block, geom.spl);
  if (!k_route) return XHIST_ERR_UNSUPPORTED;
  ensure_mixed_hint(p);
  const int exch_skip = exchange_bookkeeping(p);
  RoutePlan rp;
  if (int rc = plan_route(p, kn, k_route, sdt, wdt, weighted, scan, *pc.route.tset, shift, n_parts, rows, n_cols, geom, rp)) return rc;
  ExchPlan xp = plan_exchange(p, kn, samples, weights, n_cols, rows, sdt, wdt, rp.pack, exch_skip);
  if (xp.on) {  // a first look, before the mode's scratch is allocated (launch_exchange looks again, and decides)
    ExchInFlight& fl = exch_in_flight(p->device);
    std::lock_guard<std::mutex> lk(fl.mu);
    if (exchange_running_elsewhere(fl, stream)) xp.on = false;
  }

  ScratchScope scratch(stream);
  RouteArgs ra;
  if (int rc = alloc_fused(scratch, p, rp, n_parts, weighted, wdt == XHIST_F32, xp, ra)) return rc;
  if (first)
    if (int rrc = pc.rec->begin(kn.profile)) return rrc;
  Params kp = partitioned_params(p, pc, samples, weights, out, *pc.route.tset, rp.table_words, rows, n_parts);
  kp.parts_per_row = parts_per_row;
  kp.segs = rp.G;
  if (int rc = launch_fused(p, stream, kp, rp, ra, xp)) return rc;
  if (!last) return XHIST_OK;
  const ExchArgs& xa = xp.xa;
  const uint32_t* note = p->mixed_hint;  // (what the GPU has reported so far: the calls before this one)
  char desc[768];
  snprintf(desc, sizeof desc,
           "family=fast hist=partitioned route=fused rows_per_pass=%d parts=%d bins_per_part=%d group=%d chunk=%d chunks<=%lld tile=%d block=%d grid=%d "
           "acc_grid=%d lds_route=%zu lds_acc=%zu scan=%d weighted=%d D=%d cmp=%s records=%s exchange=%s exchange_window_ppm_before=%u exchange_aborts=%u exchange_busiest_owner_ppm_before=%u exchange_arrival_misses=%u exchange_records=%s",
           rows, n_parts, 1 << shift, kRouteGrp, 1 << rp.lg, (long long)rp.pool_chunks, rp.tile, rp.block, rp.G, rp.Gb, rp.lds_route, rp.lds_acc, scan,
           (int)weighted, p->n_dims, pc.route.f32 ? "f32thr" : "f64",
           !weighted ? "u16" : rp.pack ? "packed48(+exact if both signs)" : wdt == XHIST_F32 ? "u16+f32" : "u16+f64",
           !xp.on ? "no" : xa.force ? "forced" : xa.n_units > xa.rows_per ? "if the probe's window holds enough of the samples" : "whole histogram in the window",
           note ? note[3] : 0u, note ? note[2] : 0u, note ? note[4] : 0u, note ? note[5] : 0u,
           !xp.on ? "-" : xp.exact ? "exact12(two_rings)" : "packed8");
  return pc.rec->end(desc);
}

// One execute's arrays and shape, as the steps below see them.
struct Inputs {
  const xhist_array* samples;
  const xhist_array* weights;   // nullptr: counts
  const xhist_array* weights2;  // a second weight array binned in the same pass, or nullptr
  int64_t n_rows, n_cols;
  int D, sdt, wdt;  // wdt: -1 without weights
  bool weighted, two, float_samples;
  int n_arrays() const { return ::n_arrays(D, weights); }
  const xhist_array& array(int d) const { return array_at(samples, weights, D, d); }
};

// ---- row-per-lane mode: execute_lanes and its steps (xhist_lanes.hip.h) -------------------------------------------------
// Takes (a) views whose ROWS are the contiguous direction (row stride 1: reductions over leading axes) as they are, and (b) many
// short contiguous rows: streamed flat (hist_flat_rows), or turned around in one pass (hist_lanes_rows1), or transposed into a
// [cols, rows] scratch first (hist_lanes).  Returns XHIST_ERR_UNSUPPORTED, before anything is recorded or launched, when the
// shape is better served by the row-streaming kernels.
enum LaneFamily { kLaneFlatRows, kLaneRows1, kLaneColumns };

// What execute_lanes launches, decided by choose_lanes.
struct LaneChoice {
  int family = kLaneColumns;
  bool transpose = false;  // row-major arrays: flat rows, rows1, or hist_lanes on transposed scratch
  bool use_f32 = false;
  int scan = 0;
  const TableSet* tset = nullptr;
  size_t table_bytes = 0;
  int64_t row_blocks = 0;
  size_t lds = 0;  // dynamic LDS of the launch
  int direct = 0;
  kernel_fn_flat ff = nullptr;  // flat rows: R rows per workgroup
  int64_t R = 0;
  kernel_fn_rows1 f1 = nullptr;
  kernel_fn_lanes fn = nullptr;  // hist_lanes: lane_rows rows per workgroup, col_segs segments of cols_per_seg columns
  int lane_rows = 0, lane_pitch = 0;
  bool packed16 = false;
  int64_t col_segs = 0, cols_per_seg = 0;
};

// hist_flat_rows' LDS per row of a workgroup: uint16 counters (an even number) or float64 sums.
// (copies of a row's counters for the lanes of a wavefront to spread over — they read neighbouring samples, one or two
// rows at a time — were measured and bought nothing: 10^6 rows of 365 float32, 1 / 2 / 4 / 8 copies 0.403 / 0.411 / 0.422 /
// 0.497 ms; rows of 200: 0.463 / 0.468 / 0.520 / 0.684; the kernel keeps the parameter, at one copy here)
static constexpr int kFlatCopiesLog2 = 0;
static size_t flat_row_bytes(int64_t n_bins, bool weighted) {
  const uint32_t nbp = weighted ? (uint32_t)n_bins : (((uint32_t)n_bins + 1u) & ~1u);
  return ((size_t)nbp << kFlatCopiesLog2) * (weighted ? 8 : 2);
}

// hist_lanes with the lane groups of a row sharing one counter column per row: `rows` rows, uint16 or 4- / 8-byte counters
static size_t lanes_shared_lds(size_t table_bytes, int64_t n_bins, int rows, bool u16, bool weighted) {
  return table_bytes + (size_t)n_bins * (u16 ? (size_t)(rows / 2 + 1) * 4 : (size_t)(rows + 1) * (weighted ? 8 : 4));
}

// The digitize of the row-per-lane kernels: the plan's pick, with the overrides of small dtypes and of crowded buckets.
static void lane_tables(const xhist_plan* p, const PlanKnobs& kn, int sdt, bool small, LaneChoice& lc) {
  lc.use_f32 = sdt == XHIST_F32 && p->ts[1][0].blob != nullptr;
  lc.tset = &pick_tables(p, lc.use_f32, &lc.scan);
  if (small && lc.scan > 1) {  // their kernels exist for the one-compare scan and the binary search only
    lc.tset = &p->ts[0][0];
    lc.scan = 0;
  }
  // crowded buckets (geometric edges: a binary search in the two-level tables): the packed entries, general variant — the
  // row-per-lane and flat-rows kernels digitize sample by sample and feel every table read ((1825, 360, 720) float32 over
  // time, 50 geometric bins: 0.97 -> see profiles/r04_j_*)
  const int pk_np = small ? 0 : (sdt == XHIST_F64 ? p->pk_np : (lc.use_f32 ? p->pk32_np : 0));
  // (only against the binary search: with 3-4 edges per bucket the two-level tables are AHEAD in these LDS-hungry kernels —
  //  400 random edges, float32: row-per-lane 0.62 against 0.89 ms, flat rows 0.95 against 1.60)
  if (pk_np && kn.pack_pref >= 0 && (lc.scan == 0 || kn.pack_pref > 0)) {
    lc.tset = sdt == XHIST_F64 ? &p->ts_pk : &p->ts_pk32;
    lc.scan = kScanPackG;
  }
  lc.table_bytes = (size_t)lc.tset->words * 8;
}

// hist_flat_rows: R rows per workgroup.  False when there is no such variant or its LDS does not fit.
static bool plan_flat_rows(const xhist_plan* p, const Inputs& in, int accumulate, LaneChoice& lc) {
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const size_t row_bytes = flat_row_bytes(p->n_bins, in.weighted);
  kernel_fn_flat ff = xhist_pick_flat_rows(in.sdt, in.wdt, in.D, lc.scan);
  // R rows per workgroup: ~16 Ki samples, at most 24 KiB of counters, and enough workgroups for every CU
  int64_t R = std::min<int64_t>(16384 / n_cols, (int64_t)(24576 / row_bytes));
  R = std::min<int64_t>(R, std::max<int64_t>((2048 + n_cols - 1) / n_cols, n_rows / ((int64_t)p->cus * 8)));  // (2048+ samples a workgroup)
  R = std::max<int64_t>(1, std::min<int64_t>(R, 1024));
  const size_t lds = ((lc.table_bytes + 15) & ~(size_t)15) + (size_t)R * row_bytes + 32 * (in.weighted ? 8 : 4);
  const int64_t row_blocks = (n_rows + R - 1) / R;
  if (!ff || lds > p->lds_max || row_blocks > 2147483647LL) return false;
  lc.family = kLaneFlatRows;
  lc.ff = ff;
  lc.R = R;
  lc.lds = lds;
  lc.row_blocks = row_blocks;
  lc.direct = accumulate ? 0 : 1;
  return true;
}

// hist_lanes_rows1, the fused load-transpose-count kernel.  False when there is no such variant or its LDS does not fit.
static bool plan_rows1(const xhist_plan* p, const Inputs& in, int accumulate, LaneChoice& lc) {
  const int es = dtype_size(in.sdt);
  const size_t hist_bytes = (size_t)p->n_bins * (kLaneBlock / 2 + 1) * 4;
  const size_t lds = ((lc.table_bytes + hist_bytes + 15) & ~(size_t)15) + (size_t)kLaneBlock * (128 / es + 1) * es;
  kernel_fn_rows1 f1 = rows1_kernel(in.sdt, lc.scan);
  if (!f1 || lds > p->lds_max) return false;
  lc.family = kLaneRows1;
  lc.f1 = f1;
  lc.lds = lds;
  lc.row_blocks = (in.n_rows + kLaneBlock - 1) / kLaneBlock;
  lc.direct = accumulate ? 0 : 1;
  return true;
}

// hist_lanes: rows per workgroup, counter layout and column segments.
static int plan_lane_columns(const xhist_plan* p, const Inputs& in, int accumulate, LaneChoice& lc) {
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const bool weighted = in.weighted;
  const size_t table_bytes = lc.table_bytes;
  const size_t lds_lane = table_bytes + (size_t)p->n_bins * kLanePitch * (weighted ? 8 : 4);
  const size_t lds_lane16 = table_bytes + (size_t)p->n_bins * (kLaneBlock / 2 + 1) * 4;
  int lane_rows = kLaneBlock;  // the smallest power of two that holds the rows when there are fewer than 256
  while (lane_rows > 1 && lane_rows / 2 >= n_rows) lane_rows /= 2;
  // more rows than that, long reductions: 64-row workgroups with four column streams keep 4x the loads in
  // flight per row (10^5 x 1000 f32 over the leading axis: 0.25 -> 0.14 ms); short reductions pay for the
  // smaller blocks' zeroing and write-out instead (10^6 rows of 100: 0.17 -> 0.19 ms) and keep 256
  if (n_rows > 128 && n_cols >= 512) lane_rows = 64;
  // Counter columns per lane need n_bins x 257 words.  Where that does not fit (joint histograms over a leading axis:
  // 20 x 20 bins, (1825, 360, 720) float32 pairs over `time`: the generic family took 7.8 ms, now 1.0) or leaves one
  // workgroup per CU (float64 sums of 50 bins: 103 KB; the same array with weights 1.49 -> 0.78 ms), the lane groups of a
  // row share one column per row and the workgroup shrinks to as many rows as fit 40 KiB, 16 at least (joint counts: 64
  // rows / 54 KB 1.36 ms, 32 rows / 28 KB 1.02, 16 rows 1.80; weighted 50 bins: 128 rows / 53 KB 0.96-1.05, 64 rows 0.78-1.09).
  const bool u16_ok = !weighted && n_cols <= 65535;  // (one workgroup per row block then sees every column: see cols_per_seg below)
  constexpr size_t share_above = 64 * 1024, share_target = 40 * 1024;
  bool shared = false;
  if ((u16_ok ? lds_lane16 : lds_lane) > std::min(p->lds_max, share_above)) {
    lane_rows = std::min(lane_rows, 128);
    while (lane_rows > 16 && lanes_shared_lds(table_bytes, p->n_bins, lane_rows, u16_ok, weighted) > share_target) lane_rows /= 2;
    if (lanes_shared_lds(table_bytes, p->n_bins, lane_rows, u16_ok, weighted) > p->lds_max) return XHIST_ERR_UNSUPPORTED;
    shared = true;
  }
  // (counts: uint16 counter columns, two per word — the only unweighted form: a column segment longer than 65535 samples
  //  would need 2^24 rows to be asked for, see the check on cols_per_seg below; sums: float64 columns)
  const bool packed16 = !weighted;
  const size_t lds = shared ? lanes_shared_lds(table_bytes, p->n_bins, lane_rows, packed16, weighted) : (packed16 ? lds_lane16 : lds_lane);
  if (lds > p->lds_max) return XHIST_ERR_UNSUPPORTED;
  const int64_t row_blocks = (n_rows + lane_rows - 1) / lane_rows;
  const int bpc = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)160 * 1024 / lds));
  int64_t col_segs = std::max<int64_t>(1, ((int64_t)p->cus * bpc * 2 + row_blocks - 1) / row_blocks);
  col_segs = std::min<int64_t>(col_segs, std::max<int64_t>(1, n_cols / 64));
  col_segs = std::min<int64_t>(col_segs, 65535);
  const int64_t cols_per_seg = (n_cols + col_segs - 1) / col_segs;
  // (uint16 counters and a segment of more than 65535 columns: only with so many row blocks that there is one segment each —
  //  beyond 10^10 samples; the row-streaming kernels take that call.  The uint32-column kernels this used to fall back to were
  //  never selected by anything — census of round 6 — and are gone)
  if (packed16 && cols_per_seg > 65535) return XHIST_ERR_UNSUPPORTED;
  if (row_blocks > 2147483647LL) return XHIST_ERR_UNSUPPORTED;
  lc.family = kLaneColumns;
  lc.lane_rows = lane_rows;
  lc.lane_pitch = !shared ? 0 : packed16 ? lane_rows / 2 + 1 : lane_rows + 1;
  lc.packed16 = packed16;
  lc.lds = lds;
  lc.row_blocks = row_blocks;
  lc.col_segs = (n_cols + cols_per_seg - 1) / cols_per_seg;
  lc.cols_per_seg = cols_per_seg;
  lc.direct = (lc.col_segs == 1 && !accumulate) ? 1 : 0;
  return XHIST_OK;
}

// Every decision of execute_lanes, and every XHIST_ERR_UNSUPPORTED it returns: nothing is recorded, allocated or launched here.
static int choose_lanes(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, int accumulate, LaneChoice& lc) {
  const int D = in.D, sdt = in.sdt, wdt = in.wdt;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const bool prefer = kn.lanes > 0;
  const bool weighted = in.weighted;
  if (p->cmp != XHIST_CMP_F64 || D > 3 || n_cols >= ((int64_t)1 << 31) || p->n_bins >= (1 << 16) || p->huge) return XHIST_ERR_UNSUPPORTED;
  // integer / half-precision samples: one input, unweighted or float64 weights, and only as views whose rows
  // are the contiguous direction (10^6 x 100 int32 over the leading axis: generic family 1.70 ms)
  const bool small = sdt == XHIST_I32 || sdt == XHIST_I64 || sdt == XHIST_I16 || sdt == XHIST_U8 || sdt == XHIST_F16;
  if (small ? !(D == 1 && (wdt == -1 || wdt == XHIST_F64))
            : ((sdt != XHIST_F64 && sdt != XHIST_F32) || (wdt != -1 && wdt != XHIST_F64 && wdt != XHIST_F32)))
    return XHIST_ERR_UNSUPPORTED;
  // shape class of every array: natural (row stride 0/1, any column stride) or needs a transpose
  // (unit column stride, dense-ish rows)
  // (and dense rows of aligned vectors: what the flat-rows kernel streams)
  bool all_natural = true, all_rowmajor = true, grouped_any = false, all_dense = true;
  for (int d = 0; d < in.n_arrays(); ++d) {
    const xhist_array& a = in.array(d);
    if (d < D && a.dtype != sdt) return XHIST_ERR_UNSUPPORTED;
    const bool bcast = a.row_stride == 0 || a.col_stride == 0;
    const bool natural = bcast || (a.row_stride == 1 && (a.inner_rows ? a.col_stride >= 1 : a.col_stride >= n_rows));
    const bool rowmajor = bcast || (a.col_stride == 1 && a.row_stride >= n_cols);
    const size_t vec_bytes = (size_t)(16 / dtype_size(sdt)) * (size_t)dtype_size(a.dtype);  // one load: as many elements as a 16-byte sample vector
    grouped_any |= a.inner_rows != 0 && !bcast;
    all_natural &= natural;
    all_rowmajor &= rowmajor;
    all_dense &= a.col_stride == 1 && a.row_stride == n_cols && a.inner_rows == 0 && ((uintptr_t)a.data & (vec_bytes - 1)) == 0;
  }
  const bool rows_natural = all_natural && in.samples[0].row_stride == 1;
  if (small && !rows_natural) return XHIST_ERR_UNSUPPORTED;
  lane_tables(p, kn, sdt, small, lc);
  // dense short rows of one or two float inputs, with or without float weights: streamed flat (hist_flat_rows)
  // (3.65 x 10^8 float32 samples, 50 bins, ms per call, fused turn-around kernel / row streaming | flat: rows of 20 2.25 | 1.83;
  // 64 1.00 | 0.72; 100 1.07 | 0.66; 200 0.84 | 0.46; 365 0.79 | 0.41; 512 0.59 | 0.42; 720 0.46 | 0.43; 1024 0.33 | 0.38;
  // 2048 0.28 | 0.37: profiles/r03_f_flat_rows.txt)
  constexpr int64_t kFlatMaxCols = 800;
  const bool flat_ok = (D == 1 || D == 2) && !small && n_cols >= 1 && n_cols < 65536 && (sdt != XHIST_F32 || lc.use_f32) &&
                       flat_row_bytes(p->n_bins, weighted) <= 4096 && (!weighted || wdt == XHIST_F32 || wdt == XHIST_F64) && all_dense;
  const bool use_flat = flat_ok && !prefer && kn.flat_rows >= 0 && n_rows >= 4096 && n_cols <= (kn.flat_rows > 0 ? 65535 : kFlatMaxCols) &&
                        !rows_natural;
  // many short rows.  Measured crossovers with the row-streaming kernels (64-thread workgroups, few LDS copies, plain-store
  // flush; 3.65 x 10^8 f32 samples): ~400 columns for the fused kernel (one unweighted input: 384 columns 0.64 against
  // 0.67 ms, 512 columns 0.62 against 0.50), below ~90 for scratch-transpose + lanes (weighted, 96 columns: 3.6 against 3.3 ms)
  const bool short_rows = all_rowmajor && n_cols <= ((D == 1 && !weighted) ? 400 : 80);
  if (all_natural && (in.samples[0].row_stride == 1 || prefer)) {
    // rows are the contiguous direction: the row-streaming kernels cannot coalesce this at all
  } else if (use_flat || (all_rowmajor && prefer) || (n_rows >= 4096 && short_rows)) {
    lc.transpose = true;
  } else {
    return XHIST_ERR_UNSUPPORTED;
  }
  int vec = 1;
  lc.fn = (kernel_fn_lanes)fast_kernel(sdt, wdt, D, lc.scan, weighted ? kHistLanes : kHistLanes16, &vec);
  if (!lc.fn) return XHIST_ERR_UNSUPPORTED;
  if (use_flat && plan_flat_rows(p, in, accumulate, lc)) return XHIST_OK;
  // the flat kernel was the only reason to be here and was not launched (no such variant, or its LDS does not fit): beyond
  // the column limits of the scratch-transpose route the row-streaming kernels are the faster answer
  if (use_flat && !short_rows) return XHIST_ERR_UNSUPPORTED;
  // (hist_lanes: a counter column per lane, or — shared by a row's lane groups — per row, for as few as 16 rows per workgroup)
  const size_t lds_least = lc.table_bytes + (size_t)p->n_bins * (weighted ? 17 * 8 : 9 * 4);
  if (lds_least > p->lds_max) return XHIST_ERR_UNSUPPORTED;
  // one contiguous-row input, unweighted, < 65536 columns: the fused load-transpose-count kernel, which takes grouped rows too
  const bool rows1_ok = D == 1 && !weighted && n_cols < 65536 && in.samples[0].col_stride == 1 && in.samples[0].row_stride != 0;
  if (lc.transpose && rows1_ok && plan_rows1(p, in, accumulate, lc))
    return lc.row_blocks > 2147483647LL ? XHIST_ERR_UNSUPPORTED : XHIST_OK;
  if (lc.transpose && grouped_any) return XHIST_ERR_UNSUPPORTED;  // transpose_2d takes plain row strides only
  return plan_lane_columns(p, in, accumulate, lc);
}

static int launch_flat_rows(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const LaneChoice& lc, void* out, hipStream_t stream) {
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  // (flat rows: unit column stride and no groups, choose_lanes; what the kernel is handed of the groups stays zero)
  Params kp = fill_params(in.samples, in.weights, in.D, *lc.tset, lc.tset->words, n_rows, n_cols, p->n_bins, out);
  for (int d = 0; d < in.D; ++d) kp.s_os[d] = 0;
  kp.w_os = 0;
  const uint64_t magic = (((uint64_t)1 << 40) / (uint64_t)n_cols) + 1u;
  LaunchRecord rec(p, stream);
  if (int rrc = rec.begin(kn.profile)) return rrc;
  HIPC(set_dynamic_lds((const void*)lc.ff, lc.lds));
  XH_LAUNCH_PICKED(lc.ff, dim3((unsigned)lc.row_blocks), dim3(kLaneBlock), lc.lds, stream, kp, (int32_t)lc.direct, (int32_t)lc.R,
                   (int32_t)kFlatCopiesLog2, magic, (int64_t)(n_rows * n_cols));
  HIPC(hipGetLastError());
  char desc[320];
  snprintf(desc, sizeof desc,
           "family=flat_rows hist=%s rows_per_wg=%lld copies=%d direct_store=%d block=%d grid=%lld lds_bytes=%zu scan=%d weighted=%d D=%d cmp=%s",
           in.weighted ? "lds" : "lds16", (long long)lc.R, 1 << kFlatCopiesLog2, lc.direct, kLaneBlock, (long long)lc.row_blocks, lc.lds, lc.scan,
           (int)in.weighted, in.D, lc.use_f32 ? "f32thr" : "f64");
  return rec.end(desc);
}

static int launch_rows1(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const LaneChoice& lc, void* out, hipStream_t stream) {
  // (one unweighted input of unit column stride, choose_lanes)
  const Params kp = fill_params(in.samples, nullptr, 1, *lc.tset, lc.tset->words, in.n_rows, in.n_cols, p->n_bins, out);
  LaunchRecord rec(p, stream);
  if (int rrc = rec.begin(kn.profile)) return rrc;
  HIPC(set_dynamic_lds((const void*)lc.f1, lc.lds));
  XH_LAUNCH_PICKED(lc.f1, dim3((unsigned)lc.row_blocks), dim3(kLaneBlock), lc.lds, stream, kp, (int32_t)lc.direct);
  HIPC(hipGetLastError());
  char desc[384];
  snprintf(desc, sizeof desc,
           "family=lanes hist=lds16 transpose=fused direct_store=%d block=%d grid=%lld lds_bytes=%zu scan=%d weighted=0 D=1 cmp=%s",
           lc.direct, kLaneBlock, (long long)lc.row_blocks, lc.lds, lc.scan, lc.use_f32 ? "f32thr" : "f64");
  return rec.end(desc);
}

// hist_lanes, on the arrays as they are or on [cols, rows] scratch copies of the row-major ones (broadcast arrays stay as they are).
static int launch_lane_columns(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const LaneChoice& lc, void* out, int accumulate,
                               hipStream_t stream) {
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  ScratchScope scratch(stream);
  LaunchRecord rec(p, stream);
  if (int rrc = rec.begin(kn.profile)) return rrc;
  xhist_array views[kMaxDims + 1];  // the samples, then the weights
  for (int d = 0; d < in.n_arrays(); ++d) {
    const xhist_array& a = in.array(d);
    views[d] = a;
    if (!lc.transpose || a.row_stride == 0 || a.col_stride == 0) continue;
    const int es = dtype_size(a.dtype);
    void* dense = nullptr;
    HIPC(scratch.alloc(&dense, (size_t)n_rows * n_cols * es));
    const dim3 grid((unsigned)((n_rows + 63) / 64), (unsigned)((n_cols + 63) / 64));
    if (es == 8)
      XH_LAUNCH_PICKED(transpose_2d<double>, grid, dim3(256), 0, stream, (const double*)a.data, a.row_stride, n_rows, n_cols, (double*)dense);
    else
      XH_LAUNCH_PICKED(transpose_2d<float>, grid, dim3(256), 0, stream, (const float*)a.data, a.row_stride, n_rows, n_cols, (float*)dense);
    HIPC(hipGetLastError());
    views[d].data = dense;
    views[d].row_stride = 1;
    views[d].col_stride = n_rows;
    views[d].inner_rows = 0;
    views[d].outer_stride = 0;
  }
  Params kp = fill_params(views, in.weighted ? &views[in.D] : nullptr, in.D, *lc.tset, lc.tset->words, n_rows, n_cols, p->n_bins, out);
  kp.lane_rows = lc.lane_rows;
  kp.lane_pitch = lc.lane_pitch;
  if (!lc.direct && !accumulate)
    if (int zrc = zero_output(out, n_rows * p->n_bins, stream)) return zrc;
  HIPC(set_dynamic_lds((const void*)lc.fn, lc.lds));
  XH_LAUNCH_PICKED(lc.fn, dim3((unsigned)lc.row_blocks, (unsigned)lc.col_segs), dim3(kLaneBlock), lc.lds, stream, kp, (int32_t)lc.direct,
                   lc.cols_per_seg);
  HIPC(hipGetLastError());
  char desc[384];
  snprintf(desc, sizeof desc,
           "family=lanes hist=%s%s rows_per_wg=%d transpose=%d direct_store=%d block=%d grid=%lldx%lld lds_bytes=%zu scan=%d weighted=%d D=%d cmp=%s",
           lc.packed16 ? "lds16" : "lds", lc.lane_pitch ? "(shared)" : "", lc.lane_rows, (int)lc.transpose, lc.direct, kLaneBlock,
           (long long)lc.row_blocks, (long long)lc.col_segs, lc.lds, lc.scan, (int)in.weighted, in.D, lc.use_f32 ? "f32thr" : "f64");
  return rec.end(desc);
}

static int execute_lanes(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, void* out, int accumulate, hipStream_t stream) {
  LaneChoice lc;
  if (int rc = choose_lanes(p, kn, in, accumulate, lc)) return rc;
  switch (lc.family) {
    case kLaneFlatRows: return launch_flat_rows(p, kn, in, lc, out, stream);
    case kLaneRows1: return launch_rows1(p, kn, in, lc, out, stream);
    default: return launch_lane_columns(p, kn, in, lc, out, accumulate, stream);
  }
}

// ------------------------------------------------------------------------------------------
// the streaming kernels: execute_device and its steps
// ------------------------------------------------------------------------------------------
static int execute_device(xhist_plan* p, const xhist_array* samples, const xhist_array* weights, int64_t n_rows, int64_t n_cols,
                          void* out, int accumulate, hipStream_t stream, const xhist_array* weights2 = nullptr, void* out2 = nullptr);

// ---- a few rows that are the contiguous direction, too many bins for the row-per-lane kernels ----------------
// (the columns of an (n, K) table histogrammed over its leading axis with thousands of bins): every other kernel
// would walk them with a column stride of K elements — the generic family at ~1 TB/s, memory-side atomics at 0.1
// beyond LDS.  Gather the rows into dense scratch first (one pass, read + write) and run the vector kernels on that:
// 25 x 10^6 x 4 float32, 5000 bins 0.44 -> see profiles/r02_j_table_columns*.jsonl.
// Returns XHIST_ERR_UNSUPPORTED (nothing touched) for every other shape.
static int execute_table_columns(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, void* out, int accumulate, hipStream_t stream) {
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  if (kn.force_generic || in.two || n_rows < 1 || n_rows > 64 || n_cols < 4096) return XHIST_ERR_UNSUPPORTED;
  bool table = true;
  for (int d = 0; d < in.n_arrays() && table; ++d) {
    const xhist_array& a = in.array(d);
    table = a.inner_rows == 0 && a.row_stride == 1 && a.col_stride >= n_rows && a.col_stride > 1 &&
            ((uintptr_t)a.data % (size_t)dtype_size(a.dtype)) == 0;
  }
  // (up to four 8-byte columns with a histogram that fits LDS: the strided walk of the generic family is as fast — 25 x 10^6 x 4
  //  float64 + weights, 5000 bins: 0.50 ms against 0.87 with the gather; every other measured shape gains 1.3-9 x)
  if (table && n_rows <= 4 && dtype_size(in.samples[0].dtype) == 8 && p->n_bins * (in.weighted ? 8 : 4) <= (int64_t)96 * 1024) table = false;
  if (!table) return XHIST_ERR_UNSUPPORTED;
  ScratchScope scratch(stream);
  xhist_array dense[kMaxDims + 1];  // the samples, then the weights
  for (int d = 0; d < in.n_arrays(); ++d) {
    const xhist_array& a = in.array(d);
    const int es = dtype_size(a.dtype);
    void* buf = nullptr;
    if (scratch.alloc(&buf, (size_t)n_rows * n_cols * es) != hipSuccess) {
      (void)hipGetLastError();
      return fail(XHIST_ERR_NOMEM, "allocation of %lld bytes of gather scratch failed", (long long)n_rows * n_cols * es);
    }
    const int grid = (int)std::min<int64_t>((n_cols + 255) / 256, (int64_t)p->cus * 16);
    // whole tables with rows of whole 16-byte units: tiled through LDS (256 rows x (k + 1) elements)
    const size_t tile_lds = (size_t)256 * (n_rows + 1) * es;
    if (a.col_stride == n_rows && ((int64_t)n_rows * es) % 16 == 0 && ((uintptr_t)a.data % 16) == 0 && es >= 4 && tile_lds <= 64 * 1024) {
      const int tgrid = (int)std::min<int64_t>((n_cols + 255) / 256, (int64_t)p->cus * (int64_t)std::max<size_t>(1, (160 * 1024) / tile_lds));
      if (es == 8) XH_LAUNCH_PICKED(gather_rows_tiled<uint64_t>, dim3(tgrid), dim3(256), tile_lds, stream, (const uint64_t*)a.data, (int)n_rows, n_cols, (uint64_t*)buf);
      else XH_LAUNCH_PICKED(gather_rows_tiled<uint32_t>, dim3(tgrid), dim3(256), tile_lds, stream, (const uint32_t*)a.data, (int)n_rows, n_cols, (uint32_t*)buf);
    } else
    switch (es) {
      case 8: XH_LAUNCH_PICKED(gather_rows<uint64_t>, dim3(grid), dim3(256), 0, stream, (const uint64_t*)a.data, a.col_stride, (int)n_rows, n_cols, (uint64_t*)buf); break;
      case 4: XH_LAUNCH_PICKED(gather_rows<uint32_t>, dim3(grid), dim3(256), 0, stream, (const uint32_t*)a.data, a.col_stride, (int)n_rows, n_cols, (uint32_t*)buf); break;
      case 2: XH_LAUNCH_PICKED(gather_rows<uint16_t>, dim3(grid), dim3(256), 0, stream, (const uint16_t*)a.data, a.col_stride, (int)n_rows, n_cols, (uint16_t*)buf); break;
      default: XH_LAUNCH_PICKED(gather_rows<uint8_t>, dim3(grid), dim3(256), 0, stream, (const uint8_t*)a.data, a.col_stride, (int)n_rows, n_cols, (uint8_t*)buf); break;
    }
    if (hipGetLastError() != hipSuccess) return fail(XHIST_ERR_HIP, "gather_rows launch failed");
    dense[d] = a;
    dense[d].data = buf;
    dense[d].row_stride = n_cols;
    dense[d].col_stride = 1;
  }
  return execute_device(p, dense, in.weighted ? &dense[in.D] : nullptr, n_rows, n_cols, out, accumulate, stream);
}

// Where the histogram lives for a table footprint of `tbytes`:
//   lds:    replicated sub-histograms in LDS (one copy per lane bank), uint32 / float64
//   packed: unweighted vector family only, uint16 counters packed two per word (exact, see kernel)
//   global: device-scope atomics straight into the output
// padded_bins: hist_fast's PADDED layout (the float32 arithmetic digitize of one input).
struct Placement {
  int hist = kHistGlobal;
  int cl2 = 0;  // log2 of the LDS copies
  size_t hist_bytes = 0;
};
static Placement place_histogram(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, size_t tbytes, bool vector_family,
                                 bool padded_bins) {
  Placement pl;
  const size_t lds_cap = p->lds_max;
  if (kn.force_global || tbytes + 1024 > lds_cap || p->n_bins >= ((int64_t)1 << 24)) return pl;
  const bool weighted = in.weighted;
  const int acc_size = (weighted ? 8 : 4) * (in.two ? 2 : 1);  // two weights: two replicated histograms side by side
  const int max_cl2 = weighted ? 4 : 5;
  // replication is only worth LDS that small workgroups can share; unweighted 4-byte samples
  // issue twice the LDS atomics per byte streamed and gain 5 % from more copies (1-D, 500-2000 bins)
  const size_t soft = (!weighted && in.D == 1 && dtype_size(in.samples[0].dtype) <= 4 ? 64 : 24) * 1024;
  int cl2 = max_cl2;
  if (kn.lds_copies) { cl2 = 0; while ((1 << cl2) < kn.lds_copies) ++cl2; cl2 = std::min(cl2, max_cl2); }
  // + 32 trash slots; the padded layout of the float32 arithmetic digitize (one input): a bin in front and one behind instead
  // (2 x max(1, 32 >> c) bins of 2^c copies: 64 slots for every c <= 5)
  auto bytes_at = [&](int c) { return (((size_t)p->n_bins << c) + (padded_bins ? (size_t)std::max(64, 2 << c) : 32)) * (size_t)acc_size; };
  if (!kn.lds_copies) while (cl2 > 0 && bytes_at(cl2) > soft) --cl2;
  // short rows: a workgroup zeroes and reads back every copy, which must stay small next to the
  // samples it bins (10^5 rows x 1000 f32, 50 bins: 32 copies 0.162 ms, 4 copies 0.096 ms)
  if (!kn.lds_copies) {
    int64_t sb = 0;
    for (int d = 0; d < in.D; ++d) sb += dtype_size(in.samples[d].dtype);
    if (weighted) sb += dtype_size(in.weights->dtype);
    const double wgs = (double)std::max<int64_t>(in.n_rows, (int64_t)p->cus * 8);
    const double per_wg_bytes = (double)in.n_rows * (double)in.n_cols * (double)sb / wgs;
    while (cl2 > 0 && (double)bytes_at(cl2) > per_wg_bytes / 4) --cl2;
  }
  while (cl2 > 0 && tbytes + bytes_at(cl2) > lds_cap) --cl2;
  if (tbytes + bytes_at(cl2) <= lds_cap) {
    pl.hist = kHistLds;
    pl.cl2 = cl2;
    pl.hist_bytes = bytes_at(cl2);
  } else if (vector_family && in.float_samples && !weighted && tbytes + (((size_t)p->n_bins + 1) / 2 + 32) * 4 <= lds_cap) {
    pl.hist = kHistPacked;
    pl.hist_bytes = (((size_t)p->n_bins + 1) / 2 + 32) * 4;
  }
  return pl;
}

// What the streaming launch runs: the kernel, its family and digitize, and where the histogram lives.
struct StreamChoice {
  kernel_fn fn = nullptr;
  bool fast = false;   // the vector family (else the generic one)
  bool mixed = false;  // ... in its mixed-dtype variant
  bool use_f32 = false;  // float32-threshold tables
  bool tables_in_lds = false;
  bool long_tiles = false;
  int vec = 1, scan = 0;
  int hist = kHistGlobal, cl2 = 0;
  const TableSet* tset = nullptr;
  size_t table_bytes = 0, hist_bytes = 0, lds_bytes = 0;
  int n_slices = 1;  // bin slices (choose_slices): launches, and the bins of each
  int64_t slice_bins = 0;
};

// ---- family: fast (vector loads, homogeneous f64/f32) or generic --------------------------
// Two weights: XHIST_ERR_UNSUPPORTED before anything is touched when the vector family with an LDS histogram cannot take them.
static int choose_streaming(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, StreamChoice& sc) {
  const int D = in.D, sdt = in.sdt, wdt = in.wdt;
  const bool weighted = in.weighted, two = in.two, float_samples = in.float_samples;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const size_t lds_cap = p->lds_max;
  const bool small_samples = sdt == XHIST_I32 || sdt == XHIST_I64 || sdt == XHIST_I16 || sdt == XHIST_U8 || sdt == XHIST_F16;
  // the exact int64 domain has vector kernels for one int64 / datetime64 input
  const bool i64dom = p->cmp == XHIST_CMP_I64 && !p->uns && sdt == XHIST_I64 && D == 1 && (wdt == -1 || wdt == XHIST_F64);
  bool fast_ok = !kn.force_generic && (p->cmp == XHIST_CMP_F64 || i64dom) && p->n_bins < ((int64_t)1 << 31) &&
                 ((float_samples && D <= 3 && (wdt == -1 || wdt == XHIST_F64 || wdt == XHIST_F32)) ||
                  (small_samples && D == 1 && (wdt == -1 || wdt == XHIST_F64)));
  if (fast_ok) {
    // unit column stride is all the vector family needs: gfx950 vector loads take any
    // element-aligned address (rows of 365 or 3650 samples stay on 16-byte loads)
    for (int d = 0; d < D && fast_ok; ++d) {
      const xhist_array& a = in.samples[d];
      fast_ok = a.dtype == sdt && a.col_stride == 1 && ((uintptr_t)a.data % (size_t)dtype_size(sdt) == 0);
    }
    if (fast_ok && weighted) fast_ok = in.weights->col_stride == 1 && ((uintptr_t)in.weights->data % (size_t)dtype_size(wdt) == 0);
  }
  // Mixtures the homogeneous vector kernels do not take — float32 next to float64, integers in a joint histogram,
  // integer / bool / half weights — with unit column strides and the float64 compare domain: the MIXED variant of the
  // vector kernels (four elements per load in each array's own dtype, consumed as float64).  LDS histograms only;
  // beyond LDS the Python layer converts such inputs to float64 first (core._promote_for_big_histograms).
  bool mixed_ok = false;
  if (!fast_ok && !kn.force_generic && !two && p->cmp == XHIST_CMP_F64 && D <= 3 && p->n_bins < ((int64_t)1 << 24) && !p->huge) {
    // element-aligned, and for 1- / 2-byte elements every row dword-aligned (their four-element loads are one dword / two)
    auto vector_loadable = [&](const xhist_array& a) {
      const size_t es = (size_t)dtype_size(a.dtype), al = es < 4 ? 4 : es;
      if (!(a.col_stride == 1 || n_cols == 1) || (uintptr_t)a.data % al != 0) return false;
      if (es >= 4 || n_rows == 1) return true;
      return (a.row_stride * es) % 4 == 0 && (a.outer_stride * es) % 4 == 0;
    };
    mixed_ok = true;
    for (int d = 0; d < in.n_arrays() && mixed_ok; ++d) mixed_ok = vector_loadable(in.array(d));
    // measured (tools/mixtures.py, 2 x 10^8 samples, against the generic family): float32 + int32 weights 1.06 -> 0.30 ms,
    // int32 x int32 1.17 -> 0.40, uint8 x float32 1.15 -> 0.37, float32 x float64 0.91 -> 0.46
  }

  // Two attempts: the vector family with its tables, then (if it has no kernel for this
  // combination, or its tables do not fit LDS) the generic family with the native tables.
  // Every alternative digitize below asks place_histogram where the histogram would live with it, and takes it or leaves it.
  bool fast = false, mixed = false, use_f32 = false, tables_fit = false, tables_in_lds = false;
  int scan = 0, vec = 1;
  const TableSet* tset = nullptr;
  size_t table_bytes = 0;
  Placement pl;
  kernel_fn fn = nullptr;
  for (int attempt = (fast_ok || mixed_ok) ? 0 : 1; attempt < 2 && !fn; ++attempt) {
    fast = attempt == 0;
    mixed = fast && !fast_ok;
    // float32 samples are digitized against the float32-threshold tables (exact, see Dom<2>)
    use_f32 = fast && !mixed && sdt == XHIST_F32 && p->ts[1][0].blob != nullptr;  // (mixed dtypes are consumed as float64)
    scan = 0;
    tset = &p->ts[0][0];  // generic family: native domain, (start, cnt) tables
    if (fast) tset = &pick_tables(p, use_f32, &scan);
    if (mixed && scan >= 3) {  // the mixed variant has no 3- / 4-edge scans: binary search on the (start, cnt) tables
      scan = 0;
      tset = &p->ts[0][0];
    }
    table_bytes = (size_t)tset->words * 8;
    tables_fit = table_bytes + 1024 <= lds_cap && !(fast && p->huge);  // no bucket tables: not for the vector family
    if (tables_fit || !fast) pl = place_histogram(p, kn, in, table_bytes, fast, false);
    // Arithmetic edges (bins=int, np.linspace): when the edge tables are what keeps the histogram
    // out of LDS — or do not fit LDS at all — digitize without tables (count_le_arith): 30000
    // uniform bins stay on the streaming kernels instead of 43 ms/10^9 samples of global atomics.
    // Also when the tables fit but only with 3-4 edges per bucket (float32, 20000 bins: 1.17 against 1.39 ms);
    // with 1-2 edges per bucket the tables win (C2: 2.28 against 2.40 ms, float32 50 bins: 0.69 against 1.12).
    // (Round 3: the arithmetic digitize needs no edge any more unless the sample is next to one — bin_arith_fast, 4-19 % off
    // every table-free launch — and on one box it beat the one-edge-per-bucket tables for float64 samples too, 1.33 -> 1.22 ms
    // for the unweighted headline; on another the two were level (1.19 / 1.21), 10^6 samples went 8.8 -> 12.7 us and a 20^3
    // float64 histogram 1.97 -> 2.06 ms: the rule stays as it was.  profiles/r03_ar_arith_ab.txt)
    if (fast && (float_samples || mixed) && p->arith && kn.arith_pref >= 0 &&
        (!tables_fit || pl.hist == kHistGlobal || scan == 0 || scan >= 3 || kn.arith_pref > 0)) {
      const Placement alt = place_histogram(p, kn, in, 0, true, false);
      if (alt.hist != kHistGlobal || !tables_fit || kn.arith_pref > 0) {
        pl = alt;
        scan = kScanArith;
        use_f32 = false;
        tset = &p->ts[0][0];  // float64-domain DimTable (e_0, e_last, step); its tables are not read
        table_bytes = 0;
        tables_fit = true;
      }
    }
    // float32 samples on arithmetic edges with an LDS histogram: the bin from float32 arithmetic, no table at all
    // (bin_arith32_fast: 7-9 vector instructions and one LDS operation per sample against 12 and three for the threshold
    // tables — BASELINE C4, whose dask-chunk-sized calls run while the clock of a just-woken GPU dips)
    // ("arith" = 1 asks for the float64 arithmetic by name and keeps it; "arith" = -1 rules out both)
    if (fast && !mixed && !two && !i64dom && sdt == XHIST_F32 && p->arith32 && kn.arith32_pref >= 0 && kn.arith_pref >= 0 &&
        (kn.arith32_pref > 0 || (kn.arith_pref == 0 && (scan == 1 || scan == 2 || scan == kScanArith)))) {
      const Placement alt = place_histogram(p, kn, in, 0, true, /*padded_bins=*/D == 1);
      // (no second try without the padding: the kernel's PADDED layout is a compile-time property of <kScanArith32, D == 1, LDS>,
      //  so a one-input histogram that fits LDS only unpadded — n_bins within 64 of the cap — keeps the digitize it had)
      if (alt.hist == kHistLds) {
        pl = alt;
        scan = kScanArith32;
        use_f32 = false;
        tset = &p->ts[0][0];  // float64-domain DimTable (e_0, e_last, step, a32_*); its tables are not read
        table_bytes = 0;
        tables_fit = true;
      }
    }
    // Non-uniform edges, float64 samples: packed 16-byte bucket entries (count_le_pack) — one LDS read per sample and
    // dimension instead of two dependent ones — where the histogram stays in LDS with them.  Measured for joint histograms
    // (C3: see DESIGN 4); 1-D histograms keep the two-level tables unless "pack" = 1.
    const int pk_np = sdt == XHIST_F64 ? p->pk_np : (sdt == XHIST_F32 && use_f32 ? p->pk32_np : 0);
    if (fast && !mixed && !two && !i64dom && pk_np && kn.pack_pref >= 0 && scan != kScanArith && scan != kScanArith32 && tables_fit &&
        (scan == 0 || scan >= 2 || kn.pack_pref > 0) && (D >= 2 || scan == 0 || (sdt == XHIST_F32 && !weighted) || kn.pack_pref > 0)) {
      // (scan 0: the alternative is a binary search; 1-D: measured level for float64 samples and for weighted float32 ones,
      //  0.74 -> 0.85 of 8 TB/s for float32 counts — twice the table reads per byte streamed: profiles/r04_h_*)
      const TableSet& pk = sdt == XHIST_F64 ? p->ts_pk : p->ts_pk32;
      const size_t tb = (size_t)pk.words * 8;
      if (tb + 1024 <= lds_cap) {
        const Placement alt = place_histogram(p, kn, in, tb, true, false);
        if ((alt.hist == kHistLds || alt.hist == kHistPacked) && (alt.hist == pl.hist || kn.pack_pref > 0)) {
          pl = alt;
          scan = pk_np == 2 ? kScanPack2 : (pk_np == 3 ? kScanPack3 : kScanPackG);
          tset = &pk;
          table_bytes = tb;
        }
      }
    }
    if (fast && !tables_fit) continue;  // the vector family keeps its tables in LDS
    if (mixed && pl.hist != kHistLds) continue;  // (packed / memory-side histograms: the generic family)
    tables_in_lds = tables_fit;
    // (scan 1..4: linear in-bucket count, no bucket holds more than 4 edges — always for uniform bins)
    if (two) {  // one attempt only: the vector family, LDS histograms, table digitize with <= 2 edges per bucket
      const xhist_array* w2 = in.weights2;
      if (!fast || pl.hist != kHistLds || (scan != 1 && scan != 2) || !float_samples || w2->dtype != wdt ||
          w2->col_stride != 1 || ((uintptr_t)w2->data % (size_t)dtype_size(wdt)) != 0)
        return XHIST_ERR_UNSUPPORTED;
      fn = fast_kernel_two_weights(sdt, wdt, D, scan, &vec);
      if (!fn) return XHIST_ERR_UNSUPPORTED;
      break;
    }
    if (mixed) {
      fn = xhist_pick_mixed(weighted, D, scan);
      vec = 4;
      continue;  // (no kernel: the loop goes on to the generic family)
    }
    fn = fast ? (i64dom ? int64_domain_kernel(wdt, D, scan, pl.hist, &vec) : fast_kernel(sdt, wdt, D, scan, pl.hist, &vec))
              : generic_kernel(p->cmp, weighted, pl.hist == kHistLds, tables_in_lds);
  }
  if (!fn) return fail(XHIST_ERR_HIP, "internal: no kernel for this combination");
  // One input without weights, long rows: twice the samples per lane and tile — the 128 bytes per lane in flight that the
  // weighted kernel has with its two streams.  float64, one row of 10^9 samples, 100 bins (the headline's 8 B/sample variant):
  // 1.20-1.24 -> 1.14-1.16 ms (0.83 -> 0.86-0.88 of 8 TB/s); float32, BASELINE C4 (456 / 3650 rows of 1 036 800): 0.2872 ->
  // 0.2838 ms (0.823 -> 0.833) and 2.228 -> 2.208 ms (0.849 -> 0.857), profiles/r03_u8_unroll8.txt.  Short rows keep their tiles
  // (the geometry rules further down were fitted to them); float64 with many rows was not measured and stays as it was.
  bool long_tiles = false;
  if (fast && !mixed && !two && !i64dom && !weighted && D == 1 && pl.hist == kHistLds && (scan == 1 || scan == 2 || scan == kScanArith32) &&
      !kn.block_threads && !kn.grid_blocks) {
    kernel_fn lf = nullptr;
    // (exactly the two shape classes that were measured: one float32 row of 3*10^7 ... 10^9 samples came out 4-10 % SLOWER
    // with the long tiles in tools/size_ramp.py — its one-workgroup-per-CU geometry already has 64 KiB per CU in flight)
    if (sdt == XHIST_F64 && n_rows == 1 && n_cols >= ((int64_t)1 << 29)) lf = xhist_pick_f64_long(scan);
    else if (sdt == XHIST_F32 && n_rows >= 64 && n_cols >= ((int64_t)1 << 19)) lf = xhist_pick_f32_long(scan);
    if (lf) {
      fn = lf;
      long_tiles = true;
    }
  }
  sc.fn = fn;
  sc.fast = fast;
  sc.mixed = mixed;
  sc.use_f32 = use_f32;
  sc.tables_in_lds = tables_in_lds;
  sc.long_tiles = long_tiles;
  sc.vec = fast ? vec : 1;
  sc.scan = scan;
  sc.hist = pl.hist;
  sc.cl2 = pl.cl2;
  sc.tset = tset;
  sc.table_bytes = table_bytes;
  sc.hist_bytes = pl.hist_bytes;
  sc.lds_bytes = (tables_in_lds ? table_bytes : 0) + pl.hist_bytes;
  sc.n_slices = 1;
  sc.slice_bins = p->n_bins;
  return XHIST_OK;
}

// ---- partitions of the partitioned mode (execute_partitioned_rows; choose_slices prices it) ---------------------------
// 2^14 float64 or 2^15 uint32 bins = 128 KiB of LDS per partition, unless that leaves only a handful:
// A handful of partitions is slower than a few dozen: the routing pass ranks a tile's records with ONE returning LDS
// counter per partition, and a tile's 8192 adds on two or three addresses serialise (a tile lies in one row, so rows
// that share a pass do not help).  5*10^8 samples, ms: float32 pairs + weights 160 x 160 bins, 2 partitions -> 13:
// 3.04 -> 2.32; 200 x 200, 3 -> 20: 2.82 -> 2.35; float32 pair counts 300 x 300, 3 -> 22: 2.75 -> 1.58; 400 x 400,
// 5 -> 20: 2.33 -> 1.60; float64 pair counts 300 x 300 2.78 -> 2.36; 10^5 bins 1-D, 4 -> 25: 2.65 -> 1.53; 12 rows x
// 200 x 200 float32 weighted, 3 -> 10 per row: 2.89 -> 2.43 (profiles/r03_t_few_partitions.txt).  So the bins are cut
// finer — down to 2^11 per partition — until a row has 16 partitions ("min_parts" overrides).  float64 samples with
// float64 weights, whose tiles are half as long, gain nothing (4.10 -> 4.06, 12 rows 4.09 -> 4.34) and keep the big ones.
struct PartGeom {
  int shift;        // bins per partition = 1 << shift
  int64_t n_parts;  // partitions per row
};
static PartGeom part_geometry(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in) {
  PartGeom g;
  g.shift = in.weighted ? 14 : 15;
  g.n_parts = (p->n_bins + ((int64_t)1 << g.shift) - 1) >> g.shift;
  if (in.weighted && in.sdt == XHIST_F64 && in.wdt == XHIST_F64 && !kn.min_parts) return g;
  const bool rows_share = in.n_rows > 1 && in.n_cols < ((int64_t)1 << 27);  // (uniform_rows in execute_partitioned_rows: several rows per pass)
  const int64_t want_parts = kn.min_parts ? kn.min_parts : 16;
  while (g.shift > 11 && g.n_parts < want_parts) {
    const int64_t finer = (p->n_bins + ((int64_t)1 << (g.shift - 1)) - 1) >> (g.shift - 1);
    // rows that fit ONE pass with 8+ partitions each stay in one pass (a pass costs ~0.1 ms beyond its traffic)
    if (rows_share && g.n_parts >= 8 && in.n_rows * g.n_parts <= 128 && in.n_rows * finer > 128) break;
    --g.shift;
    g.n_parts = finer;
  }
  return g;
}

// ---- a few times the LDS capacity: bin slices ---------------------------------------------------
// S launches, each streaming all samples and keeping 1/S of the bins in LDS (hist_fast<SLICED>),
// cost S x the streaming time; the partitioned mode moves B + 2 x record bytes per sample once and needs a few
// long rows.  Round 3, 5*10^8 samples, slices | partitioned ms (profiles/r03_t_few_partitions.txt): float32 pairs +
// float32 weights S = 2: 1.80 | 2.32, S = 3: 2.67 | 2.35, S = 4: 3.53 | 2.21; float64 pairs + float64 weights S = 2:
// 3.47 | 4.03, S = 3: 5.21 | 4.06; float32 pair counts (packed uint16 slices) S = 2: 1.73 | 1.58, S = 3: 2.62 | 1.60;
// float64 pair counts S = 2: 2.43 | 2.36, S = 3: 3.69 | 2.38.  (Round 1's rule — written when the partitioned mode took
// three passes, 9.3 ms for 200 x 200 weighted bins — kept slices up to S = 3-4.)
static void choose_slices(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, StreamChoice& sc) {
  const size_t lds_cap = p->lds_max;
  if (!(sc.fast && in.float_samples && sc.hist == kHistGlobal && !kn.force_global && !in.two && kn.slices_pref >= 0 &&
        p->n_bins < ((int64_t)1 << 24) && (sc.scan == 1 || sc.scan == 2 || sc.scan == kScanArith) && sc.table_bytes + 4096 < lds_cap))
    return;
  const bool weighted = in.weighted;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const size_t budget = lds_cap - sc.table_bytes - 2048;
  const int64_t cap = weighted ? (int64_t)(budget / 8) - 32 : (((int64_t)(budget / 2) - 66) & ~(int64_t)1);
  const int64_t S = (p->n_bins + cap - 1) / cap;
  int64_t B = 0;
  for (int d = 0; d < in.n_arrays(); ++d) B += dtype_size(in.array(d).dtype);
  const int64_t rec = 2 + (weighted ? (in.wdt == XHIST_F32 ? 4 : 8) : 0);  // a record: uint16 code + the weight in its own precision
  const PartGeom pg = part_geometry(p, kn, in);
  const int64_t parts_per_row = pg.n_parts;
  const bool part_ok = kn.partition >= 0 && n_rows <= 64 && n_cols >= ((int64_t)1 << 22) && parts_per_row <= kPartMaxParts;
  // per sample: a slice pass streams B bytes at ~6.5 TB/s (packed uint16 counters: no faster than 5.7 x 10^11 samples
  // a second); the partitioned mode moves B + 2 x record bytes at ~4.7 TB/s and no faster than 3.3 x 10^11 samples a second
  const double per_slice = std::max((double)B / 6.5e12, weighted ? 0.0 : 1.0 / 5.7e11);
  const double per_part = std::max(((double)B + 2.0 * (double)(weighted ? std::min<int64_t>(rec, 8) : rec)) / 4.7e12, 1.0 / 3.3e11);
  // (+ ~0.1 ms per routing / adding-up pass: rows share a pass while rows x partitions <= 128)
  const double n_all = (double)n_rows * (double)n_cols;
  const int64_t rows_per_pass = (n_rows > 1 && n_cols < ((int64_t)1 << 27) && parts_per_row * 2 <= 128) ? std::max<int64_t>(1, 128 / parts_per_row) : 1;
  const double t_part = n_all * per_part + (double)((n_rows + rows_per_pass - 1) / rows_per_pass) * 1.0e-4;
  // every slice pass ends with one global atomic per non-empty bin and workgroup (~2 x 10^11 a second for the chip) and costs
  // ~13 us to launch: 10^7 float64 pairs into 512 x 512 counts, 5 slices 0.377 ms against 0.112 partitioned
  const double slice_wgs = (double)std::max<int64_t>(p->cus, n_rows);
  const double slice_bins_each = (double)((p->n_bins + S - 1) / S);
  const double t_slice_fixed = 13e-6 + slice_wgs * std::min(slice_bins_each, n_all / slice_wgs) / 2.0e11;
  bool choose = kn.slices_pref > 0 ? S <= 64 : (kn.partition > 0 ? false : (part_ok ? (double)S * (n_all * per_slice + t_slice_fixed) <= t_part : S <= 16));
  if (choose && kn.slices_pref == 0) {
    // few samples: S launches cost S x ~13 us before they stream anything, memory-side atomics 2.4-2.7 x 10^10
    // per second (10^5 samples, 256 x 256 weighted bins: 4 slices 54 us, global atomics 13 us)
    const double t_global = 8e-6 + n_all / (weighted ? 2.4e10 : 2.7e10);
    const double t_slices = (double)S * (13e-6 + n_all * (double)B / 4.0e12);
    choose = t_slices <= t_global;
  }
  if (!choose || S < 1) return;
  const int shist = weighted ? kHistLds : kHistPacked;
  kernel_fn sfn = fast_kernel_sliced(in.sdt, in.wdt, in.D, sc.scan, shist, &sc.vec);
  if (!sfn) return;
  sc.fn = sfn;
  sc.hist = shist;
  sc.cl2 = 0;
  sc.n_slices = (int)S;
  sc.slice_bins = ((p->n_bins + S - 1) / S + 1) & ~(int64_t)1;  // even: packed counters pair up inside a slice
  sc.hist_bytes = weighted ? ((size_t)sc.slice_bins + 32) * 8 : (((size_t)sc.slice_bins + 1) / 2 + 32) * 4;
  sc.tables_in_lds = true;
  sc.lds_bytes = sc.table_bytes + sc.hist_bytes;
}

// Row r of every array of a call: the samples into row_s, the weights into row_w.  Plain rows, no groups: a view is one row, or
// rows at one row stride when the arrays have no groups to begin with (the partitioned mode's several rows per pass).
static void row_views(const Inputs& in, int64_t r, xhist_array* row_s, xhist_array& row_w) {
  for (int d = 0; d < in.n_arrays(); ++d) {
    const xhist_array& a = in.array(d);
    xhist_array& v = d < in.D ? row_s[d] : row_w;
    v = a;
    v.data = const_cast<void*>(advance(a.data, a.dtype, row_offset(r, a.row_stride, a.inner_rows, a.outer_stride)));
    v.inner_rows = 0;
    v.outer_stride = 0;
  }
}

// The digitize of the routing pass.  It keeps the digitize tables in LDS next to its sort buffers; where they do not fit (or
// cost a workgroup per CU) and the edges are arithmetic (C5: 2 x 1025 np.linspace edges, 32 KiB of tables) it digitizes
// table-free.
static RouteDigitize route_digitize(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const StreamChoice& sc, int64_t n_parts) {
  const int D = in.D, sdt = in.sdt;
  const bool weighted = in.weighted;
  const int scan = sc.scan;
  const TableSet* tset = sc.tset;
  RouteDigitize r{scan, tset, sc.use_f32, RouteGeom{}};
  const bool can_arith = p->arith && kn.arith_pref >= 0 && n_parts <= 128;
  const int w_tag = weighted ? in.wdt : -1;
  // geometry first: the long tile with the arithmetic digitize where the edges allow it, else with the tables if both
  // fit the LDS, else the short tile
  RouteGeom& geom = r.geom;
  geom = route_geom_for(kn, sdt, w_tag, D, can_arith ? kScanArith : scan);
  if (geom.spl == 8 && (can_arith || scan == kScanArith)) {
    if (scan != kScanArith) {
      r.scan = kScanArith;
      r.tset = &p->ts[0][0];
      r.f32 = false;
    }
  } else {
    if (geom.spl == 8 && !kn.route_spl &&
        part_route_lds((size_t)tset->words * 8, (int)n_parts, weighted, route_tile(geom.block, 8), geom.block) > p->lds_max)
      geom.spl = 4;
    if (can_arith && scan != kScanArith) {
      const int t4 = route_tile(geom.block, geom.spl);
      const size_t lds_tab = part_route_lds((size_t)tset->words * 8, (int)n_parts, weighted, t4, geom.block),
                   lds_notab = part_route_lds(0, (int)n_parts, weighted, t4, geom.block);
      if (lds_tab > p->lds_max || (size_t)160 * 1024 / lds_notab > (size_t)160 * 1024 / lds_tab) {
        r.scan = kScanArith;
        r.tset = &p->ts[0][0];
        r.f32 = false;
      }
    }
  }
  // non-uniform edges: the packed entries (general variant) instead of a binary search or a 2-4-edge scan per sample and
  // dimension — the routing pass feels its digitize (5*10^8 float64 pairs into 512 x 512 counts: linspace 2.07 ms, random
  // edges 2.48, geometric 3.42; profiles/r04_l_*) — where entries and sort buffers fit the LDS together
  const int pk_np = sdt == XHIST_F64 ? p->pk_np : (sdt == XHIST_F32 && sc.use_f32 ? p->pk32_np : 0);
  if (pk_np && kn.pack_pref >= 0 && r.scan != kScanArith && (r.scan == 0 || r.scan >= 2 || kn.pack_pref > 0) && n_parts <= 128) {
    const TableSet& pk = sdt == XHIST_F64 ? p->ts_pk : p->ts_pk32;
    int spl = geom.spl;
    if (spl == 8 && part_route_lds((size_t)pk.words * 8, (int)n_parts, weighted, route_tile(geom.block, 8), geom.block) > p->lds_max) spl = 4;
    if (part_route_lds((size_t)pk.words * 8, (int)n_parts, weighted, route_tile(geom.block, spl), geom.block) <= p->lds_max &&
        route_kernel(sdt, w_tag, D, kScanPackG, false, geom.block, spl)) {
      r.scan = kScanPackG;
      r.tset = &pk;
      geom.spl = spl;
    }
  }
  return r;
}

// ---- histograms beyond LDS: partitioned multi-pass instead of memory-side atomics ----------
// (a few long rows — e.g. one joint histogram per time step — run it row by row)
// XHIST_ERR_UNSUPPORTED: nothing was launched.  The output may have been zeroed by then; `accumulate` is 1 if so.
static int execute_partitioned_rows(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const StreamChoice& sc, void* out,
                                    int& accumulate, hipStream_t stream) {
  const bool weighted = in.weighted;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  // (sc.fast with float samples: the vector family, whose arrays all have unit column stride — choose_streaming)
  if (!(sc.fast && in.float_samples && sc.hist == kHistGlobal && !kn.force_global && kn.partition >= 0 && n_rows <= 64 && !in.two &&
        sc.n_slices == 1))
    return XHIST_ERR_UNSUPPORTED;
  const PartGeom pg = part_geometry(p, kn, in);
  const int shift = pg.shift;
  const int64_t n_parts = pg.n_parts;
  const bool big_enough = n_cols >= ((int64_t)1 << 22) || (kn.partition > 0 && n_cols >= 4);  // part_scatter reads whole weight quads
  if (n_parts > kPartMaxParts || !big_enough || (size_t)(1u << shift) * (weighted ? 8 : 4) + 1024 > p->lds_max) return XHIST_ERR_UNSUPPORTED;
  if (!accumulate) {
    if (int zrc = zero_output(out, n_rows * p->n_bins, stream)) return zrc;
    accumulate = 1;  // (for the streaming kernels, should nothing below launch)
  }
  LaunchRecord rec(p, stream);
  const PartCall pc{in.sdt, in.wdt, n_cols, shift, (int)n_parts, sc.scan, sc.use_f32, sc.tset, route_digitize(p, kn, in, sc, n_parts), &rec};
  const int r_block = pc.route.geom.block, r_tile = route_tile(r_block, pc.route.geom.spl);
  // rows that follow each other at one stride go through the routing pass several at a time
  // (32 x 3*10^7 float32 pairs + weights, 300 x 300 bins: 8.05 -> 6.02 ms; 8 x 6*10^7 float64, 512 x 512: 5.17 -> 4.18;
  // rows of 5*10^8 samples gain nothing — 8.63 -> 8.95 ms with 128 partitions in flight — and stay one per pass)
  // a single row of float64 samples with float64 weights below ~1.5 x 10^7 samples: the routing pass's fixed costs (chunk
  // pool, lists, one partial chunk per workgroup and partition) show, and count + prefix + scatter is 9-15 % faster
  // (5*10^6: 0.155 | 0.132 ms, 10^7: 0.191 | 0.174, 2*10^7: 0.273 | 0.269: profiles/r03_h_fused_vs_three_pass_mid_sizes.txt);
  // every other dtype combination is ahead with one pass from 5*10^6 samples on
  const bool three_pass = kn.fused_pref == 0 && kn.partition == 0 && n_rows == 1 && weighted && in.sdt == XHIST_F64 && in.wdt == XHIST_F64 && n_cols < 15000000;
  const int fused_use = three_pass ? -1 : kn.fused_pref;
  bool uniform_rows = fused_use >= 0 && n_rows > 1 && n_parts * 2 <= 128 && n_cols < ((int64_t)1 << 27);
  for (int d = 0; d < in.n_arrays(); ++d) uniform_rows &= in.array(d).inner_rows == 0;
  xhist_array row_s[XHIST_MAX_DIMS], row_w;
  const xhist_array* row_wp = weighted ? &row_w : nullptr;
  int rc = XHIST_OK;
  int64_t r = 0;
  while (uniform_rows && r < n_rows && rc == XHIST_OK) {
    int rows = (int)std::min<int64_t>(n_rows - r, 128 / n_parts);
    const size_t tab_bytes = pc.route.scan == kScanArith ? 0 : (size_t)pc.route.tset->words * 8;
    while (rows > 1 && part_route_lds(tab_bytes, rows * (int)n_parts, weighted, r_tile, r_block) > p->lds_max) --rows;
    if (rows < 2) break;  // (one row at a time below)
    row_views(in, r, row_s, row_w);
    void* row_out = static_cast<char*>(out) + (size_t)r * p->n_bins * 8;
    rc = execute_partitioned_fused(p, kn, pc, row_s, row_wp, row_out, stream, r == 0, r + rows == n_rows, rows);
    if (rc == XHIST_ERR_UNSUPPORTED) {
      if (r > 0) rc = fail(XHIST_ERR_HIP, "internal: partitioned mode refused rows from %lld after accepting row 0", (long long)r);
      else rc = XHIST_OK;  // nothing launched: row by row below
      break;
    }
    r += rows;
  }
  for (; r < n_rows && rc == XHIST_OK; ++r) {
    row_views(in, r, row_s, row_w);
    void* row_out = static_cast<char*>(out) + (size_t)r * p->n_bins * 8;
    // one routing pass (44 B per C5 sample) where it applies, else count + prefix + scatter (52.5 B); the
    // choice depends on the plan and the dtypes only, so every row of a call takes the same route
    rc = fused_use >= 0 ? execute_partitioned_fused(p, kn, pc, row_s, row_wp, row_out, stream, r == 0, r == n_rows - 1)
                         : XHIST_ERR_UNSUPPORTED;
    if (rc == XHIST_ERR_UNSUPPORTED) rc = execute_partitioned(p, kn, pc, row_s, row_wp, row_out, stream, r == 0, r == n_rows - 1);
    if (rc == XHIST_ERR_UNSUPPORTED && r > 0) rc = fail(XHIST_ERR_HIP, "internal: partitioned mode refused row %lld after accepting row 0", (long long)r);
  }
  return rc;  // UNSUPPORTED (from row 0, nothing launched): the caller goes on to global atomics
}

// rows per launch are bounded by the grid limit
static constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;

// Launch geometry of the streaming kernels.
struct StreamGeom {
  int unroll;
  int block, bpc;     // threads per workgroup, workgroups per CU
  int over;           // oversubscription of the chip (many rows)
  bool exact;         // exactly the workgroups that are resident at once, a whole number per row
  int64_t target;     // workgroups over all rows
  int64_t tile;       // samples a workgroup takes per step
  int64_t col_chunk;  // columns per launch
  int64_t segs0;      // workgroups per row of the first launch
  bool direct;        // plain stores of the LDS histogram, no zeroing pass
};

// ---- geometry -----------------------------------------------------------------------------
// Workgroups per CU are sized by bytes in flight, not by occupancy: measured on MI355X
// (profiles/r01_a_sweep.jsonl) the streaming rate peaks at ~64 KiB of outstanding loads per CU
// (f64+weights: 2 x 256 threads x 128 B; f64: 4 x 256 x 64 B) and falls by 5-10% with more.
static StreamGeom streaming_geometry(const xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const StreamChoice& sc, int accumulate) {
  const int D = in.D;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const bool fast = sc.fast, mixed = sc.mixed;
  const int vec = sc.vec, scan = sc.scan, hist = sc.hist;
  const size_t lds_bytes = sc.lds_bytes;
  const int block_threads = kn.block_threads, grid_blocks = kn.grid_blocks;
  StreamGeom g;
  const int kUnroll = sc.long_tiles ? 8 : (mixed ? mixed_unroll(D) : (fast ? unroll_for(D, vec, scan) : 1));
  int64_t lane_bytes = 0;
  for (int d = 0; d < in.n_arrays(); ++d) lane_bytes += dtype_size(in.array(d).dtype);
  if (in.two) lane_bytes += dtype_size(in.weights->dtype);
  lane_bytes *= fast ? (int64_t)vec * kUnroll : 4;
  int block = block_threads ? block_threads : 256;
  if (!block_threads && lds_bytes > 40 * 1024) {
    // one to three workgroups fit a CU: make them carry the ~64 KiB of loads in flight together
    // (2 x f64 with 128 B per lane: 512 threads; 2 x f32 with 64 B per lane and 88 KB of LDS:
    // 1024 — 4.85 TB/s at 512).  The packed-uint16 histogram waits on returning atomics and wants
    // half as much again (C3: 768).
    const int fit = (int)std::max<int64_t>(1, std::min<int64_t>(3, (int64_t)(160 * 1024 / lds_bytes)));
    int64_t want = (64 * 1024) / (fit * std::max<int64_t>(lane_bytes, 1));
    if (hist == kHistPacked) want += want / 2;
    block = (int)std::min<int64_t>(1024, std::max<int64_t>(256, (want + 255) / 256 * 256));
  }
  if (!block_threads && n_rows > 1 && lds_bytes <= 40 * 1024) {
    // many rows, one workgroup each: a tile should be ~1/4 of the row or most of the workgroup
    // idles in the ragged tile (100k rows x 3650: 0.46 -> 0.39 ms; 356k x 1024: 1.3 -> 0.58 ms)
    const int64_t per_lane = fast ? (int64_t)vec * unroll_for(D, vec, scan) : 4;
    int64_t want = n_cols / (4 * per_lane);
    block = 64;
    while (block < 256 && block * 2 <= want) block *= 2;
  }
  // (generic family, long rows: 512-thread workgroups — 2 x 10^8 f32 samples 0.74 -> 0.61 ms)
  if (!block_threads && !fast && n_cols >= 65536 && lds_bytes <= 40 * 1024) block = 512;
  int bpc = (int)std::max<int64_t>(1, std::min<int64_t>(8, (64 * 1024 + block * lane_bytes / 2) / (block * lane_bytes)));
  // Many rows: a workgroup is tied to one row, so the tail is balanced by OVERSUBSCRIBING the chip 8x
  // with small workgroups (C4 shape: 5.6 -> 6.5 TB/s) — as long as their flushes are cheap: every
  // workgroup ends with one global atomic per non-empty bin (runs of consecutive bins: ~2*10^11 per
  // second for the chip), and the workgroups of one row meet on the same addresses (~25 ns each).  The
  // factor is halved until the flushes would take under 20 % of the streaming time; a few rows are one
  // row in a few parts and never oversubscribe.
  // (2 x 5*10^7 f32, 50 bins: 8192 workgroups 149 us, 2 x 128 of 1024 threads 65 us;
  //  32 x 312500 f64, 1000 bins: 4896 workgroups 45 us, 32 x 8 of 512 threads 19 us.)
  const int64_t sample_bytes = lane_bytes / (fast ? (int64_t)vec * kUnroll : 4);
  const double total_samples = (double)n_rows * (double)n_cols;
  // (C4 shard, 456 rows: 18 workgroups per row 0.2875 ms, 36: 0.2839 — and an ODD number per row is 2.5-7 % slower than its
  // even neighbours: 17 / 19 / 21 / 23 / 27 / 31 per row 0.2946 / 0.2942 / 0.2980 / 0.2965 / 0.3067 / 0.3013 ms against
  // 0.2854-0.2876 for 16 ... 28, profiles/r03_n_c4_segs_per_row.txt: the workgroups of a row walk its 16 KiB tiles interleaved,
  // and an odd stride between a workgroup's tiles lands on the memory channels worse.  Hence 16 x, and an even count below.)
  int over = n_rows <= 16 ? 1 : 16;
  if (!grid_blocks && over > 1) {
    const double t_stream = total_samples * (double)sample_bytes / 6.0e12;
    while (over > 1) {
      const double wgs = std::max<double>((double)n_rows, (double)p->cus * bpc * over);
      const double dense = wgs * std::min<double>((double)p->n_bins, total_samples / wgs) / 2.0e11;
      const double serial = wgs / (double)n_rows * 25e-9;
      if (std::max(dense, serial) <= 0.2 * t_stream) break;
      over /= 2;
    }
  }
  const bool exact = over == 1;  // exactly the workgroups that are resident at once, a whole number per row
  if (!block_threads && !grid_blocks && exact && n_cols >= 65536 && fast && hist == kHistLds && lds_bytes <= 40 * 1024) {
    // Small histogram, long rows: ONE workgroup per CU, as wide as the loads in flight ask for.  Measured
    // (tools/size_ramp.py, profiles/r01_u_*): ~32 KiB per CU for 8-byte samples with the one-compare
    // digitize (f64, uniform-style edges: 512 threads), ~64 KiB for 4-byte samples, which do twice the LDS
    // atomics per byte, and for every heavier digitize (f32, non-uniform edges, int64 domain: 1024; 8-byte
    // geometric edges at 512 threads: 300 us per 10^8, at 1024: 234).  8-byte samples with 128 B per lane
    // (f64 + f64 weights, two f64 inputs) only below 256 MB — above, two
    // 256-thread workgroups per CU are 15-20 % ahead.  The block shrinks until there is a tile for half
    // the CUs, and to whatever size lets a whole number of workgroups per row fill the chip best.
    int64_t ssz = 0;
    for (int d = 0; d < D; ++d) ssz = std::max<int64_t>(ssz, dtype_size(in.samples[d].dtype));
    int64_t threads_per_cu = (int64_t)bpc * 256;  // (block is 64..256 here, bpc was sized for 256)
    block = 256;
    if (mixed || !(lane_bytes >= 128 && ssz >= 8 && total_samples * (double)sample_bytes > (double)((int64_t)256 << 20))) {
      int64_t per_cu = (ssz >= 8 && scan == 1 && in.float_samples ? 32 : 64) * 1024 / std::max<int64_t>(lane_bytes, 1);
      // the mixed-dtype kernels convert after loading and want the whole CU: float32 x float64, 2 x 10^8 samples:
      // 256 threads per CU 0.88 ms, 512 0.52, 1024 0.44 (tools/mixtures.py)
      if (mixed) per_cu = 1024;
      threads_per_cu = std::min<int64_t>(1024, std::max<int64_t>(256, per_cu / 256 * 256));
      block = (int)threads_per_cu;
      while (block > 256 && n_rows * (n_cols / ((int64_t)block * vec * kUnroll)) < p->cus / 2) block -= 256;
      if (block == 768) block = 512;
    }
    const int64_t slots = (int64_t)p->cus * threads_per_cu;  // threads the launch should keep resident
    int best = 256;
    int64_t best_used = -1;
    for (int b = block; b >= 256; b /= 2) {
      const int64_t used = n_rows * (slots / (n_rows * b)) * b;
      if (used > best_used + best_used / 16) { best_used = used; best = b; }  // a smaller block must fill 6 % more
    }
    if (best_used > 0) {
      block = best;
      bpc = (int)std::max<int64_t>(1, threads_per_cu / block);
    } else {
      block = 256;  // more rows than the chip holds workgroups: one 256-thread workgroup each
    }
  }
  bpc = std::min<int>(bpc, 2048 / block);
  if (lds_bytes) bpc = std::max<int>(1, std::min<int64_t>(bpc, (int64_t)(160 * 1024 / lds_bytes)));
  int64_t target = grid_blocks ? grid_blocks : (int64_t)p->cus * bpc * over;
  if (!grid_blocks && exact) {
    // small inputs: streaming gains ~25 GB/s per 256 threads, every workgroup of a row costs ~12 ns at the
    // end.  The sum of the two is minimal at sqrt(bytes / (25 GB/s * 12 ns)) workgroups per row
    // (10^6 f64 samples: 18 -> 9 us)
    // A big histogram raises the second term: a workgroup flushes min(bins, its samples) counters at
    // ~2*10^11 per second (256 x 256 packed counters, 10^7 samples: 256 workgroups 117 us, 96: 94 us).
    const double bytes = (double)n_cols * (double)sample_bytes;
    const double rate = 25e9 * block / 256;
    const int64_t cap = std::max<int64_t>(1, target / n_rows);
    int64_t per_row = std::max<int64_t>(1, std::min<int64_t>(cap, (int64_t)std::sqrt(bytes / (rate * 12e-9))));
    const double flushed = std::min<double>((double)(sc.n_slices > 1 ? sc.slice_bins : p->n_bins), (double)n_cols / (double)per_row);
    const double per_wg = std::max(12e-9, flushed / 2.0e11);
    per_row = std::max<int64_t>(1, std::min<int64_t>(cap, (int64_t)std::sqrt(bytes / (rate * per_wg))));
    target = per_row * n_rows;  // a whole number per row, never more than are resident at once
  }
  const int64_t tile = fast ? (int64_t)block * vec * kUnroll : (int64_t)block * 4;
  const int64_t tiles_per_row = (n_cols + tile - 1) / tile;
  // columns per launch bounded so that no workgroup can overflow a uint32 LDS counter (< 2^31 samples per workgroup per launch)
  int64_t col_chunk = n_cols;
  {
    int64_t segs_full = std::max<int64_t>(1, std::min<int64_t>(tiles_per_row, (target + n_rows - 1) / n_rows));
    const int64_t per_wg = ((tiles_per_row + segs_full - 1) / segs_full) * tile;
    if (per_wg >= ((int64_t)1 << 31)) col_chunk = segs_full * (((int64_t)1 << 30) / tile) * tile;
  }
  // One workgroup per row (many short rows): its LDS histogram IS the row's result, so it is stored
  // with plain writes — no zeroing pass over the output, no global atomics (10^5 rows x 1000 f32,
  // 50 bins: the 5 x 10^6 flush atomics alone took the whole 0.18 ms).
  int64_t segs0 = std::max<int64_t>(1, std::min<int64_t>((std::min(col_chunk, n_cols) + tile - 1) / tile, (target + n_rows - 1) / n_rows));
  if (!exact && !grid_blocks && segs0 > 1 && (segs0 & 1) && segs0 + 1 <= (std::min(col_chunk, n_cols) + tile - 1) / tile) ++segs0;
  g.unroll = kUnroll;
  g.block = block;
  g.bpc = bpc;
  g.over = over;
  g.exact = exact;
  g.target = target;
  g.tile = tile;
  g.col_chunk = col_chunk;
  g.segs0 = segs0;
  g.direct = !accumulate && !in.two && fast && hist == kHistLds && sc.n_slices == 1 && col_chunk >= n_cols && segs0 == 1 && n_rows <= kMaxGrid;
  return g;
}

// ---- the streaming launches: column chunks x row ranges x bin slices ----------------------------------
static int launch_streaming(xhist_plan* p, const PlanKnobs& kn, const Inputs& in, const StreamChoice& sc, const StreamGeom& g, void* out,
                            void* out2, int accumulate, hipStream_t stream) {
  const int D = in.D;
  const int64_t n_rows = in.n_rows, n_cols = in.n_cols;
  const xhist_array *samples = in.samples, *weights = in.weights, *weights2 = in.weights2;
  const DimTable* dims = sc.tset->dim;
  const int32_t table_words = (sc.scan == kScanArith || sc.scan == kScanArith32) ? 0 : sc.tset->words;  // arithmetic edges: nothing to stage
  Params base = fill_params(samples, weights, D, *sc.tset, table_words, n_rows, n_cols, p->n_bins, out);
  base.tables_in_lds = sc.tables_in_lds ? 1 : 0;
  base.copies_log2 = sc.cl2;
  base.direct_store = g.direct ? 1 : 0;
  if (in.two) {
    base.w2_rs = weights2->row_stride;
    base.w2_ir = weights2->inner_rows;
    base.w2_os = weights2->outer_stride;
  }
  HIPC(set_dynamic_lds((const void*)sc.fn, sc.lds_bytes));
  if (!accumulate && !g.direct && !in.two)
    if (int zrc = zero_output(out, n_rows * p->n_bins, stream)) return zrc;
  bool first_launch = true;
  LaunchRecord rec(p, stream);
  char desc[384];
  for (int64_t c0 = 0; c0 < n_cols; c0 += g.col_chunk) {
    const int64_t nc = std::min(g.col_chunk, n_cols - c0);
    const int64_t tpr = (nc + g.tile - 1) / g.tile;
    for (int64_t r0 = 0; r0 < n_rows;) {
      int64_t segs = std::max<int64_t>(1, std::min<int64_t>(tpr, (g.target + (n_rows - r0) - 1) / (n_rows - r0)));
      if (!g.exact && !kn.grid_blocks && segs > 1 && (segs & 1) && segs + 1 <= tpr) ++segs;  // oversubscribed rows: an even number each
      const int64_t nr = std::min<int64_t>(n_rows - r0, kMaxGrid / segs);
      Params kp = base;
      for (int d = 0; d < D; ++d) kp.s_ptr[d] = advance(samples[d].data, samples[d].dtype, c0 * samples[d].col_stride);
      if (in.weighted) kp.w_ptr = advance(weights->data, weights->dtype, c0 * weights->col_stride);
      if (in.two) {
        kp.w2_ptr = advance(weights2->data, weights2->dtype, c0);
        kp.out2 = static_cast<char*>(out2) + (size_t)r0 * p->n_bins * 8;
      }
      kp.row0 = r0;
      kp.n_rows = nr;
      kp.n_cols = nc;
      kp.out = static_cast<char*>(out) + (size_t)r0 * p->n_bins * 8;
      kp.segs = (int32_t)segs;
      const dim3 grid((unsigned)(nr * segs));
      if (first_launch)
        if (int rrc = rec.begin(kn.profile)) return rrc;
      for (int sl = 0; sl < sc.n_slices; ++sl) {  // (one launch unless the histogram is built in bin slices)
        kp.slice_lo = (int64_t)sl * sc.slice_bins;
        kp.slice_n = (int32_t)std::min<int64_t>(sc.slice_bins, p->n_bins - kp.slice_lo);
        XH_LAUNCH_PICKED(sc.fn, grid, dim3(g.block), sc.lds_bytes, stream, kp);
        HIPC(hipGetLastError());
      }
      if (first_launch) {
        snprintf(desc, sizeof desc,
                 "family=%s hist=%s vec=%d unroll=%d block=%d grid=%lld segs=%lld lds_bytes=%zu copies=%d table_bytes=%zu "
                 "lut_k0=%d steps0=%d scan=%d weighted=%d D=%d cmp=%s lds_cap=%zu%s slices=%d direct_store=%d",
                 sc.mixed ? "fast mixed-dtypes" : (sc.fast ? "fast" : "generic"), sc.hist == kHistLds ? "lds" : (sc.hist == kHistPacked ? "packed16" : "global"),
                 sc.fast ? sc.vec : 1, sc.fast ? g.unroll : 1, g.block, (long long)(nr * segs), (long long)segs, sc.lds_bytes, 1 << sc.cl2,
                 sc.table_bytes, dims[0].lut_k, dims[0].steps, sc.scan, (int)in.weighted, D,
                 sc.use_f32 ? "f32thr" : (p->cmp == XHIST_CMP_I64 ? "i64" : (p->cmp == XHIST_CMP_F64 ? "f64" : "per-input")), p->lds_max,
                 in.two ? " weights=2" : "", sc.n_slices, (int)g.direct);
      }
      first_launch = false;
      r0 += nr;
    }
  }
  return rec.end(desc);
}

// weights2 / out2 (optional): a second weight array binned in the same pass (hist_fast<..., W2>).
// Only the vector family with LDS histograms does that; anything else returns
// XHIST_ERR_UNSUPPORTED before touching the outputs, and the caller runs two passes.
static int execute_device(xhist_plan* p, const xhist_array* samples, const xhist_array* weights, int64_t n_rows, int64_t n_cols,
                          void* out, int accumulate, hipStream_t stream, const xhist_array* weights2, void* out2) {
  const bool two = weights2 != nullptr;
  const int64_t out_elems = n_rows * p->n_bins;
  if (out_elems == 0) return XHIST_OK;
  if (n_cols == 0) {
    if (!accumulate) {
      if (int zrc = zero_output(out, out_elems, stream)) return zrc;
      if (two)
        if (int zrc = zero_output(out2, out_elems, stream)) return zrc;
    }
    return XHIST_OK;
  }
  PlanKnobs kn;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    kn = p->knobs;
  }
  Inputs in;
  in.samples = samples;
  in.weights = weights;
  in.weights2 = weights2;
  in.n_rows = n_rows;
  in.n_cols = n_cols;
  in.D = p->n_dims;
  in.sdt = samples[0].dtype;
  in.wdt = weights ? weights->dtype : -1;
  in.weighted = weights != nullptr;
  in.two = two;
  in.float_samples = in.sdt == XHIST_F64 || in.sdt == XHIST_F32;

  // ---- many short rows / leading-axis reductions: one row per lane (xhist_lanes.hip.h) --------
  if (kn.lanes >= 0 && !kn.force_generic && !kn.force_global && !two) {
    const int rc = execute_lanes(p, kn, in, out, accumulate, stream);
    if (rc != XHIST_ERR_UNSUPPORTED) return rc;  // UNSUPPORTED = not this shape, fall through
  }
  // (the output is zeroed further down, once the launch geometry says whether it has to be at all)
  {
    const int rc = execute_table_columns(p, kn, in, out, accumulate, stream);
    if (rc != XHIST_ERR_UNSUPPORTED) return rc;
  }
  StreamChoice sc;
  if (int rc = choose_streaming(p, kn, in, sc)) return rc;
  if (two && !accumulate) {
    if (int zrc = zero_output(out, out_elems, stream)) return zrc;
    if (int zrc = zero_output(out2, out_elems, stream)) return zrc;
  }
  choose_slices(p, kn, in, sc);
  {
    const int rc = execute_partitioned_rows(p, kn, in, sc, out, accumulate, stream);
    if (rc != XHIST_ERR_UNSUPPORTED) return rc;
  }
  const StreamGeom g = streaming_geometry(p, kn, in, sc, accumulate);
  return launch_streaming(p, kn, in, sc, g, out, out2, accumulate, stream);
}
