// xhist_values.hip.h — what the per-bin statistics of a value array share: histogram_extrema and histogram_argextrema (xhist_extrema.hip.h), the
// quantiles (xhist_quantile.hip.h) and the moments (xhist_moments.hip.h: histogram_mean_var, histogram_cov and their weighted
// forms).  The one kernel skeleton per family, into which
// a statistic plugs an accumulator policy, and the one host-side launcher: the family and LDS rule, the launch geometry, the
// Params of a launch, and the one driver of the two-pass statistics (two_pass_run, at the end: mean_var, its weighted form, cov).
// The host functions take the record of the call (ValuesCall, xhist_values_api.h) and name only what differs per launch.
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  A counted sample whose
// value is not NaN hands that value to the policy.  The slots of a workgroup sit in LDS behind the staged tables; the generic
// family without LDS room hands every value straight to global memory.
//
// The weighted statistics (histogram_mean_var with weights, xhist_meanvar_w.hip) read a third stream, the weights, through the
// same skeletons: a policy with kExtra = 1 is handed (value, weight) pairs, and its kernels take WParams.
//
// The weighted statistic of two value arrays (histogram_weighted_cov, xhist_cov_w.hip) reads a fourth stream the same way: a
// policy with kExtra = 2 is handed (a, b, weight) triples, and its kernels take CovWParams.
//
// Nothing here instantiates a kernel: the skeletons are templates, and the kernels are instantiated in the statistic's own
// translation unit only.  The C ABI unit does not include this header: what it shares with the statistics' units (ValuesPlan,
// ValuesCall, the drivers' prototypes) is xhist_values_api.h, which holds no device code.
#pragma once

#include "xhist_kernels.hip.h"
#include "xhist_values_api.h"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace xhist {

// the slots sit behind the staged tables, 16-byte aligned
__host__ __device__ __forceinline__ size_t ext_slots_offset(const Params& p) { return (size_t)((p.table_words + 1) & ~1) * 8; }

// The Params of the weighted statistics' kernels: Params, whose fields do not move, and the weights, a third input stream laid
// out as the values are (x_ptr[row_offset(r, x_rs, x_ir, x_os) + c * x_cs], dtype x_dt).  Only the weighted kernels take it.
struct WParams : Params {
  const void* x_ptr;
  int64_t x_rs, x_cs, x_ir, x_os;
  int32_t x_dt;
};

// The Params of the statistics of two value arrays (histogram_cov, xhist_cov.hip.h): the second array travels as the weights
// do, and a pass writes more arrays than out / out2 name, so each of out, out2 and w2_ptr is a block of [n_rows, n_bins] planes
// `plane` 8-byte elements apart (launch_values_pass fills it).
struct CovParams : WParams {
  int64_t plane;
};

// The Params of the weighted statistics of two value arrays (histogram_weighted_cov, xhist_cov_w.hip.h): CovParams, whose x_*
// block is the second value array, and the weights, a fourth input stream laid out as the x_* block is.
struct CovWParams : CovParams {
  const void* y_ptr;
  int64_t y_rs, y_cs, y_ir, y_os;
  int32_t y_dt;
};

// The values of a call as a kernel outside the skeletons reads them (sort_keys, rank_heads): the call's xhist_array, advanced to
// no row.  Element (r, c) of a launch whose first row is `row0` is ptr[row_offset(row0 + r, rs, ir, os) + c * cs], dtype dt.
struct ValuesRead {
  const void* ptr;
  int64_t rs, cs, ir, os, row0;
  int32_t dt;
};
static inline ValuesRead values_read(const xhist_array& a, int64_t row0) {
  return ValuesRead{a.data, a.row_stride, a.col_stride, a.inner_rows, a.outer_stride, row0, a.dtype};
}

// An accumulator policy `Acc` is one statistic's (one pass's) use of the slots:
//   slot_t                    one bin's LDS slot
//   kCopies                   the fast family keeps 2^p.copies_log2 copies of every slot, lane i adding into copy
//                             i mod 2^copies_log2: bin b's copy c is slot (b << p.copies_log2) + c (the generic family: one)
//   init(slots, p, row)       the workgroup's slots, before the first sample
//   lds_add(slots, i, v)      one value into slot i: v in the sample type (fast family) or float64 (generic family)
//   global_add(p, row, b, v)  one float64 value straight into bin b of the output row (generic family without LDS)
//   flush(slots, p, row)      the workgroup's slots into its output row
//   kExtra                    the input streams it reads beyond the samples and the values: 0, 1 or 2
// Outputs are [n_rows, n_bins] arrays at p.out / p.out2, pre-advanced to row p.row0; the values are p.w_*.
// A policy of one extra stream (kExtra = 1; its kernels take WParams, the stream at p.x_*: the weights, or histogram_cov's
// second value array) takes that stream's element as well:
//   lds_add(slots, i, v, w)  global_add(p, row, b, v, w)   (w in the sample type or float64, as v)
// A policy of two extra streams (kExtra = 2; its kernels take CovWParams, the second value array at p.x_* and the weights at
// p.y_*) takes both:
//   lds_add(slots, i, a, b, w)  global_add(p, row, bin, a, b, w)
// A policy that declares kIndex = true (only with kExtra = 0: histogram_argextrema's second pass, xhist_extrema.hip.h) is handed
// the sample's column index inside its row as well, a uint64:
//   lds_add(slots, i, v, col)  global_add(p, row, bin, v, col)
// The skeletons choose the streams and the index at compile time (if constexpr).
//
// The bodies take the kernel's Params as `const Params& __restrict__`.  A body is optimised on its own before it is inlined
// into its kernel, and without __restrict__ that step must assume the LDS and global atomics may write the Params: the
// fast arithmetic-edge kernels then held up to 23 more VGPRs, and the generic ones spilled SGPRs to scratch.  With it the
// body compiles as if written in the kernel, where Params is a private copy nothing else writes.

// whether a policy asks for the sample's column index: its kIndex where it declares one, else no
template <class Acc, class = void>
struct acc_wants_index : std::false_type {};
template <class Acc>
struct acc_wants_index<Acc, std::void_t<decltype(Acc::kIndex)>> : std::integral_constant<bool, Acc::kIndex> {};

// ---------------------------------------------------------------------------------------------
// GENERIC family: any dtype per input and for the values, any element strides (broadcast and grouped rows), 1..8 inputs,
// compare domains 0 (float64), 1 (int64) and 3 (per input).  LDS: the slots of every bin in LDS behind the tables (which are
// then in LDS too).  Else every value goes to global memory, and the tables are read from LDS when they fit there
// (p.tables_in_lds) and through L2 otherwise.
// ---------------------------------------------------------------------------------------------
template <class Acc, int CMP, bool LDS, class P>
__device__ __forceinline__ void values_generic_body(const P& __restrict__ p) {
  constexpr bool W = Acc::kExtra >= 1, W2 = Acc::kExtra == 2;
  constexpr bool IDX = acc_wants_index<Acc>::value;
  static_assert(!IDX || !W, "the column index goes to policies without extra streams");
  static_assert(!W || std::is_base_of<WParams, P>::value, "a policy of an extra stream reads the x_* block of WParams");
  static_assert(!W2 || std::is_base_of<CovWParams, P>::value, "a policy of two extra streams reads the y_* block of CovWParams too");
  using CT = typename Dom<CMP>::T;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = p.tables_in_lds ? stage_tables(p) : p.tables;
  typename Acc::slot_t* slots = reinterpret_cast<typename Acc::slot_t*>(xhist_smem + ext_slots_offset(p));
  if (LDS) Acc::init(slots, p, row);
  __syncthreads();

  const int nd = p.n_dims;
  int64_t roff[kMaxDims];
#pragma unroll
  for (int d = 0; d < kMaxDims; ++d) roff[d] = d < nd ? row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]) : 0;
  const int64_t voff = row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);

  const int64_t stride = (int64_t)p.segs * blockDim.x;
  // The weight's element index walks with i, per lane: the weights then hold 5 SGPRs (pointer, dtype, step) instead of 7,
  // and the weighted kernels keep clear of scratch (with a row offset and a column stride live, two of them reserved 36 bytes).
  int64_t xi = 0, xstep = 0;
  if constexpr (W) {
    xi = row_offset(p.row0 + row, p.x_rs, p.x_ir, p.x_os) + ((int64_t)seg * blockDim.x + threadIdx.x) * p.x_cs;
    xstep = stride * p.x_cs;
  }
  // The fourth stream walks as a per-lane address in bytes: it then holds 3 SGPRs (dtype, step), and the kernels of two extra
  // streams keep clear of scratch too (walked by element index, covw_sum_generic<1, false> reserved 36 bytes).
  const char* yp = nullptr;
  int64_t ystep = 0;
  if constexpr (W2) {
    const int64_t eb = dt_size(p.y_dt);
    yp = static_cast<const char*>(p.y_ptr) +
         (row_offset(p.row0 + row, p.y_rs, p.y_ir, p.y_os) + ((int64_t)seg * blockDim.x + threadIdx.x) * p.y_cs) * eb;
    ystep = stride * p.y_cs * eb;
  }
  for (int64_t i = (int64_t)seg * blockDim.x + threadIdx.x; i < p.n_cols; i += stride, xi += xstep) {
    const char* const ycur = yp;  // (this sample's weight; the address moves on here, ahead of the `continue` below)
    if constexpr (W2) yp += ystep;
    const double v = load_as<double>(p.w_ptr, p.w_dt, voff + i * p.w_cs);
    bool ok = v == v;  // NaN values are ignored (np.fmin / np.fmax, np.nanmean / np.nanvar)
    int64_t flat = 0;
#pragma unroll
    for (int d = 0; d < kMaxDims; ++d) {
      if (d < nd) {
        const CT x = load_dom<CMP>(p.s_ptr[d], p.s_dt[d], roff[d] + i * p.s_cs[d], p.dim[d]);
        const int b = digitize<CMP>(x, p.dim[d], tab);
        ok &= (b >= 0);
        flat += (int64_t)b * p.dim[d].out_stride;
      }
    }
    if (!ok) continue;
    if constexpr (W2) {
      const double b = load_as<double>(p.x_ptr, p.x_dt, xi);  // (both only for a sample that counts)
      const double w = load_as<double>(ycur, p.y_dt, 0);
      if (LDS) Acc::lds_add(slots, (uint32_t)flat, v, b, w);
      else Acc::global_add(p, row, flat, v, b, w);
    } else if constexpr (W) {
      const double w = load_as<double>(p.x_ptr, p.x_dt, xi);  // (only for a sample that counts)
      if (LDS) Acc::lds_add(slots, (uint32_t)flat, v, w);
      else Acc::global_add(p, row, flat, v, w);
    } else if constexpr (IDX) {
      if (LDS) Acc::lds_add(slots, (uint32_t)flat, v, (uint64_t)i);
      else Acc::global_add(p, row, flat, v, (uint64_t)i);
    } else {
      if (LDS) Acc::lds_add(slots, (uint32_t)flat, v);  // (one copy of the slots: p.copies_log2 == 0)
      else Acc::global_add(p, row, flat, v);
    }
  }
  if (LDS) {
    __syncthreads();
    Acc::flush(slots, p, row);
  }
}

// ---------------------------------------------------------------------------------------------
// VECTOR fast path: float32 or float64 samples with values of the same type, unit column stride, one or two inputs, slots
// in LDS; digitize by the tables with at most two edges per bucket (SCAN 1 / 2: float64 edges for float64 samples, float32
// thresholds for float32 ones) or by arithmetic (kScanArith).  Tiles as in hist_fast: VEC elements per 16-byte
// non-temporal load, UNROLL loads in flight per array and lane; the workgroups of a row walk its tiles interleaved.  A weighted
// policy's weights have the sample type and unit column stride too, and are loaded the same way; so is the fourth stream of a
// policy of two extra streams.
// ---------------------------------------------------------------------------------------------
// the parts a fast form reads its tile in: the fewest (a power of two, at most one load per array and part) that keep `limit`
// bytes per lane in flight
constexpr int fast_halves(int tile_bytes, int limit, int unroll) {
  int h = 1;
  while (tile_bytes / h > limit && h < unroll) h *= 2;
  return h;
}

template <class Acc, typename ST, int D, int SCAN, class P>
__device__ __forceinline__ void values_fast_body(const P& __restrict__ p) {
  constexpr bool W = Acc::kExtra >= 1, W2 = Acc::kExtra == 2;
  constexpr bool IDX = acc_wants_index<Acc>::value;
  static_assert(!IDX || !W, "the column index goes to policies without extra streams");
  static_assert(!W || std::is_base_of<WParams, P>::value, "a policy of an extra stream reads the x_* block of WParams");
  static_assert(!W2 || std::is_base_of<CovWParams, P>::value, "a policy of two extra streams reads the y_* block of CovWParams too");
  static_assert(__is_same(ST, double) || __is_same(ST, float), "float32 / float64 samples and values");
  static_assert(SCAN == 1 || SCAN == 2 || SCAN == kScanArith, "tables with <= 2 edges per bucket, or arithmetic edges");
  constexpr int CMP = (__is_same(ST, float) && SCAN != kScanArith) ? 2 : 0;
  constexpr int VEC = 16 / (int)sizeof(ST);
  constexpr int UNROLL = D == 1 ? 4 : 8 / VEC;  // 128 bytes of samples and values per lane in flight (192 for two inputs)
  // A form reads STREAMS arrays (D inputs, the values, the weights or second values, the fourth stream) of 16 * UNROLL bytes per
  // lane and tile each, and reads its tile in HALVES parts of UNROLL / HALVES loads per array (fast_halves).  The tile, and with
  // it the launch geometry, stays.  No form keeps more than 192 bytes per lane in flight, what three streams of 64 bytes hold:
  // weighted float64 pairs would keep 256, and in two halves they keep the VGPRs, hence the waves per SIMD, of the unweighted
  // form.  The same rule serves the forms with a fourth stream: their single inputs read two halves (128 bytes), float64 pairs
  // two halves and float32 pairs the whole tile (160 bytes).  Six of the pair kernels then have three waves per SIMD where
  // their histogram_cov twins have four; splitting further to keep the wave was measured and is slower.
  //   streams   form                                    whole tile   HALVES   in flight per lane
  //   2         single input                                  128        1         128
  //   3         single input, weighted or two values          192        1         192
  //   3         float64 pairs                                 192        1         192
  //   3         float32 pairs                                  96        1          96
  //   4         float64 pairs, weighted or two values         256        2         128
  //   4         float32 pairs, weighted or two values         128        1         128
  //   4         single input, two values and weights          256        2         128   (float64 and float32)
  //   5         float64 pairs, two values and weights         320        2         160
  //   5         float32 pairs, two values and weights         160        1         160
  constexpr int STREAMS = D + 1 + (W ? 1 : 0) + (W2 ? 1 : 0);
  constexpr int HALVES = fast_halves(STREAMS * 16 * UNROLL, 192, UNROLL);
  static_assert(W2 || HALVES == ((W && D == 2 && __is_same(ST, double)) ? 2 : 1), "the forms of up to four streams keep their halves");
  constexpr int UH = UNROLL / HALVES;
  using svec = typename VecOf<ST, VEC>::type;

  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = stage_tables(p);
  typename Acc::slot_t* slots = reinterpret_cast<typename Acc::slot_t*>(xhist_smem + ext_slots_offset(p));
  Acc::init(slots, p, row);
  __syncthreads();

  const ST* sp[D];
#pragma unroll
  for (int d = 0; d < D; ++d) sp[d] = reinterpret_cast<const ST*>(p.s_ptr[d]) + row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]);
  const ST* vp = reinterpret_cast<const ST*>(p.w_ptr) + row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);
  const ST* xp = nullptr;
  if constexpr (W) xp = reinterpret_cast<const ST*>(p.x_ptr) + row_offset(p.row0 + row, p.x_rs, p.x_ir, p.x_os);
  const ST* yp = nullptr;
  if constexpr (W2) yp = reinterpret_cast<const ST*>(p.y_ptr) + row_offset(p.row0 + row, p.y_rs, p.y_ir, p.y_os);
  const uint32_t nb1 = D == 2 ? (uint32_t)p.dim[1].nb : 1u;
  const uint32_t mycopy = Acc::kCopies ? (uint32_t)tid & ((1u << p.copies_log2) - 1u) : 0u;

  const int64_t tile_elems = (int64_t)blockDim.x * VEC * UNROLL;
  const int64_t n_tiles = (p.n_cols + tile_elems - 1) / tile_elems;
  for (int64_t t = seg; t < n_tiles; t += p.segs) {
    const int64_t base = t * tile_elems;
    const bool full = base + tile_elems <= p.n_cols;
#pragma unroll
    for (int h = 0; h < HALVES; ++h) {
      svec xv[D][UH], vv[UH], wv[W ? UH : 1], yv[W2 ? UH : 1];
      if (full) {
#pragma unroll
        for (int u = 0; u < UH; ++u) {
          const int64_t i = base + ((int64_t)(h * UH + u) * blockDim.x + tid) * VEC;
#pragma unroll
          for (int d = 0; d < D; ++d) xv[d][u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(sp[d] + i));
          vv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(vp + i));
          if constexpr (W) wv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(xp + i));
          if constexpr (W2) yv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(yp + i));
        }
      } else {  // the ragged last tile: positions past the end become NaN samples, which digitize drops (their weights are 0)
#pragma unroll
        for (int u = 0; u < UH; ++u) {
          const int64_t i = base + ((int64_t)(h * UH + u) * blockDim.x + tid) * VEC;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const bool in = i + v < p.n_cols;
#pragma unroll
            for (int d = 0; d < D; ++d) xv[d][u][v] = in ? sp[d][i + v] : (ST)__builtin_nanf("");
            vv[u][v] = in ? vp[i + v] : (ST)__builtin_nanf("");
            if constexpr (W) wv[u][v] = in ? xp[i + v] : (ST)0;
            if constexpr (W2) yv[u][v] = in ? yp[i + v] : (ST)0;
          }
        }
      }
      uint32_t cnt[D][UH][VEC];
      count_le_tile<CMP, SCAN, D, UH, VEC>(xv, p, tab, 1, cnt);
#pragma unroll
      for (int u = 0; u < UH; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const ST val = vv[u][v];
          bool ok = val == val;
          uint32_t flat = 0;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const int b = bin_from_tile_count<CMP, SCAN>((typename Dom<CMP>::T)xv[d][u][v], p.dim[d], cnt[d][u][v]);
            ok &= b >= 0;
            flat = d == 0 ? (uint32_t)b : flat * nb1 + (uint32_t)b;
          }
          if constexpr (W2) {
            if (ok) Acc::lds_add(slots, Acc::kCopies ? (flat << p.copies_log2) + mycopy : flat, val, (ST)wv[u][v], (ST)yv[u][v]);
          } else if constexpr (W) {
            if (ok) Acc::lds_add(slots, Acc::kCopies ? (flat << p.copies_log2) + mycopy : flat, val, (ST)wv[u][v]);
          } else if constexpr (IDX) {
            if (ok)
              Acc::lds_add(slots, Acc::kCopies ? (flat << p.copies_log2) + mycopy : flat, val,
                           (uint64_t)(base + ((int64_t)(h * UH + u) * blockDim.x + tid) * VEC + v));
          } else {
            if (ok) Acc::lds_add(slots, Acc::kCopies ? (flat << p.copies_log2) + mycopy : flat, val);
          }
        }
    }
  }
  __syncthreads();
  Acc::flush(slots, p, row);
}

}  // namespace xhist

// ---- host side (the plan's view and the call's record: xhist_values_api.h) -----------------------------------------------------
namespace xhist {

typedef void (*values_fn)(const Params);

// every kernel of a statistic goes through the census log of the dispatch surface (XH_LAUNCH_PICKED of
// xhist_host_common.hip.h, whose logger lives in xhist_capi.hip)
#define XH_VALUES_LAUNCH(fn, ...)                               \
  do {                                                          \
    xhist_log_picked_kernel(reinterpret_cast<const void*>(fn)); \
    hipLaunchKernelGGL(fn, __VA_ARGS__);                        \
  } while (0)

static inline int values_error(const ValuesCall& k, const char* what, hipError_t e) {
  return k.fail(XHIST_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// after a launch of call `k`: a failed one ends the driver with `what` and HIP's text in k.err
#define XH_VALUES_LAUNCH_CHECK(k, what)                          \
  do {                                                           \
    hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return values_error(k, what, e_);      \
  } while (0)

static inline int elem_bytes(int dt) {
  return (dt == XHIST_F64 || dt == XHIST_I64 || dt == XHIST_U64) ? 8 : (dt == XHIST_F32 || dt == XHIST_I32 || dt == XHIST_U32) ? 4
       : (dt == XHIST_F16 || dt == XHIST_I16 || dt == XHIST_U16) ? 2 : 1;
}

// A statistic's LDS slots, for the family rule: the bytes of a bin's slot in each of its passes (0: no second pass), the
// same for the fast family on float32 values, and whether the fast family keeps copies of its slots.
struct ValuesSlots {
  size_t bytes[2], fast32[2];
  bool copies;
};

// What the binning launches run and where their slots live.
struct ValuesChoice {
  bool fast = false, lds = false, tables_in_lds = false, f32 = false;
  int scan = 0, copies_log2 = 0;
  const ValuesTables* tab = nullptr;
  int32_t table_words = 0;
  size_t lds_bytes[2] = {0, 0};  // per pass
};

// Copies of the fast family's slots: the most (up to 16) whose largest slots stay within 24 KiB, so that a CU still holds
// several workgroups.  mean_var: C2's 100 bins get 8, C4's 50 get 16; above 1024 bins there is one.
static inline int fast_copies_log2(int64_t n_bins, size_t slot, size_t tbytes, size_t lds_max) {
  int cl = 0;
  while (cl < 4 && ((size_t)n_bins * slot << (cl + 1)) <= 24 * 1024 && tbytes + ((size_t)n_bins * slot << (cl + 1)) <= lds_max) ++cl;
  return cl;
}

// fast if eligible, else generic with its slots in LDS, else generic straight into global memory.  The largest slot of the
// passes decides; every pass takes the family, the home and the copies chosen for it.  The call's third stream (nullptr: none)
// must qualify for the fast family as the values do: the sample dtype, unit column stride (or one column), element-aligned; so
// must its fourth, and either alone sends the call to the generic family.  A call without values (k.values == nullptr: the maps
// of xhist_map.hip that read the samples alone) is judged by its samples.
static inline ValuesChoice choose_values(const ValuesCall& k, const ValuesSlots& sl) {
  const ValuesPlan& pl = k.pl;
  const xhist_array *samples = k.samples, *values = k.values;
  const int64_t n_cols = k.n_cols;
  ValuesChoice c;
  const int D = pl.n_dims;
  const int sdt = samples[0].dtype;
  c.f32 = sdt == XHIST_F32;
  bool fast_ok = pl.cmp == XHIST_CMP_F64 && D <= 2 && (sdt == XHIST_F64 || sdt == XHIST_F32) && (!values || values->dtype == sdt) &&
                 pl.n_bins < ((int64_t)1 << 24);
  for (int d = 0; d < D && fast_ok; ++d)
    fast_ok = samples[d].dtype == sdt && (samples[d].col_stride == 1 || n_cols == 1) && (uintptr_t)samples[d].data % (size_t)elem_bytes(sdt) == 0;
  if (fast_ok && values) fast_ok = (values->col_stride == 1 || n_cols == 1) && (uintptr_t)values->data % (size_t)elem_bytes(sdt) == 0;
  for (const xhist_array* x : {k.third, k.fourth})
    if (fast_ok && x) fast_ok = x->dtype == sdt && (x->col_stride == 1 || n_cols == 1) && (uintptr_t)x->data % (size_t)elem_bytes(sdt) == 0;
  if (fast_ok) {
    const size_t* bytes = c.f32 ? sl.fast32 : sl.bytes;
    const size_t slot = std::max(bytes[0], bytes[1]);
    const size_t slots = (size_t)pl.n_bins * slot;
    const ValuesTables& fine = c.f32 ? pl.fine32 : pl.fine64;
    const size_t fine_tbytes = ((size_t)fine.words + 1) / 2 * 16;
    size_t tbytes = 0;
    if (fine.blob && fine.max_cnt >= 1 && fine.max_cnt <= 2 && fine_tbytes + slots <= pl.lds_max) {
      c.scan = fine.max_cnt;
      c.tab = &fine;
      c.table_words = fine.words;
      tbytes = fine_tbytes;
    } else if (pl.arith && slots <= pl.lds_max) {
      c.scan = kScanArith;
      c.tab = &pl.native;  // (the float64-domain DimTable carries e_0, e_last and the step; no table is read)
      c.table_words = 0;
    }
    if (c.tab) {
      c.copies_log2 = sl.copies ? fast_copies_log2(pl.n_bins, slot, tbytes, pl.lds_max) : 0;
      for (int k = 0; k < 2; ++k) c.lds_bytes[k] = bytes[k] ? tbytes + ((size_t)pl.n_bins * bytes[k] << c.copies_log2) : 0;
      c.fast = c.lds = c.tables_in_lds = true;
      return c;
    }
  }
  c.tab = &pl.native;
  const size_t tbytes = ((size_t)pl.native.words + 1) / 2 * 16;
  c.tables_in_lds = tbytes + 1024 <= pl.lds_max;
  c.table_words = c.tables_in_lds ? pl.native.words : 0;
  c.lds = c.tables_in_lds && pl.n_bins < ((int64_t)1 << 24) &&
          tbytes + (size_t)pl.n_bins * std::max(sl.bytes[0], sl.bytes[1]) <= pl.lds_max;
  for (int k = 0; k < 2; ++k)
    c.lds_bytes[k] = c.tables_in_lds && sl.bytes[k] ? tbytes + (c.lds ? (size_t)pl.n_bins * sl.bytes[k] : 0) : 0;
  return c;
}

// The kernel a choice runs, from a statistic's kernel set K: K::fast<ST, D, SCAN>() and K::generic<CMP, LDS>() name its
// instantiations (values_fn, or the WParams form of the weighted kernels).  nullptr: none for this combination.
template <class K>
using values_fn_of = decltype(K::template generic<0, true>());

template <class K, typename ST, int D>
static values_fn_of<K> fast_scan(int scan) {
  if (scan == 1) return K::template fast<ST, D, 1>();
  if (scan == 2) return K::template fast<ST, D, 2>();
  if (scan == kScanArith) return K::template fast<ST, D, kScanArith>();
  return nullptr;
}
// the compare domain of the generic family's kernels for a plan (0 float64, 1 int64, 3 per input), as describe() names it
static inline int values_cmp(const ValuesPlan& pl) { return pl.cmp == XHIST_CMP_F64 ? 0 : pl.cmp == XHIST_CMP_I64 ? 1 : 3; }

template <class K>
static values_fn_of<K> pick_values_kernel(const ValuesChoice& c, const ValuesPlan& pl) {
  if (c.fast) {
    if (c.f32) return pl.n_dims == 1 ? fast_scan<K, float, 1>(c.scan) : fast_scan<K, float, 2>(c.scan);
    return pl.n_dims == 1 ? fast_scan<K, double, 1>(c.scan) : fast_scan<K, double, 2>(c.scan);
  }
  // (the domain as the histogram's generic family reads it: exactly float64, exactly int64, else per input)
  if (pl.cmp == XHIST_CMP_F64) return c.lds ? K::template generic<0, true>() : K::template generic<0, false>();
  if (pl.cmp == XHIST_CMP_I64) return c.lds ? K::template generic<1, true>() : K::template generic<1, false>();
  return c.lds ? K::template generic<3, true>() : K::template generic<3, false>();
}

// Launch geometry, the same for every pass: every resident workgroup at once, the workgroups of a row walking its tiles
// interleaved; the largest pass's LDS footprint sets the residency.
struct ValuesGeometry {
  int block = 0;
  int64_t segs = 0, max_rows = 0;
};
static inline ValuesGeometry values_geometry(const ValuesPlan& pl, const ValuesChoice& c, int64_t n_rows, int64_t n_cols) {
  ValuesGeometry g;
  g.block = c.fast ? 256 : 512;
  const int vec = c.f32 ? 4 : 2;
  const int64_t per_tile = c.fast ? (int64_t)g.block * (pl.n_dims == 1 ? 4 * vec : 8) : g.block;  // (fast body: VEC x UNROLL per lane)
  const size_t lds = std::max(c.lds_bytes[0], c.lds_bytes[1]);
  int bpc = 2048 / g.block;
  if (lds) bpc = (int)std::max<size_t>(1, std::min<size_t>((size_t)bpc, 160 * 1024 / lds));
  const int64_t target = (int64_t)pl.cus * bpc;
  const int64_t tiles = (n_cols + per_tile - 1) / per_tile;
  g.segs = std::max<int64_t>(1, std::min<int64_t>(tiles, (target + n_rows - 1) / n_rows));
  // A workgroup sees fewer than 2^31 samples, so uint32 counts in its slots cannot wrap.  Only mean_var counts; for extrema the
  // guard changes only the grid (and describe()'s segs), never the result.  It moves segs for rows longer than 2^31 samples
  // once the rows alone fill the device (n_rows >= cus * bpc, segs 1), e.g. rows broadcast at row stride 0.
  g.segs = std::max<int64_t>(g.segs, (tiles * per_tile + ((int64_t)1 << 31) - 1) >> 31);
  // A launch's grid counts its work-items in 32 bits: a grid of 2^31 - 1 workgroups of 256 lanes wraps to 2^24 - 1 of them, and
  // the rows past those were never binned.  So a chunk of rows keeps both the workgroups below 2^31 and the lanes below 2^32.
  g.max_rows = std::min<int64_t>(((int64_t)1 << 31) - 1, (((int64_t)1 << 32) - 1) / g.block) / g.segs;
  return g;
}

// A kernel's dynamic LDS beyond 48 KiB must be allowed before its first launch; drivers do it for every pass up front.
template <class F>
static int allow_values_lds(const ValuesCall& k, F fn, size_t lds, const char* what) {
  if (lds <= 48 * 1024) return XHIST_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return e == hipSuccess ? XHIST_OK : values_error(k, what, e);
}

// The Params of a launch over rows [r0, r0 + nr) of the call's inputs: samples, values, tables and geometry; the outputs (out,
// out2, w2_ptr) are the caller's to set.
static inline Params values_params(const ValuesCall& k, const ValuesChoice& c, int64_t segs, int64_t r0, int64_t nr) {
  const ValuesPlan& pl = k.pl;
  const xhist_array *samples = k.samples, *values = k.values;
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
  if (values) {  // (a call without values leaves the block zeroed: its kernels read none)
    kp.w_ptr = values->data;
    kp.w_rs = values->row_stride;
    kp.w_cs = values->col_stride;
    kp.w_ir = values->inner_rows;
    kp.w_os = values->outer_stride;
    kp.w_dt = values->dtype;
  }
  kp.row0 = r0;
  kp.n_dims = pl.n_dims;
  kp.tables = c.tab->blob;
  kp.table_words = c.table_words;
  kp.tables_in_lds = c.tables_in_lds ? 1 : 0;
  kp.n_rows = nr;
  kp.n_cols = k.n_cols;
  kp.n_bins = pl.n_bins;
  kp.segs = (int32_t)segs;
  kp.copies_log2 = c.copies_log2;
  return kp;
}

// the weights of a WParams launch over rows from r0 on
static inline void weights_params(WParams& kp, const xhist_array* weights) {
  kp.x_ptr = weights->data;
  kp.x_rs = weights->row_stride;
  kp.x_cs = weights->col_stride;
  kp.x_ir = weights->inner_rows;
  kp.x_os = weights->outer_stride;
  kp.x_dt = weights->dtype;
}
// ... and the fourth stream of a CovWParams launch
static inline void weights_params(CovWParams& kp, const xhist_array* third, const xhist_array* fourth) {
  weights_params(kp, third);
  kp.y_ptr = fourth->data;
  kp.y_rs = fourth->row_stride;
  kp.y_cs = fourth->col_stride;
  kp.y_ir = fourth->inner_rows;
  kp.y_os = fourth->outer_stride;
  kp.y_dt = fourth->dtype;
}

// One binning pass: the launches of row chunks of at most g.max_rows (the grid stays below 2^31 workgroups and 2^32 lanes).  out / out2 / in2 are [n_rows, n_bins] arrays of 8-byte elements,
// advanced to each chunk's first row (Params::out, out2 and w2_ptr); `what` names the pass in error messages.  A weighted
// kernel (it takes WParams) reads the call's third stream; for a CovParams kernel each of the three is the first of several
// such arrays, n_rows * n_bins elements apart; a CovWParams kernel reads the fourth stream as well.
template <class P>
static int launch_values_pass(void (*fn)(const P), size_t lds, const char* what, const ValuesCall& k, const ValuesChoice& c,
                              const ValuesGeometry& g, void* out, void* out2, const void* in2) {
  const int64_t n_bins = k.pl.n_bins;
  for (int64_t r0 = 0; r0 < k.n_rows; r0 += g.max_rows) {
    const int64_t nr = std::min(g.max_rows, k.n_rows - r0);
    P kp;
    static_cast<Params&>(kp) = values_params(k, c, g.segs, r0, nr);
    if constexpr (std::is_base_of<CovWParams, P>::value) weights_params(kp, k.third, k.fourth);
    else if constexpr (std::is_base_of<WParams, P>::value) {
      static const xhist_array no_stream = {};  // (a CovParams kernel of one value array without weights reads no x_* stream)
      weights_params(kp, k.third ? k.third : &no_stream);
    }
    if constexpr (std::is_base_of<CovParams, P>::value) kp.plane = k.n_rows * n_bins;  // (the whole call's rows, whatever the chunk)
    kp.w2_ptr = in2 ? static_cast<const uint64_t*>(in2) + r0 * n_bins : nullptr;
    kp.out = static_cast<uint64_t*>(out) + r0 * n_bins;
    kp.out2 = static_cast<uint64_t*>(out2) + r0 * n_bins;
    XH_VALUES_LAUNCH(fn, dim3((unsigned)(nr * g.segs)), dim3(g.block), lds, k.stream, kp);
    XH_VALUES_LAUNCH_CHECK(k, what);
  }
  return XHIST_OK;
}

// the prefix of a two-pass statistic's pass-1 kernels: M::sum_prefix where it names one, else M::prefix (see two_pass_run)
template <class M, class = void>
struct sum_prefix_of {
  static constexpr const char* value = M::prefix;
};
template <class M>
struct sum_prefix_of<M, std::void_t<decltype(M::sum_prefix)>> {
  static constexpr const char* value = M::sum_prefix;
};

// The driver of the two-pass statistics: the scratch block, the zeroing and the five launches on the call's stream (pass 1,
// means, pass 2, finalize).  M names what a statistic brings (xhist_meanvar.hip: MeanVar, xhist_meanvar_w.hip: MeanVarW,
// xhist_cov.hip: Cov, xhist_cov_w.hip: CovW; SkewKurt and SkewKurtW, next to MeanVar and MeanVarW, whose pass 1 they run):
//   Sum, Dev          the kernel sets of the two passes, for pick_values_kernel (each with the Params type of its own kernels)
//   mean, finalize    the kernels of the steps after them, over the first output (counts or sums of weights)
//   slots             the ValuesSlots of the two passes
//   planes            the [n_rows, n_bins] planes behind first, out_mean, out_m2 and sd, in this order (cov: 1, 2, 3, 2)
//   name, prefix      the statistic in messages and in describe() (mean_var / mean_var_w / cov), and its kernels' prefix
//   sum_prefix        (optional) the prefix of pass 1's kernels and of the means' step where they are another statistic's:
//                     skew_kurt runs mean_var's (mv_sum_*, then sk_dev_*), and the passes' kernels then take different Params
//   spelled           the statistic where a message spells it out ("weighted mean_var")
// `first` is out_count or out_wsum; the call's third stream the weights or the second value array, its fourth the weights of a
// statistic of two value arrays.  sd, the sums of deviations between the passes, is the driver's own: planes[3] planes from the
// call's allocator, the very count it zeroes.
template <class M, class First>
static int two_pass_run(const ValuesCall& k, First* first, double* out_mean, double* out_m2) {
  const ValuesPlan& pl = k.pl;
  const int64_t n_out = k.n_rows * pl.n_bins;
  double* const sd = static_cast<double*>(k.scratch((size_t)(M::planes[3] * n_out) * sizeof(double)));
  if (!sd) return k.fail(XHIST_ERR_NOMEM, "allocation of the %s scratch block%s failed", M::spelled, M::planes[3] > 1 ? "s" : "");
  char buf[48];
  auto what = [&](const char* a, const char* b) {  // "<a><b> launch": only XH_VALUES_LAUNCH_CHECK calls it, after a failed launch
    snprintf(buf, sizeof buf, "%s%s launch", a, b);
    return buf;
  };
  char lds_what[64], sum_what[32], dev_what[32];  // (handed over before anything can fail, so made up front)
  snprintf(lds_what, sizeof lds_what, "%s: setting the dynamic LDS size failed", M::name);
  const char* const prefix1 = sum_prefix_of<M>::value;
  snprintf(sum_what, sizeof sum_what, "%s_sum launch", prefix1);
  snprintf(dev_what, sizeof dev_what, "%s_dev launch", M::prefix);
  const auto mean = M::mean;
  const auto finalize = M::finalize;
  const int grid_io = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_out + 255) / 256));
  void* const zero[4] = {first, out_mean, out_m2, sd};
  for (int i = 0; i < 4; ++i) {
    XH_LAUNCH_LOGGED_LOCAL(zero_words, dim3(grid_io), dim3(256), 0, k.stream, static_cast<unsigned long long*>(zero[i]), M::planes[i] * n_out);
    XH_VALUES_LAUNCH_CHECK(k, what(M::name, " zeroing"));
  }

  ValuesChoice c;
  ValuesGeometry g;
  values_fn_of<typename M::Sum> sum = nullptr;
  values_fn_of<typename M::Dev> dev = nullptr;
  if (k.n_cols > 0) {
    c = choose_values(k, M::slots);
    sum = pick_values_kernel<typename M::Sum>(c, pl);
    dev = pick_values_kernel<typename M::Dev>(c, pl);
    if (!sum || !dev) return k.fail(XHIST_ERR_HIP, "internal: no %s kernel for this combination", M::spelled);
    if (int rc = allow_values_lds(k, sum, c.lds_bytes[0], lds_what)) return rc;
    if (int rc = allow_values_lds(k, dev, c.lds_bytes[1], lds_what)) return rc;
    g = values_geometry(pl, c, k.n_rows, k.n_cols);
    if (int rc = launch_values_pass(sum, c.lds_bytes[0], sum_what, k, c, g, first, out_mean, nullptr)) return rc;
  }
  XH_VALUES_LAUNCH(mean, dim3(grid_io), dim3(256), 0, k.stream, first, out_mean, n_out);
  XH_VALUES_LAUNCH_CHECK(k, what(prefix1, "_mean"));
  if (k.n_cols > 0) {
    if (int rc = launch_values_pass(dev, c.lds_bytes[1], dev_what, k, c, g, sd, out_m2, out_mean)) return rc;
  }
  XH_VALUES_LAUNCH(finalize, dim3(grid_io), dim3(256), 0, k.stream, first, sd, out_m2, n_out);
  XH_VALUES_LAUNCH_CHECK(k, what(M::prefix, "_finalize"));
  const char* fam = !sum ? "none" : c.fast ? "fast" : "generic";
  const char* home = !sum ? "none" : c.lds ? "lds" : "global";
  k.describe("%s pass1=%s_sum_%s slots=%s pass2=%s_dev_%s slots=%s scan=%d copies=%d block=%d segs=%lld lds_bytes=%zu/%zu "
             "tables_in_lds=%d D=%d cmp=%d",
             M::name, prefix1, fam, home, M::prefix, fam, home, c.scan, 1 << c.copies_log2, g.block, (long long)g.segs, c.lds_bytes[0],
             c.lds_bytes[1], (int)c.tables_in_lds, pl.n_dims, values_cmp(pl));
  return XHIST_OK;
}

}  // namespace xhist
