// xhist_map.hip.h — the per-sample maps (bin_index, histogram_lookup, histogram_anomaly): the gather direction of the per-bin
// statistics.  Every other kernel of the library reduces samples into bins; these write one 8-byte element per sample, into a
// dense row-major [n_rows, n_cols] block:
//   kMapIndex     int64: the C-order flat index of the sample's bin, -1 for a sample the histogram does not count
//   kMapTake      float64: centre[row, bin], NaN for a sample that is not counted
//   kMapAnomaly   float64: float64(v) - centre[row, bin], divided by scale[row, bin] where a scale table is given (one IEEE
//                 subtraction, one IEEE division); NaN for a sample that is not counted, and a NaN value stays NaN
// Which samples count is decided exactly as for the histogram: the same loads, the same digitize (count_le_tile / digitize),
// the same tables, the same (row, seg) grid with interleaved tiles as the bodies of xhist_values.hip.h.  There is no
// accumulation and no flush: every output element is written exactly once, by the lane that read its sample.
//
// The float64 table row of the workgroup's row (and the scale row behind it) is staged in LDS behind the digitize tables and
// read per sample; the generic family reads it through L2 from global memory where it does not fit (table home "global").
// Whether a scale table is present is a kernel-uniform parameter, not a template axis.
//
// Nothing here instantiates a kernel: xhist_map.hip does.
#pragma once

#include "xhist_values.hip.h"

namespace xhist {

constexpr int kMapIndex = XHIST_MAP_INDEX, kMapTake = XHIST_MAP_TAKE, kMapAnomaly = XHIST_MAP_ANOMALY;

// Params, whose fields do not move (the values of kMapAnomaly travel as w_*; out is the output block, pre-advanced to the
// launch's first row), and the tables: [n_rows, n_bins] float64, pre-advanced to the launch's first row as well.
struct MapParams : Params {
  const double* centre;
  const double* scale;  // nullptr: none
};

// two 8-byte results side by side: one 16-byte store.  The block is dense, so a row starts wherever the rows before it end:
// 8-byte alignment is all a pair can count on (gfx950's global stores need dword alignment only).
typedef uint64_t map_pair __attribute__((ext_vector_type(2), aligned(8)));

constexpr uint64_t kMapNaN = 0x7ff8000000000000ull;  // what a sample that is not counted reads as: the quiet NaN of np.nan

// one sample's 8 bytes: `ok` whether it counts, `flat` its bin (any value where !ok), `v` its value (kMapAnomaly only);
// centre / scale: the row's tables, in LDS or in global memory
template <int OP, typename IT>
__device__ __forceinline__ uint64_t map_result(bool ok, IT flat, double v, const double* centre, const double* scale) {
  if constexpr (OP == kMapIndex) {
    return ok ? (uint64_t)flat : ~0ull;
  } else {
    const IT at = ok ? flat : (IT)0;  // (a bin of the row whatever the sample: no read outside the table)
    double r = centre[at];
    if constexpr (OP == kMapAnomaly) {
      r = v - r;
      if (scale) r = r / scale[at];
    }
    return ok ? __builtin_bit_cast(uint64_t, r) : kMapNaN;
  }
}

// the workgroup's table row(s) into LDS behind the digitize tables; returns the centre row (the scale row: n_bins on)
__device__ __forceinline__ double* map_stage_rows(const MapParams& p, int64_t row) {
  double* dst = reinterpret_cast<double*>(xhist_smem + ext_slots_offset(p));
  const double* c = p.centre + row * p.n_bins;
  for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) dst[b] = c[b];
  if (p.scale) {
    const double* s = p.scale + row * p.n_bins;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) dst[p.n_bins + b] = s[b];
  }
  return dst;
}

// ---------------------------------------------------------------------------------------------
// GENERIC family: any dtype per input and for the values, any element strides, 1..8 inputs, compare domains 0 / 1 / 3.
// TLDS: the table row(s) in LDS behind the digitize tables (which are then in LDS too); else they are read from global memory,
// and the digitize tables from LDS when they fit there (p.tables_in_lds) and through L2 otherwise.  kMapIndex has no table.
// ---------------------------------------------------------------------------------------------
template <int OP, int CMP, bool TLDS>
__device__ __forceinline__ void map_generic_body(const MapParams& __restrict__ p) {
  static_assert(OP != kMapIndex || !TLDS, "bin_index reads no table");
  using CT = typename Dom<CMP>::T;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = p.tables_in_lds ? stage_tables(p) : p.tables;
  const double* centre = nullptr;
  const double* scale = nullptr;
  if constexpr (OP != kMapIndex) {
    if constexpr (TLDS) {
      centre = map_stage_rows(p, row);
      scale = p.scale ? centre + p.n_bins : nullptr;
    } else {
      centre = p.centre + row * p.n_bins;
      scale = p.scale ? p.scale + row * p.n_bins : nullptr;
    }
  }
  __syncthreads();

  const int nd = p.n_dims;
  int64_t roff[kMaxDims];
#pragma unroll
  for (int d = 0; d < kMaxDims; ++d) roff[d] = d < nd ? row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]) : 0;
  uint64_t* out = reinterpret_cast<uint64_t*>(p.out) + row * p.n_cols;

  const int64_t stride = (int64_t)p.segs * blockDim.x;
  // The value's element index walks with i, per lane, as the weights' does in values_generic_body: row offset and column stride
  // then leave the SGPRs before the loop (with both live, map_generic<anomaly, 0, false> reserved 36 bytes of scratch).
  int64_t vi = 0, vstep = 0;
  if constexpr (OP == kMapAnomaly) {
    vi = row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os) + ((int64_t)seg * blockDim.x + threadIdx.x) * p.w_cs;
    vstep = stride * p.w_cs;
  }
  for (int64_t i = (int64_t)seg * blockDim.x + threadIdx.x; i < p.n_cols; i += stride, vi += vstep) {
    double v = 0.0;
    if constexpr (OP == kMapAnomaly) v = load_as<double>(p.w_ptr, p.w_dt, vi);
    bool ok = true;
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
    out[i] = map_result<OP>(ok, flat, v, centre, scale);  // (a 64-bit bin: the joint bins of up to 8 inputs may pass 2^32)
  }
}

// ---------------------------------------------------------------------------------------------
// VECTOR fast path: float32 or float64 samples (kMapAnomaly: values of the same type), unit column stride, one or two inputs,
// SCAN 1 / 2 / kScanArith, as values_fast_body: VEC elements per 16-byte non-temporal load, UNROLL loads in flight per array
// and lane, the workgroups of a row walking its tiles interleaved.  The results of a load's VEC samples leave as VEC / 2
// 16-byte non-temporal stores of two int64 or two float64 each; the ragged last tile is written by guarded scalar stores.
//
// Bytes in flight per lane: the loads of a tile, at most three streams (float64 pairs with values) of 16 * UNROLL = 64 bytes:
// 192, the limit values_fast_body documents, so no form reads its tile in halves.  The stores are not waited for.
//   streams   form                                  in flight per lane
//   1         single input, index / take                  64
//   2         single input, anomaly; pairs, index / take  128 (float32 pairs: 64)
//   3         pairs, anomaly                              192 (float32 pairs: 96)
// ---------------------------------------------------------------------------------------------
template <int OP, typename ST, int D, int SCAN>
__device__ __forceinline__ void map_fast_body(const MapParams& __restrict__ p) {
  static_assert(__is_same(ST, double) || __is_same(ST, float), "float32 / float64 samples and values");
  static_assert(SCAN == 1 || SCAN == 2 || SCAN == kScanArith, "tables with <= 2 edges per bucket, or arithmetic edges");
  constexpr bool V = OP == kMapAnomaly;
  constexpr int CMP = (__is_same(ST, float) && SCAN != kScanArith) ? 2 : 0;
  constexpr int VEC = 16 / (int)sizeof(ST);
  constexpr int UNROLL = D == 1 ? 4 : 8 / VEC;  // (the tile of values_fast_body: values_geometry counts on it)
  static_assert((D + (V ? 1 : 0)) * 16 * UNROLL <= 192, "no form keeps more than 192 bytes per lane in flight");
  using svec = typename VecOf<ST, VEC>::type;

  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = stage_tables(p);
  const double* centre = nullptr;
  const double* scale = nullptr;
  if constexpr (OP != kMapIndex) {
    centre = map_stage_rows(p, row);
    scale = p.scale ? centre + p.n_bins : nullptr;
  }
  __syncthreads();

  const ST* sp[D];
#pragma unroll
  for (int d = 0; d < D; ++d) sp[d] = reinterpret_cast<const ST*>(p.s_ptr[d]) + row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]);
  const ST* vp = nullptr;
  if constexpr (V) vp = reinterpret_cast<const ST*>(p.w_ptr) + row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);
  uint64_t* out = reinterpret_cast<uint64_t*>(p.out) + row * p.n_cols;
  const uint32_t nb1 = D == 2 ? (uint32_t)p.dim[1].nb : 1u;

  const int64_t tile_elems = (int64_t)blockDim.x * VEC * UNROLL;
  const int64_t n_tiles = (p.n_cols + tile_elems - 1) / tile_elems;
  for (int64_t t = seg; t < n_tiles; t += p.segs) {
    const int64_t base = t * tile_elems;
    const bool full = base + tile_elems <= p.n_cols;
    svec xv[D][UNROLL], vv[V ? UNROLL : 1];
    if (full) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d][u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(sp[d] + i));
        if constexpr (V) vv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(vp + i));
      }
    } else {  // the ragged last tile: positions past the end become NaN samples, and nothing is written for them
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const bool in = i + v < p.n_cols;
#pragma unroll
          for (int d = 0; d < D; ++d) xv[d][u][v] = in ? sp[d][i + v] : (ST)__builtin_nanf("");
          if constexpr (V) vv[u][v] = in ? vp[i + v] : (ST)__builtin_nanf("");
        }
      }
    }
    uint32_t cnt[D][UNROLL][VEC];
    count_le_tile<CMP, SCAN, D, UNROLL, VEC>(xv, p, tab, 1, cnt);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
      uint64_t r[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        bool ok = true;
        uint32_t flat = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int b = bin_from_tile_count<CMP, SCAN>((typename Dom<CMP>::T)xv[d][u][v], p.dim[d], cnt[d][u][v]);
          ok &= b >= 0;
          flat = d == 0 ? (uint32_t)b : flat * nb1 + (uint32_t)b;
        }
        double val = 0.0;
        if constexpr (V) val = (double)vv[u][v];
        r[v] = map_result<OP>(ok, flat, val, centre, scale);
      }
      if (full) {
#pragma unroll
        for (int v = 0; v < VEC; v += 2) {
          map_pair pr;
          pr[0] = r[v];
          pr[1] = r[v + 1];
          __builtin_nontemporal_store(pr, reinterpret_cast<map_pair*>(out + i + v));
        }
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (i + v < p.n_cols) out[i + v] = r[v];
      }
    }
  }
}

// The kernels: map_fast<OP, ST, D, SCAN> (block 256) and map_generic<OP, CMP, TLDS> (block 512).
template <int OP, typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) map_fast(const MapParams p) {
  map_fast_body<OP, ST, D, SCAN>(p);
}
template <int OP, int CMP, bool TLDS>
__global__ void __launch_bounds__(512) map_generic(const MapParams p) {
  map_generic_body<OP, CMP, TLDS>(p);
}

}  // namespace xhist
