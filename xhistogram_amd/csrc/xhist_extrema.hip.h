// xhist_extrema.hip.h — per-bin minimum and maximum of a value array (histogram_extrema): the kernels, and what the C ABI
// (xhist_capi.hip) hands the selection function of the translation unit xhist_extrema.hip.
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  What a counted sample
// contributes is its value, converted to float64 (numpy's astype) and mapped to an order-preserving unsigned key
//     key(v) = bits(v) ^ (sign(v) ? ~0 : 1 << 63)
// under which unsigned integer order is the total order of the values with -0.0 < +0.0 (infinities and subnormals in their
// places).  Min and max are then integer atomics on keys: exact, deterministic, independent of the order of arrival.
// NaN values never become keys; the only bit patterns that map to ~0 (the "empty" marker of a minimum) and to 0 (that of a
// maximum) are NaNs, so a marker is never mistaken for a value.
//
// The caller's two float64 outputs ARE the key buffers: a prepare kernel writes the markers (or, accumulating, turns the
// doubles already there into keys, NaN into the marker), the binning kernel runs, a finalize kernel turns the keys back into
// doubles, markers into NaN.  No scratch.
//
// Read before you atomic: a bin's [min, max] keys sit side by side in one LDS slot (16 bytes; 8 for float32 values, whose
// keys are 32-bit).  A sample reads its slot with one ds_read and issues ds_min / ds_max only when it improves on what it
// read — on unordered data the improvements per bin grow like log(n), so the steady state is one LDS read per sample.  A
// stale read is never wrong: keys only move towards the extreme, so a value that does not beat an older key does not beat
// the current one.  The flush into the output and the kernels that work straight in global memory filter the same way.
#pragma once

#include "xhist_kernels.hip.h"

#include "../../include/xhist_amd.h"

namespace xhist {

constexpr uint64_t kEmptyMin64 = ~0ull, kEmptyMax64 = 0ull;
constexpr uint32_t kEmptyMin32 = ~0u, kEmptyMax32 = 0u;

__host__ __device__ __forceinline__ uint64_t extrema_key64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  return b ^ ((uint64_t)((int64_t)b >> 63) | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double extrema_value64(uint64_t k) {
  return __builtin_bit_cast(double, k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull));
}
__host__ __device__ __forceinline__ uint32_t extrema_key32(float v) {
  const uint32_t b = __builtin_bit_cast(uint32_t, v);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__host__ __device__ __forceinline__ float extrema_value32(uint32_t k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : ~0u));
}

// one bin's [min, max] keys, read together
typedef uint64_t ext_slot64 __attribute__((ext_vector_type(2), aligned(16)));
typedef uint32_t ext_slot32 __attribute__((ext_vector_type(2), aligned(8)));

template <typename KT>
struct ExtKeys;
template <>
struct ExtKeys<uint64_t> {
  using slot_t = ext_slot64;
  static constexpr uint64_t kMin = kEmptyMin64, kMax = kEmptyMax64;
  static __device__ __forceinline__ uint64_t key(double v) { return extrema_key64(v); }
  static __device__ __forceinline__ uint64_t wide(uint64_t k) { return k; }  // the output's 64-bit key of an LDS key
};
template <>
struct ExtKeys<uint32_t> {
  using slot_t = ext_slot32;
  static constexpr uint32_t kMin = kEmptyMin32, kMax = kEmptyMax32;
  static __device__ __forceinline__ uint32_t key(float v) { return extrema_key32(v); }
  // float -> double is exact and monotone: the float32 key's value, keyed again in 64 bits
  static __device__ __forceinline__ uint64_t wide(uint32_t k) { return extrema_key64((double)extrema_value32(k)); }
};

// one key into a bin's LDS slot, atomics only where it improves on what the slot holds
template <typename KT>
__device__ __forceinline__ void ext_lds_update(typename ExtKeys<KT>::slot_t* slots, uint32_t bin, KT k) {
  typename ExtKeys<KT>::slot_t* s = slots + bin;
  const typename ExtKeys<KT>::slot_t cur = *s;
  KT* keys = reinterpret_cast<KT*>(s);
  if (k < cur[0]) atomicMin(keys, k);
  if (k > cur[1]) atomicMax(keys + 1, k);
}

// ... and into the output's two key arrays (global memory): the same filter on a relaxed read of each
__device__ __forceinline__ void ext_global_update(uint64_t* kmin, uint64_t* kmax, int64_t bin, uint64_t k) {
  if (k < __hip_atomic_load(kmin + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(reinterpret_cast<unsigned long long*>(kmin + bin), (unsigned long long)k);
  if (k > __hip_atomic_load(kmax + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(reinterpret_cast<unsigned long long*>(kmax + bin), (unsigned long long)k);
}

// the slots sit behind the staged tables, 16-byte aligned
__host__ __device__ __forceinline__ size_t ext_slots_offset(const Params& p) { return (size_t)((p.table_words + 1) & ~1) * 8; }

template <typename KT>
__device__ __forceinline__ void ext_init(typename ExtKeys<KT>::slot_t* slots, uint32_t n_bins) {
  typename ExtKeys<KT>::slot_t e;
  e[0] = ExtKeys<KT>::kMin;
  e[1] = ExtKeys<KT>::kMax;
  for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x) slots[b] = e;
}

// a workgroup's LDS slots into the output rows `kmin` / `kmax`; bins nothing reached are skipped
template <typename KT>
__device__ __forceinline__ void ext_flush(const typename ExtKeys<KT>::slot_t* slots, uint32_t n_bins, uint64_t* kmin, uint64_t* kmax) {
  for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x) {
    const typename ExtKeys<KT>::slot_t s = slots[b];
    if (s[0] == ExtKeys<KT>::kMin) continue;  // (the min and the max of a bin are set together)
    const uint64_t lo = ExtKeys<KT>::wide(s[0]), hi = ExtKeys<KT>::wide(s[1]);
    if (lo < __hip_atomic_load(kmin + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(reinterpret_cast<unsigned long long*>(kmin + b), (unsigned long long)lo);
    if (hi > __hip_atomic_load(kmax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(reinterpret_cast<unsigned long long*>(kmax + b), (unsigned long long)hi);
  }
}

// ---------------------------------------------------------------------------------------------
// GENERIC family: any dtype per input and for the values, any element strides (broadcast and grouped rows), 1..8 inputs,
// compare domains 0 (float64), 1 (int64) and 3 (per input).  Params as for hist_generic, with the values in the w_* fields,
// the minimum keys at `out` and the maximum keys at `out2` ([n_rows, n_bins] each, pre-advanced to row p.row0).
//   LDS: the slots of every bin in LDS behind the tables (which are then in LDS too).  Else every update goes to global
//   memory, and the tables are read from LDS when they fit there (p.tables_in_lds) and through L2 otherwise.
// ---------------------------------------------------------------------------------------------
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) extrema_generic(const Params p) {
  using CT = typename Dom<CMP>::T;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = p.tables_in_lds ? stage_tables(p) : p.tables;
  ext_slot64* slots = reinterpret_cast<ext_slot64*>(xhist_smem + ext_slots_offset(p));
  if (LDS) ext_init<uint64_t>(slots, (uint32_t)p.n_bins);
  __syncthreads();

  uint64_t* kmin = reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins;
  uint64_t* kmax = reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins;
  const int nd = p.n_dims;
  int64_t roff[kMaxDims];
#pragma unroll
  for (int d = 0; d < kMaxDims; ++d) roff[d] = d < nd ? row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]) : 0;
  const int64_t voff = row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);

  const int64_t stride = (int64_t)p.segs * blockDim.x;
  for (int64_t i = (int64_t)seg * blockDim.x + threadIdx.x; i < p.n_cols; i += stride) {
    const double v = load_as<double>(p.w_ptr, p.w_dt, voff + i * p.w_cs);
    bool ok = v == v;  // NaN values are ignored (np.fmin / np.fmax)
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
    const uint64_t k = extrema_key64(v);
    if (LDS) ext_lds_update<uint64_t>(slots, (uint32_t)flat, k);
    else ext_global_update(kmin, kmax, flat, k);
  }
  if (LDS) {
    __syncthreads();
    ext_flush<uint64_t>(slots, (uint32_t)p.n_bins, kmin, kmax);
  }
}

// ---------------------------------------------------------------------------------------------
// VECTOR fast path: float32 or float64 samples with values of the same type, unit column stride, one or two inputs, bins in
// LDS; digitize by the tables with at most two edges per bucket (SCAN 1 / 2: float64 edges for float64 samples, float32
// thresholds for float32 ones) or by arithmetic (kScanArith).  Tiles as in hist_fast: VEC elements per 16-byte load, UNROLL
// loads in flight per array and lane; the workgroups of a row walk its tiles interleaved.  Keys are 32-bit for float32 values.
// ---------------------------------------------------------------------------------------------
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) extrema_fast(const Params p) {
  static_assert(__is_same(ST, double) || __is_same(ST, float), "float32 / float64 samples and values");
  static_assert(SCAN == 1 || SCAN == 2 || SCAN == kScanArith, "tables with <= 2 edges per bucket, or arithmetic edges");
  constexpr int CMP = (__is_same(ST, float) && SCAN != kScanArith) ? 2 : 0;
  constexpr int VEC = 16 / (int)sizeof(ST);
  constexpr int UNROLL = D == 1 ? 4 : 8 / VEC;  // 128 bytes of samples and values per lane in flight (192 for two inputs)
  using KT = typename std::conditional<__is_same(ST, float), uint32_t, uint64_t>::type;
  using K = ExtKeys<KT>;
  using slot_t = typename K::slot_t;
  using svec = typename VecOf<ST, VEC>::type;

  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = stage_tables(p);
  slot_t* slots = reinterpret_cast<slot_t*>(xhist_smem + ext_slots_offset(p));
  ext_init<KT>(slots, (uint32_t)p.n_bins);
  __syncthreads();

  const ST* sp[D];
#pragma unroll
  for (int d = 0; d < D; ++d) sp[d] = reinterpret_cast<const ST*>(p.s_ptr[d]) + row_offset(p.row0 + row, p.s_rs[d], p.s_ir[d], p.s_os[d]);
  const ST* vp = reinterpret_cast<const ST*>(p.w_ptr) + row_offset(p.row0 + row, p.w_rs, p.w_ir, p.w_os);
  const uint32_t nb1 = D == 2 ? (uint32_t)p.dim[1].nb : 1u;

  const int64_t tile_elems = (int64_t)blockDim.x * VEC * UNROLL;
  const int64_t n_tiles = (p.n_cols + tile_elems - 1) / tile_elems;
  for (int64_t t = seg; t < n_tiles; t += p.segs) {
    const int64_t base = t * tile_elems;
    svec xv[D][UNROLL], vv[UNROLL];
    if (base + tile_elems <= p.n_cols) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int d = 0; d < D; ++d) xv[d][u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(sp[d] + i));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const svec*>(vp + i));
      }
    } else {  // the ragged last tile: positions past the end become NaN samples, which digitize drops
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + ((int64_t)u * blockDim.x + tid) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const bool in = i + v < p.n_cols;
#pragma unroll
          for (int d = 0; d < D; ++d) xv[d][u][v] = in ? sp[d][i + v] : (ST)__builtin_nanf("");
          vv[u][v] = in ? vp[i + v] : (ST)__builtin_nanf("");
        }
      }
    }
    uint32_t cnt[D][UNROLL][VEC];
    count_le_tile<CMP, SCAN, D, UNROLL, VEC>(xv, p, tab, 1, cnt);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
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
        if (ok) ext_lds_update<KT>(slots, flat, K::key(val));
      }
  }
  __syncthreads();
  ext_flush<KT>(slots, (uint32_t)p.n_bins, reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins,
                reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins);
}

}  // namespace xhist

// ---- the selection function of xhist_extrema.hip, called by xhist_plan_execute_extrema (xhist_capi.hip) --------------------
// What it needs of a plan: the compare domain, the native (start, cnt) tables, the uint16 tables of the linear scan in the
// float64 and the float32-threshold domain (blob == nullptr: not built), and whether every dimension has arithmetic edges.
struct ExtremaTables {
  const xhist::DimTable* dim;
  const uint64_t* blob;
  int32_t words;
  int max_cnt;
};
struct ExtremaPlan {
  int n_dims, cmp;
  int64_t n_bins;
  int cus;
  size_t lds_max;
  bool arith;
  ExtremaTables native, fine64, fine32;
};
// The three launches on `stream` (prepare, binning, finalize) for DEVICE arrays the caller has validated, n_rows and n_cols
// > 0, the plan's device current.  Returns XHIST_OK, or an error status with a message in `err`; `desc` receives a line
// about the launch.
int xhist_extrema_run(const ExtremaPlan& pl, const xhist_array* samples, const xhist_array* values, int64_t n_rows, int64_t n_cols,
                      double* out_min, double* out_max, int accumulate, hipStream_t stream, char* err, size_t err_cap, char* desc,
                      size_t desc_cap);
// the census log of launched kernels (xhist_host_common.hip.h: log_picked_kernel), for the launches of xhist_extrema.hip
void xhist_log_picked_kernel(const void* fn);
