// xhist_extrema.hip.h — per-bin minimum and maximum of a value array (histogram_extrema): the keys, the statistic's policy
// for the shared kernel skeletons of xhist_values.hip.h, and its binning kernels (the drivers of xhist_extrema.hip are declared in
// xhist_values_api.h).
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

#include "xhist_values.hip.h"

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

// The statistic of the shared skeletons (xhist_values.hip.h): a bin's [min, max] keys, KT 64-bit (float64 values, and every
// value of the generic family) or 32-bit (float32 values of the fast family).  One copy of the slots.
template <typename KT>
struct ExtAcc {
  using K = ExtKeys<KT>;
  using slot_t = typename K::slot_t;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 0;
  static __device__ __forceinline__ void init(slot_t* slots, const Params& p, int64_t) {
    slot_t e;
    e[0] = K::kMin;
    e[1] = K::kMax;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) slots[b] = e;
  }
  // one value into a bin's LDS slot, atomics only where its key improves on what the slot holds
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* slots, uint32_t bin, V v) {
    const KT k = K::key(v);
    slot_t* s = slots + bin;
    const slot_t cur = *s;
    KT* keys = reinterpret_cast<KT*>(s);
    if (k < cur[0]) atomicMin(keys, k);
    if (k > cur[1]) atomicMax(keys + 1, k);
  }
  // ... and into the output's two key arrays (global memory): the same filter on a relaxed read of each
  static __device__ __forceinline__ void global_update(uint64_t* kmin, uint64_t* kmax, int64_t bin, uint64_t lo, uint64_t hi) {
    if (lo < __hip_atomic_load(kmin + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(reinterpret_cast<unsigned long long*>(kmin + bin), (unsigned long long)lo);
    if (hi > __hip_atomic_load(kmax + bin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(reinterpret_cast<unsigned long long*>(kmax + bin), (unsigned long long)hi);
  }
  static __device__ __forceinline__ void global_add(const Params& p, int64_t row, int64_t bin, double v) {
    const uint64_t k = extrema_key64(v);
    global_update(reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins, reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins, bin, k, k);
  }
  // the workgroup's slots into its output rows of minimum keys (out) and maximum keys (out2); bins nothing reached are skipped
  static __device__ __forceinline__ void flush(const slot_t* slots, const Params& p, int64_t row) {
    uint64_t* kmin = reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins;
    uint64_t* kmax = reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      const slot_t s = slots[b];
      if (s[0] == K::kMin) continue;  // (the min and the max of a bin are set together)
      global_update(kmin, kmax, b, K::wide(s[0]), K::wide(s[1]));
    }
  }
};

// The binning kernels: extrema_generic<CMP, LDS> (block 512) and extrema_fast<ST, D, SCAN> (block 256), the families of
// xhist_values.hip.h with the minimum keys at `out` and the maximum keys at `out2`.  Keys are 32-bit for float32 values.
//
// extrema_generic keeps the strided loop of values_generic_body written out in the kernel.  Through the shared body the
// LDS instances (<*, true>) hoist the per-input Params fields out of the loop and spill twice as many SGPRs (138 -> 266 for
// <0, true>), which costs up to 3.5% on int64 / mixed-domain inputs; written in the kernel they reload them from the
// kernel arguments.  The mean_var generic kernels use the shared body, as they always did.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) extrema_generic(const Params p) {
  using CT = typename Dom<CMP>::T;
  using A = ExtAcc<uint64_t>;
  const int64_t row = blockIdx.x / p.segs;
  const int seg = blockIdx.x % p.segs;
  const uint64_t* tab = p.tables_in_lds ? stage_tables(p) : p.tables;
  A::slot_t* slots = reinterpret_cast<A::slot_t*>(xhist_smem + ext_slots_offset(p));
  if (LDS) A::init(slots, p, row);
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
    bool ok = v == v;
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
    if (LDS) A::lds_add(slots, (uint32_t)flat, v);
    else A::global_update(kmin, kmax, flat, k, k);
  }
  if (LDS) {
    __syncthreads();
    A::flush(slots, p, row);
  }
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) extrema_fast(const Params p) {
  values_fast_body<ExtAcc<typename std::conditional<__is_same(ST, float), uint32_t, uint64_t>::type>, ST, D, SCAN>(p);
}

// ---------------------------------------------------------------------------------------------
// histogram_argextrema: where a bin's minimum and maximum lie.  Two passes, because no atomic takes a (key, position) pair of
// 128 bits.  Pass 1 is histogram_extrema's own (extrema_prepare and the binning kernels above) and leaves the keys of every
// bin's extremes in the two value outputs.  Pass 2 streams the samples and values again: of the samples whose key EQUALS the
// bin's minimum (maximum) key it keeps the smallest column index, a 64-bit unsigned minimum, so the answer is exact and does
// not depend on the order of arrival.  A finalize turns the keys into doubles.
//
// A bin's slot in pass 2 is [kmin, kmax, imin, imax]: 32 bytes with 64-bit keys, 24 for the fast family on float32 values.
// The keys are read-only there (init stages them from pass 1's output, which travels as w2_ptr with CovParams::plane between
// the two key planes); a position starts as ~0, which every column index undercuts and which reads as -1 in the int64 output.
//
// Equality, then minimum — and read before you atomic again: a sample goes on only where its key equals one of the slot's two,
// reads that position, and issues the atomic only where its own is smaller.  On unordered data almost no sample ties with an
// extreme; on constant or boolean values every sample does, and then the read keeps all but the improving ones (the lowest
// lanes of a workgroup's first tile) from the atomic unit.  A stale read is never wrong: positions only decrease.
// ---------------------------------------------------------------------------------------------
constexpr uint64_t kNoPosition = ~0ull;

template <typename KT>
struct ArgSlot {
  KT kmin, kmax;
  uint64_t imin, imax;
};
static_assert(sizeof(ArgSlot<uint64_t>) == 32 && sizeof(ArgSlot<uint32_t>) == 24, "the slot sizes the family rule is given");

// pass 1's 64-bit key of an output bin, as the slot holds it: exact for the 32-bit keys, whose values were float32
template <typename KT>
__device__ __forceinline__ KT arg_narrow(uint64_t k);
template <>
__device__ __forceinline__ uint64_t arg_narrow<uint64_t>(uint64_t k) { return k; }
template <>
__device__ __forceinline__ uint32_t arg_narrow<uint32_t>(uint64_t k) {
  if (k == kEmptyMin64) return kEmptyMin32;  // (the markers are no values; no sample's key equals one)
  if (k == kEmptyMax64) return kEmptyMax32;
  return extrema_key32((float)extrema_value64(k));
}

template <typename KT>
struct ArgAcc {
  using K = ExtKeys<KT>;
  using slot_t = ArgSlot<KT>;
  static constexpr bool kCopies = false;
  static constexpr int kExtra = 0;
  static constexpr bool kIndex = true;
  static __device__ __forceinline__ void init(slot_t* slots, const CovParams& p, int64_t row) {
    const uint64_t* kmin = reinterpret_cast<const uint64_t*>(p.w2_ptr) + row * p.n_bins;  // (the maximum keys: p.plane on)
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      slot_t e;
      e.kmin = arg_narrow<KT>(kmin[b]);
      e.kmax = arg_narrow<KT>(kmin[p.plane + b]);
      e.imin = e.imax = kNoPosition;
      slots[b] = e;
    }
  }
  // min(*at, pos) where pos improves on a relaxed read of *at
  static __device__ __forceinline__ void lds_lower(uint64_t* at, uint64_t pos) {
    if (pos < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
      atomicMin(reinterpret_cast<unsigned long long*>(at), (unsigned long long)pos);
  }
  static __device__ __forceinline__ void global_lower(uint64_t* at, uint64_t pos) {
    if (pos < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(reinterpret_cast<unsigned long long*>(at), (unsigned long long)pos);
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* slots, uint32_t bin, V v, uint64_t pos) {
    const KT k = K::key(v);
    slot_t* s = slots + bin;
    const KT lo = s->kmin, hi = s->kmax;  // (nothing writes the keys during the pass)
    if (k == lo) lds_lower(&s->imin, pos);
    if (k == hi) lds_lower(&s->imax, pos);
  }
  // the positions of row `row`: minima at out, maxima at out2
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double v, uint64_t pos) {
    const uint64_t k = extrema_key64(v);
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(p.w2_ptr) + row * p.n_bins + bin;
    if (k == keys[0]) global_lower(reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins + bin, pos);
    if (k == keys[p.plane]) global_lower(reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins + bin, pos);
  }
  // (a workgroup may have met a bin's minimum and not its maximum: each position on its own)
  static __device__ __forceinline__ void flush(const slot_t* slots, const CovParams& p, int64_t row) {
    uint64_t* imin = reinterpret_cast<uint64_t*>(p.out) + row * p.n_bins;
    uint64_t* imax = reinterpret_cast<uint64_t*>(p.out2) + row * p.n_bins;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      const uint64_t lo = slots[b].imin, hi = slots[b].imax;
      if (lo != kNoPosition) global_lower(imin + b, lo);
      if (hi != kNoPosition) global_lower(imax + b, hi);
    }
  }
};

// Pass 2's binning kernels, through the shared skeletons: argext_generic<CMP, LDS> (block 512), argext_fast<ST, D, SCAN>
// (block 256).  They take CovParams for its plane stride and read no x_* stream.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) argext_generic(const CovParams p) {
  values_generic_body<ArgAcc<uint64_t>, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) argext_fast(const CovParams p) {
  values_fast_body<ArgAcc<typename std::conditional<__is_same(ST, float), uint32_t, uint64_t>::type>, ST, D, SCAN>(p);
}

}  // namespace xhist

// xhist_extrema.hip, for the units whose statistic starts from a bin's extremes (xhist_sum.hip): pass 1 as histogram_argextrema
// runs it, the keys left in kmin / kmax [n_rows, n_bins]; *segs and *lds_bytes: its segments per row and its LDS bytes (0: no columns, no binning launch)
int xhist_extrema_pass1(const ValuesCall& k, const xhist::ValuesChoice& c, uint64_t* kmin, uint64_t* kmax, int64_t* segs,
                        size_t* lds_bytes);
