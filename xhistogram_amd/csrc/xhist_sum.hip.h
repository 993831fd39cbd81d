// xhist_sum.hip.h — per-bin sums of a value array that do not depend on the order of arrival (histogram_sum): the integer
// arithmetic of the definition, stated once for host and device, the accumulator policy of pass 2 for the shared kernel skeletons
// of xhist_values.hip.h, and its binning kernels (the driver of xhist_sum.hip is declared in xhist_values_api.h).
//
// Which samples count is decided exactly as for the histogram: the same digitize, the same tables.  A counted sample whose value
// is not NaN contributes that value, converted to float64.  Per (row, bin), all on integers:
//   1. A = the largest |v| of the bin: max(|vmin|, |vmax|) of histogram_extrema, whose kernels are pass 1, unchanged.
//   2. E = frexp(A)'s exponent (|v| < 2^E), U = max(E - 96, -1074); the unit is 2^U.
//   3. A value v = s * m * 2^e (m the 53-bit integer significand, e = -1074 for subnormals) becomes q = m << (e - U), or
//      m >> (U - e) truncated towards zero where e < U (0 once the shift reaches 64).  q < 2^96: three unsigned 32-bit limbs, and
//      s * limb_j is added into three int64 accumulators L0, L1, L2.
//   4. A row has fewer than 2^31 samples, so |L_j| < 2^63 and S = L0 + L1 * 2^32 + L2 * 2^64 fits a signed 128-bit integer.
//   5. total = RN_even(S * 2^U): one rounding, in integer arithmetic (sum_round), overflowing to +-inf as IEEE does; zero is +0.0.
//   6. A = inf: pass 2 counts the +inf values in L0 and the -inf values in L1 and skips the finite ones; total is NaN where both
//      counts are non-zero, else the infinity present.
// Integer addition is associative, so the result is the same bits for any order of arrival, launch geometry, number of slot
// copies, family and home.  A value whose lowest set bit lies at or above 2^U is converted exactly: every value within a factor
// 2^43 of A, and every value where E - 96 <= -1074.  A bin of such values gets the correctly rounded exact sum; in general
// |total - exact| <= ulp(total) / 2 + n * 2^(E - 96).
//
// Pass 2's LDS slot is 30 bytes: {int64 L0, L1, L2; uint32 count; int16 U}, four slots to a group of 120 bytes (SumGroup), the
// same for float32 values.  init stages U from pass
// 1's key planes (w2_ptr: the minimum keys, the maximum keys CovParams::plane on, as ArgAcc reads them); a sample reads U, forms
// its limbs and issues up to three 64-bit integer LDS adds (a zero limb is skipped) and the count.  The fast family keeps
// 2^copies_log2 copies of every slot, as the moments do.  A flush adds the slots nothing left empty into the int64 planes with
// 64-bit integer global atomics; without LDS room the generic family adds every sample there.
#pragma once

#include "xhist_extrema.hip.h"

namespace xhist {

constexpr int32_t kSumUnitMin = -1074;        // the unit of the subnormals: no unit lies below it
constexpr int32_t kSumUnitInf = 0x7fffffff;   // the marker exponent of a bin that holds an infinity

// steps 1 and 2: a bin's unit exponent U from pass 1's keys, or kSumUnitInf (an empty bin: any U, nothing reaches it)
__host__ __device__ __forceinline__ int32_t sum_unit(uint64_t kmin, uint64_t kmax) {
  if (kmin == kEmptyMin64) return kSumUnitMin;
  const uint64_t mag = 0x7fffffffffffffffull;
  const uint64_t a = __builtin_bit_cast(uint64_t, extrema_value64(kmin)) & mag, b = __builtin_bit_cast(uint64_t, extrema_value64(kmax)) & mag;
  const int32_t be = (int32_t)((a > b ? a : b) >> 52);  // (the order of the bit patterns is the order of the magnitudes)
  if (be == 0x7ff) return kSumUnitInf;
  // a normal A = 1.f * 2^(be - 1023) has E = be - 1022; a subnormal or zero A (be 0) lands below the floor
  const int32_t u = be - 1022 - 96;
  return u < kSumUnitMin ? kSumUnitMin : u;
}

// step 3: the limbs of |v| in units of 2^U, for a finite v of a bin with this U; returns whether v is negative.  Where the
// shift is to the left it is at most 43: a normal v has m >= 2^52 and q < 2^96; a subnormal v has e = -1074 <= U.
__host__ __device__ __forceinline__ bool sum_limbs(double v, int32_t U, uint32_t (&limb)[3]) {
  const uint64_t bits = __builtin_bit_cast(uint64_t, v);
  const int32_t be = (int32_t)((bits >> 52) & 0x7ff);
  const uint64_t frac = bits & 0x000fffffffffffffull;
  const uint64_t m = be ? frac | 0x0010000000000000ull : frac;
  const int32_t sh = (be ? be - 1075 : -1074) - U;
  uint64_t lo, hi = 0;
  if (sh > 0) {
    lo = m << sh;
    hi = m >> (64 - sh);
  } else {
    lo = -sh >= 64 ? 0 : m >> -sh;
  }
  limb[0] = (uint32_t)lo;
  limb[1] = (uint32_t)(lo >> 32);
  limb[2] = (uint32_t)hi;
  return (bits >> 63) != 0;
}

// steps 4 and 5: RN_even((L0 + L1 * 2^32 + L2 * 2^64) * 2^U) for U >= -1074.  A magnitude of at most 53 bits is exact, as a
// subnormal too (the unit of the subnormals is 2^-1074 <= 2^U); a longer one is a normal number, rounded once from the bits it
// drops: the half bit, and whether anything lies below it.
__host__ __device__ __forceinline__ double sum_round(int64_t L0, int64_t L1, int64_t L2, int32_t U) {
  typedef unsigned __int128 u128;
  const u128 s = (u128)(__int128)L0 + ((u128)(__int128)L1 << 32) + ((u128)(__int128)L2 << 64);  // (two's complement: exact, |S| < 2^127)
  const bool neg = (__int128)s < 0;
  const u128 mag = neg ? (u128)0 - s : s;
  if (mag == 0) return 0.0;
  const uint64_t top = (uint64_t)(mag >> 64);
  const int nbits = top ? 128 - __builtin_clzll(top) : 64 - __builtin_clzll((uint64_t)mag);
  int64_t e_top = (int64_t)U + nbits - 1;  // the value lies in [2^e_top, 2^(e_top + 1))
  uint64_t out;
  if (e_top < -1022) {
    out = (uint64_t)mag << (U + 1074);  // subnormal: a whole number of units 2^-1074, below 2^52 of them
  } else {
    uint64_t mant;
    if (nbits <= 53) {
      mant = (uint64_t)mag << (53 - nbits);
    } else {
      const int drop = nbits - 53;
      mant = (uint64_t)(mag >> drop);
      const u128 rem = mag & (((u128)1 << drop) - 1), half = (u128)1 << (drop - 1);
      if (rem > half || (rem == half && (mant & 1))) ++mant;
      if (mant >> 53) {  // rounded up to the next power of two
        mant >>= 1;
        ++e_top;
      }
    }
    out = e_top > 1023 ? 0x7ff0000000000000ull : ((uint64_t)(e_top + 1023) << 52) | (mant & 0x000fffffffffffffull);
  }
  return __builtin_bit_cast(double, out | (neg ? 0x8000000000000000ull : 0ull));
}

// step 6 and the empty bin: a bin's total from its count, its keys and its limbs
__host__ __device__ __forceinline__ double sum_total(uint64_t count, uint64_t kmin, uint64_t kmax, int64_t L0, int64_t L1, int64_t L2) {
  if (!count) return 0.0;
  const int32_t U = sum_unit(kmin, kmax);
  if (U != kSumUnitInf) return sum_round(L0, L1, L2, U);
  if (L0 && L1) return __builtin_nan("");
  return L0 ? __builtin_inf() : -__builtin_inf();
}

// Pass 2's slots, four to a group of 120 bytes, 30 bytes a slot: slot i is entry i & 3 of group i >> 2.  A slot of its own would
// take 32 bytes, and at 32 bytes C4's 50 bins keep 8 copies within the 24 KiB of the copies' rule where 30 bytes keep 16, and
// 50 x 50 bins leave room for one workgroup on a CU where 30 bytes leave room for two (measured: DESIGN 4.7).  The unit
// exponent fits 16 bits.  The family rule is told 30 bytes; the driver rounds the slots up to whole groups.
struct SumGroup {
  int64_t L[4][3];
  uint32_t count[4];
  int16_t U[4];
};
static_assert(sizeof(SumGroup) == 120 && alignof(SumGroup) == 8, "four slots of 30 bytes, the size the family rule is given");
constexpr int16_t kSumUnitInf16 = 0x7fff;  // kSumUnitInf as a group holds it

struct SumAcc {
  using slot_t = SumGroup;
  static constexpr bool kCopies = true;
  static constexpr int kExtra = 0;
  static __device__ __forceinline__ void init(slot_t* s, const CovParams& p, int64_t row) {
    const uint64_t* kmin = reinterpret_cast<const uint64_t*>(p.w2_ptr) + row * p.n_bins;  // (the maximum keys: p.plane on)
    const uint32_t n = (uint32_t)p.n_bins << p.copies_log2;
    for (uint32_t i = threadIdx.x; i < ((n + 3) & ~3u); i += blockDim.x) {  // (the last group whole: its spare slots too)
      slot_t& g = s[i >> 2];
      const uint32_t k = i & 3, b = i >> p.copies_log2;
      g.L[k][0] = g.L[k][1] = g.L[k][2] = 0;
      g.count[k] = 0;
      const int32_t U = i < n ? sum_unit(kmin[b], kmin[p.plane + b]) : kSumUnitMin;
      g.U[k] = U == kSumUnitInf ? kSumUnitInf16 : (int16_t)U;
    }
  }
  // one value into the accumulators L[0], L[stride], L[2 * stride] of a bin with unit exponent U (LDS or global memory: the
  // address space follows the pointer once this is inlined)
  static __device__ __forceinline__ void add(unsigned long long* L, int64_t stride, int32_t U, double v) {
    if (U == kSumUnitInf) {
      const uint64_t bits = __builtin_bit_cast(uint64_t, v);
      if ((bits & 0x7fffffffffffffffull) == 0x7ff0000000000000ull) atomicAdd(L + ((bits >> 63) ? stride : 0), 1ull);
      return;
    }
    uint32_t limb[3];
    const bool neg = sum_limbs(v, U, limb);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (limb[j]) atomicAdd(L + j * stride, neg ? 0ull - (unsigned long long)limb[j] : (unsigned long long)limb[j]);
  }
  template <typename V>
  static __device__ __forceinline__ void lds_add(slot_t* s, uint32_t i, V v) {
    slot_t& g = s[i >> 2];
    const uint32_t k = i & 3;
    atomicAdd(&g.count[k], 1u);
    const int16_t U = g.U[k];  // (nothing writes U during the pass)
    add(reinterpret_cast<unsigned long long*>(g.L[k]), 1, U == kSumUnitInf16 ? kSumUnitInf : (int32_t)U, (double)v);
  }
  // the limb planes of row `row` at out [3], the counts at out2
  static __device__ __forceinline__ void global_add(const CovParams& p, int64_t row, int64_t bin, double v) {
    const int64_t i = row * p.n_bins + bin;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(p.w2_ptr) + i;
    atomicAdd(reinterpret_cast<unsigned long long*>(p.out2) + i, 1ull);
    add(reinterpret_cast<unsigned long long*>(p.out) + i, p.plane, sum_unit(keys[0], keys[p.plane]), v);
  }
  // the copies of a bin summed (integers: in any order), then the bins something reached into the planes
  static __device__ __forceinline__ void flush(const slot_t* s, const CovParams& p, int64_t row) {
    unsigned long long* L = reinterpret_cast<unsigned long long*>(p.out) + row * p.n_bins;
    unsigned long long* count = reinterpret_cast<unsigned long long*>(p.out2) + row * p.n_bins;
    const uint32_t copies = 1u << p.copies_log2;
    for (uint32_t b = threadIdx.x; b < (uint32_t)p.n_bins; b += blockDim.x) {
      unsigned long long a0 = 0, a1 = 0, a2 = 0, n = 0;
      for (uint32_t c = 0; c < copies; ++c) {
        const uint32_t i = (b << p.copies_log2) + c;
        const slot_t& g = s[i >> 2];
        a0 += (unsigned long long)g.L[i & 3][0];
        a1 += (unsigned long long)g.L[i & 3][1];
        a2 += (unsigned long long)g.L[i & 3][2];
        n += g.count[i & 3];
      }
      if (!n) continue;
      atomicAdd(count + b, n);
      if (a0) atomicAdd(L + b, a0);
      if (a1) atomicAdd(L + p.plane + b, a1);
      if (a2) atomicAdd(L + 2 * p.plane + b, a2);
    }
  }
};

// Pass 2's binning kernels, through the shared skeletons: sum_generic<CMP, LDS> (block 512), sum_fast<ST, D, SCAN> (block 256).
// They take CovParams for its plane stride and read no x_* stream.
template <int CMP, bool LDS>
__global__ void __launch_bounds__(512) sum_generic(const CovParams p) {
  values_generic_body<SumAcc, CMP, LDS>(p);
}
template <typename ST, int D, int SCAN>
__global__ void __launch_bounds__(256) sum_fast(const CovParams p) {
  values_fast_body<SumAcc, ST, D, SCAN>(p);
}

}  // namespace xhist
