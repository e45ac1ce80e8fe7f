// k16_rows.hpp -- what the candidate rows of the split-fp16 search (knn16.hip) need to be ranked: shared with refine.hip, whose
// fused row pass takes the rows raw and ranks them in registers.
#pragma once
#include "common.hpp"

namespace meld {

constexpr int K16_ROW_CAPMAX = 256;                 // largest row stride of a candidate row (ksel = 128)
constexpr int K16_ROW_SLOTS = K16_ROW_CAPMAX / 64;  // row entries per lane

// fp32 -> unsigned with the same order (and back)
__device__ __forceinline__ unsigned ordered_bits(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Bitonic network over the 64 SL keys of a wave, ascending: element i = 64 e + lane sits in key[e], so exchanges at distance >= 64
// stay inside a lane and the others are one __shfl_xor.
template <int SL>
__device__ __forceinline__ void k16_bitonic_sort(unsigned long long (&key)[SL], int lane) {
  constexpr int NE = 64 * SL;
#pragma unroll
  for (int k = 2; k <= NE; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
        const int je = j >> 6;
#pragma unroll
        for (int e = 0; e < SL; ++e) {
          if ((e & je) == 0) {
            const int i = 64 * e + lane;
            const bool asc = (i & k) == 0;
            const unsigned long long a = key[e], b = key[e | je];
            const bool sw = asc ? (b < a) : (a < b);
            key[e] = sw ? b : a;
            key[e | je] = sw ? a : b;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < SL; ++e) {
          const int i = 64 * e + lane;
          const unsigned long long o = __shfl_xor(key[e], j, 64);
          const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
          key[e] = keep_min ? (o < key[e] ? o : key[e]) : (o < key[e] ? key[e] : o);
        }
      }
    }
  }
}

}  // namespace meld
