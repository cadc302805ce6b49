// The map byte of generateGainMap for a gain-map gamma != 1 without a pow: both byte functions of the encode side --
//   one pass  (uint8_t)(powf(n, gamma) * 255.0f)                                              (gainmapmath.cpp:769-770)
//   two pass  m = (float)pow((double)m, (double)gamma); clip(m * 255 + 0.5, 0, 255), truncated  (gainmapmath.cpp:784-789)
// are staircases of one float, byte(v) = max{ k : T[k] <= v } over the 256 thresholds the host built and checked with its own libm
// (host_tables.cpp: gamma_code_table; T[0] = 0, T[k] the smallest float whose byte is >= k).  A block holds the one-pass set,
// then the two-pass set, kGammaCodeN floats each.
//   gamma_code  the eight-step binary search, exact for every float: a negative argument or a NaN passes no comparison and gives
//               0, which is what the reference's conversion of pow's NaN gives; anything from T[255] on gives 255.  For a gamma
//               that is an even integer pow(-x, gamma) is pow(x, gamma) instead: T[0] is then -0.0f (the search never reads
//               T[0]) and its sign bit clears the argument's.
// No estimate-and-settle form (gain_index.h): the search is eight dependent loads of a 1 KB table on paths that run per sample
// only where no bucket table exists.
// Shared by encode_core.h (encode_gain's per-sample tail), generate_gainmap.hip (the table builder and pass 2's per-sample tail) and
// encode_api1_fused.hip (map_blocks_kernel's per-sample tail); swept over every float on the device by selftest.hip (sweep 6).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "uhdr_types.h"

namespace uhdr {

__device__ __forceinline__ uint32_t gamma_code(float v, const float* T) {
  v = __uint_as_float(__float_as_uint(v) & ~__float_as_uint(T[0]));
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = (uint32_t)kGammaCodeN / 2; step; step >>= 1)
    if (v >= T[lo + step]) lo += step;  // lo + step <= 255
  return lo;
}
__device__ __forceinline__ const float* gamma_thr_onepass(const float* block) { return block; }
__device__ __forceinline__ const float* gamma_thr_twopass(const float* block) { return block + kGammaCodeN; }

}  // namespace uhdr
