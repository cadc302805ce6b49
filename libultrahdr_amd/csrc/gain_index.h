// GainLUT::getGainFactor's table index for a gain-map gamma != 1 -- int(pow(g, 1 / gamma) * 1023 + 0.5) clipped to 0..1023
// (gainmapmath.h:483-489) -- without a pow: index(g) = max{ i : T[i] <= g } over the thresholds the host built and checked
// with its own libm (host_tables.cpp: gamma_index_table).  T points one float into a kGammaThrN block: T[-1] = 0,
// T[0] = 0, T[1..1023] the steps (non-decreasing), T[1024] = T[1025] = +inf.
//   gain_index_search  the ten-step binary search, exact for every g >= 0
//   gain_index         the hardware's log2 / exp2 give an estimate; the four thresholds around it -- two adjacent pairs --
//                      settle the index when T[est - 1] <= g < T[est + 2], which also proves it.  A lane whose estimate is
//                      further off says so, and the search runs for the wave's flagged lanes.  Either way the result is a
//                      function of T alone: the accuracy of the estimate decides the cost, never the index.
//                      g = 0: log2 = -inf, exp2 = 0, estimate 0 = the index.  g just above 1: estimate 1023, and
//                      T[1024] = +inf confirms it.
// Shared by apply_gainmap.hip (quad kernel SMODE 2, generic kernel GTAB 1) and the device-wide sweep of selftest.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace uhdr {

__device__ __forceinline__ uint32_t gain_index_search(float g, const float* T) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = 512; step; step >>= 1)
    if (g >= T[lo + step]) lo += step;  // lo + step <= 1023
  return lo;
}

__device__ __forceinline__ uint32_t gain_index_try(float g, const float* T, float ginv, bool& ok) {
  const float e = __builtin_amdgcn_exp2f(ginv * __builtin_amdgcn_logf(g));  // v_log_f32, v_mul_f32, v_exp_f32
  uint32_t est;
  asm("v_cvt_u32_f32 %0, %1" : "=v"(est) : "v"(__builtin_fmaf(e, 1023.0f, 0.5f)));  // saturating: NaN and negatives give 0
  est = est < 1023u ? est : 1023u;
  const float* q = T + est;
  const float a = q[-1], b = q[0], c = q[1], d = q[2];
  ok = g >= a && g < d;
  return est + (g >= c ? 1u : 0u) - (g < b ? 1u : 0u);
}

__device__ __forceinline__ uint32_t gain_index(float g, const float* T, float ginv) {
  bool ok;
  uint32_t idx = gain_index_try(g, T, ginv, ok);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, 0)) {
    if (!ok) idx = gain_index_search(g, T);
  }
  return idx;
}

}  // namespace uhdr
