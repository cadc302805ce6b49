// What the subsampled-JPEG -> packed RGB kernels share (jpeg_upsample.hip: 4:2:0, jpeg_upsample422.hip: 4:2:2): the 16-point
// pass of IJG libjpeg 9's scaled IDCTs, libjpeg's ycc_rgb_convert of one pixel, and the wave-private LDS fence.
#pragma once
#include "uhdr_types.h"

namespace uhdr {
namespace upsample {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

#define FIX13(x) ((int)((x) * 8192.0 + 0.5))
#define FIX16(x) ((int)((x) * 65536.0 + 0.5))

// jidctint.c jpeg_idct_16x16, one 16-point pass on 8 inputs.  T = int: wrap-around 32-bit arithmetic; T = long long: exact.
// Pass 1 (columns): libjpeg's INT32 is `long`, 64 bits, and the stored workspace value is bits 11..42 of the sum -- exact
// only in 64 bits unless every input is small (see the caller).  Pass 2 (rows): the range-limit index is bits 18..27 of the
// sum, which wrap-around arithmetic reproduces; the rounding constant and RANGE_CENTER ride on the DC term as in libjpeg.
// jpeg_idct_16x8's row pass is this pass 2, statement for statement.
template <bool PASS1, typename T>
__device__ __forceinline__ void idct16_1d(const int x[8], int out[16]) {
  T tmp0 = PASS1 ? (T)x[0] * (T)8192 + (T)(1 << 10) : (T)((uint32_t)(x[0] + ((512 << 5) + (1 << 4))) << 13);
  T z1 = x[4];
  T tmp1 = z1 * FIX13(1.306562965), tmp2 = z1 * FIX13(0.541196100);
  T tmp10 = tmp0 + tmp1, tmp11 = tmp0 - tmp1, tmp12 = tmp0 + tmp2, tmp13 = tmp0 - tmp2;
  z1 = x[2];
  T z2 = x[6];
  T z3 = z1 - z2;
  T z4 = z3 * FIX13(0.275899379);
  z3 = z3 * FIX13(1.387039845);
  tmp0 = z3 + z2 * FIX13(2.562915447);
  tmp1 = z4 + z1 * FIX13(0.899976223);
  tmp2 = z3 - z1 * FIX13(0.601344887);
  T tmp3 = z4 - z2 * FIX13(0.509795579);
  const T tmp20 = tmp10 + tmp0, tmp27 = tmp10 - tmp0, tmp21 = tmp12 + tmp1, tmp26 = tmp12 - tmp1;
  const T tmp22 = tmp13 + tmp2, tmp25 = tmp13 - tmp2, tmp23 = tmp11 + tmp3, tmp24 = tmp11 - tmp3;
  z1 = x[1]; z2 = x[3]; z3 = x[5]; z4 = x[7];
  tmp11 = z1 + z3;
  tmp1 = (z1 + z2) * FIX13(1.353318001);
  tmp2 = tmp11 * FIX13(1.247225013);
  tmp3 = (z1 + z4) * FIX13(1.093201867);
  tmp10 = (z1 - z4) * FIX13(0.897167586);
  tmp11 = tmp11 * FIX13(0.666655658);
  tmp12 = (z1 - z2) * FIX13(0.410524528);
  tmp0 = tmp1 + tmp2 + tmp3 - z1 * FIX13(2.286341144);
  tmp13 = tmp10 + tmp11 + tmp12 - z1 * FIX13(1.835730603);
  z1 = (z2 + z3) * FIX13(0.138617169);
  tmp1 += z1 + z2 * FIX13(0.071888074);
  tmp2 += z1 - z3 * FIX13(1.125726048);
  z1 = (z3 - z2) * FIX13(1.407403738);
  tmp11 += z1 - z3 * FIX13(0.766367282);
  tmp12 += z1 + z2 * FIX13(1.971951411);
  z2 += z4;
  z1 = z2 * -FIX13(0.666655658);
  tmp1 += z1;
  tmp3 += z1 + z4 * FIX13(1.065388962);
  z2 = z2 * -FIX13(1.247225013);
  tmp10 += z2 + z4 * FIX13(3.141271809);
  tmp12 += z2;
  z2 = (z3 + z4) * -FIX13(1.353318001);
  tmp2 += z2;
  tmp3 += z2;
  z2 = (z4 - z3) * FIX13(0.410524528);
  tmp10 += z2;
  tmp11 += z2;
  const T e[8] = {tmp20, tmp21, tmp22, tmp23, tmp24, tmp25, tmp26, tmp27};
  const T o[8] = {tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13};
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const T a = e[k] + o[k], b = e[k] - o[k];
    if constexpr (PASS1) {
      out[k] = (int)(a >> 11);
      out[15 - k] = (int)(b >> 11);
    } else {
      out[k] = min(max((int)(((uint32_t)a >> 18) & 1023u) - 384, 0), 255);
      out[15 - k] = min(max((int)(((uint32_t)b >> 18) & 1023u) - 384, 0), 255);
    }
  }
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t ycc_px(uint32_t y, uint32_t cb, uint32_t cr, int k_cr_g, int k_cb_g) {
  const int half = 1 << 15;
  const int yy = (int)y, u = (int)cb - 128, v = (int)cr - 128;
  const uint32_t r = clamp255(yy + ((FIX16(1.40200) * v + half) >> 16));
  const uint32_t g = clamp255(yy + (((-k_cb_g) * u + half + (-k_cr_g) * v) >> 16));
  const uint32_t b = clamp255(yy + ((FIX16(1.77200) * u + half) >> 16));
  return r | (g << 8) | (b << 16) | (255u << 24);
}

}  // namespace upsample
}  // namespace uhdr
