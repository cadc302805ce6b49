// What the JPEG -> packed RGB kernels share (jpeg_upsample.hip: 4:2:0 and 4:2:2, jpeg_decode.hip: 4:4:4): the passes of IJG
// libjpeg 9's scaled IDCTs, libjpeg's ycc_rgb_convert of one pixel with its family's green constants, the packed store of
// eight pixels, the wave-private LDS fence and the resident grid size.
#pragma once
#include "cu_count.h"
#include "idct_core.h"
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

// jidctint.c jpeg_idct_16x8 pass 1 = the 8-point islow column pass, in libjpeg's own width: INT32 is `long`, 64 bits, so the
// sum is exact and the workspace keeps (int)(sum >> 11), bits 11..42.  For inputs |v| <= M every product sum of the pass is
// bounded by (16384 + 2 * 4433 + 15137) M + 1024 in the even part plus (25172 + 2 * 20995 + 2 * 16069 + 4 * 9633) M in the
// odd part (the tmp2 output, the largest), 178219 M + 1024 together:
//   |v| <= 8191 (idct_core.h's `big` flag clear): below 1.46e9 < 2^31 -- idct_1d<0, true> gives the same bits in 32;
//   baseline's extreme, |coefficient| 1023 x table entry 255: up to 4.6e10 -- 32-bit wrap-around would keep bits 11..31
//     only, so this pass runs in 64 bits;  any int16 coefficient x 16-bit table entry: |v| < 2^31, sums < 2^49, still exact.
// Pass 2 (rows, idct16_1d<false, int>) needs no such care: the range-limit index is bits 18..27 of its sum.
__device__ __forceinline__ void idct8_columns_exact(const int in[8], int out[8]) {
  typedef long long T;
  T z2 = in[2], z3 = in[6];
  T z1 = (z2 + z3) * FIX_0_541196100;
  T tmp2 = z1 - z3 * FIX_1_847759065;
  T tmp3 = z1 + z2 * FIX_0_765366865;
  z2 = in[0]; z3 = in[4];
  T tmp0 = (z2 + z3) * 8192 + (1 << 10);
  T tmp1 = (z2 - z3) * 8192 + (1 << 10);
  const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  T z4 = tmp1 + tmp3;
  const T z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336; tmp1 *= FIX_2_053119869; tmp2 *= FIX_3_072711026; tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const T sum[8] = {tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3};
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = (int)(sum[k] >> 11);
}

// two little-endian words -> the eight samples of a row segment
__device__ __forceinline__ void unpack8(uint2 v, uint32_t s[8]) {
#pragma unroll
  for (int c = 0; c < 4; c++) { s[c] = (v.x >> (8 * c)) & 0xff; s[4 + c] = (v.y >> (8 * c)) & 0xff; }
}

// jdcolor.c ycc_rgb_convert: r = y + ((FIX(1.402) v + half) >> 16), b likewise with 1.772 u,
// g = y + ((-k_cb_g u + half - k_cr_g v) >> 16), each clamped to [0, 255]; the pixel is R | G << 8 | B << 16 | 255 << 24
__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t ycc_px(uint32_t y, uint32_t cb, uint32_t cr, int k_cr_g, int k_cb_g) {
  const int half = 1 << 15;
  const int yy = (int)y, u = (int)cb - 128, v = (int)cr - 128;
  const uint32_t r = clamp255(yy + ((FIX16(1.40200) * v + half) >> 16));
  const uint32_t g = clamp255(yy + (((-k_cb_g) * u + half + (-k_cr_g) * v) >> 16));
  const uint32_t b = clamp255(yy + ((FIX16(1.77200) * u + half) >> 16));
  return r | (g << 8) | (b << 16) | (255u << 24);
}

// the green constants of the two libjpeg families: variant 0 libjpeg 6b / libjpeg-turbo, 1 IJG 9
inline void ycc_green_constants(int variant, int* k_cr_g, int* k_cb_g) {
  *k_cr_g = variant ? FIX16(0.714136286) : FIX16(0.71414);
  *k_cb_g = variant ? FIX16(0.344136286) : FIX16(0.34414);
}

// four RGBA pixels -> the twelve bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
__device__ __forceinline__ void pack_rgb888(const uint32_t px[4], uint32_t d[3]) {
  d[0] = (px[0] & 0xffffff) | (px[1] << 24);
  d[1] = ((px[1] >> 8) & 0xffff) | (px[2] << 16);
  d[2] = ((px[2] >> 16) & 0xff) | (px[3] << 8);
}

// Eight horizontally adjacent pixels from column x0 of a w pixel wide image to dst: 32 (24) contiguous bytes as two (three)
// vector stores when all eight lie inside the image and the rows keep dst aligned (vec_ok), else byte by byte.  The alpha byte
// of that path is the pixel's own top byte (255, ycc_px): all four bytes of an RGBA pixel then come from one register.
template <int BPP>
__device__ __forceinline__ void store_px8(uint8_t* dst, const uint32_t px[8], uint32_t x0, uint32_t w, bool vec_ok) {
  if (vec_ok && x0 + 8 <= w) {
    if constexpr (BPP == 4) {
      *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]);
      *(uint4*)(dst + 16) = make_uint4(px[4], px[5], px[6], px[7]);
    } else {
      uint32_t d[6];
      pack_rgb888(px, d);
      pack_rgb888(px + 4, d + 3);
      *(uint2*)dst = make_uint2(d[0], d[1]);
      *(uint2*)(dst + 8) = make_uint2(d[2], d[3]);
      *(uint2*)(dst + 16) = make_uint2(d[4], d[5]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; c++) {
      if (x0 + c < w) {
        dst[c * BPP] = (uint8_t)px[c]; dst[c * BPP + 1] = (uint8_t)(px[c] >> 8); dst[c * BPP + 2] = (uint8_t)(px[c] >> 16);
        if constexpr (BPP == 4) dst[c * BPP + 3] = (uint8_t)(px[c] >> 24);
      }
    }
  }
}

// host: the grid of a persistent kernel, per_cu workgroups on each CU (cu_count.h) or one per tile when there are fewer
inline int resident_grid(uint32_t tiles, int per_cu) {
  const uint32_t r = (uint32_t)(device_cu_count() * per_cu);
  return (int)(tiles < r ? (tiles ? tiles : 1u) : r);
}

}  // namespace upsample
}  // namespace uhdr
