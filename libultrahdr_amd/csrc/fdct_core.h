// The libjpeg JDCT_ISLOW forward DCT + quantizer as wave-level building blocks, bit-exact; the counterpart of idct_core.h.
// Shared by the stand-alone kernels (fdct_quant.hip) and the fused encode kernels (encode_api1_fused.hip).
//
// The arithmetic is NOT in the reference tree: libultrahdr hands planes to libjpeg
// (its lib/src/jpegencoderhelper.cpp:187-198 sets jpeg_set_quality(q, TRUE) and
// dct_method = JDCT_ISLOW; :297 jpeg_write_raw_data).  What runs there is the public
// Loeffler-Ligtenberg-Moschytz integer DCT (libjpeg jfdctint.c: CONST_BITS 13, PASS1_BITS 2, a
// row pass scaled by 4 then a column pass, round-to-nearest descales) followed by jcdctmgr.c's
// round-half-away division by (quantval << 3).  Integers only => results are exact.
//
// Mapping: one wavefront = 8 blocks.  Row pass: lane (row rr = lane/8, block rb = lane%8) holds the 8 samples of its row and
// runs the 1-D butterfly in registers.  The 8x8 tiles are transposed through LDS (row-padded to 9 words: conflict-free column
// reads), the column pass and the quantizer run with lane = (block, column), and a second LDS transpose lets every lane emit
// one coefficient ROW (8 x int16 = 16 bytes), so a wave that owns 8 adjacent blocks writes 1 KiB contiguous in libjpeg's
// JBLOCK order.  The quantizer divides by multiplying with ceil(2^32 / q) (exact for the 19-bit magnitudes that occur;
// q <= 2040); divisors and their reciprocals are computed on the host and travel in the kernel arguments.  Every butterfly
// operand is below 2^23 in magnitude (samples +-128 -> row pass <= 2^13 -> column pass <= 2^16; constants < 2^15), so the
// multiplies are the full-rate 24-bit ones (v_mul_i32_i24 returns the low 32 bits of the exact product).
#pragma once
#include "jdct_fix.h"
#include "uhdr_types.h"

namespace uhdr {
namespace fdct {

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one 8-point pass.  PASS 0: rows, results scaled by 4.  PASS 1: columns.
template <int PASS>
__device__ __forceinline__ void fdct_1d(const int in[8], int out[8]) {
  constexpr int sh = PASS == 0 ? 13 - 2 : 13 + 2;
  int t0 = in[0] + in[7], t7 = in[0] - in[7], t1 = in[1] + in[6], t6 = in[1] - in[6];
  int t2 = in[2] + in[5], t5 = in[2] - in[5], t3 = in[3] + in[4], t4 = in[3] - in[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (PASS == 0) {
    out[0] = (t10 + t11) * 4;
    out[4] = (t10 - t11) * 4;
  } else {
    out[0] = descale(t10 + t11, 2);
    out[4] = descale(t10 - t11, 2);
  }
  int z1 = __mul24(t12 + t13, FIX_0_541196100);
  out[2] = descale(z1 + __mul24(t13, FIX_0_765366865), sh);
  out[6] = descale(z1 + __mul24(t12, -FIX_1_847759065), sh);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = __mul24(z3 + z4, FIX_1_175875602);
  t4 = __mul24(t4, FIX_0_298631336);
  t5 = __mul24(t5, FIX_2_053119869);
  t6 = __mul24(t6, FIX_3_072711026);
  t7 = __mul24(t7, FIX_1_501321110);
  z1 = __mul24(z1, -FIX_0_899976223);
  z2 = __mul24(z2, -FIX_2_562915447);
  z3 = __mul24(z3, -FIX_1_961570560);
  z4 = __mul24(z4, -FIX_0_390180644);
  z3 += z5;
  z4 += z5;
  out[7] = descale(t4 + z1 + z3, sh);
  out[5] = descale(t5 + z2 + z4, sh);
  out[3] = descale(t6 + z2 + z3, sh);
  out[1] = descale(t7 + z1 + z4, sh);
}

// jcdctmgr.c forward_DCT's quantizer, sign(v) * ((|v| + q/2) / q), branch free: |v| through the sign mask, the quotient through
// the reciprocal (0 for |v| + q/2 < q by itself: a * ceil(2^32 / q) < 2^32 whenever a < q < 65536), the sign put back the same way
__device__ __forceinline__ int quantize(int v, uint32_t divisor, uint32_t reciprocal) {
  const int sgn = v >> 31;
  const uint32_t a = (uint32_t)((v ^ sgn) - sgn) + (divisor >> 1);
  const uint32_t q = __umulhi(a, reciprocal);
  return (int)(q ^ (uint32_t)sgn) - sgn;
}

// ---- quantisation tables -----------------------------------------------------------------------------------------------------
struct QuantTable {   // natural order
  uint32_t qv[64];    // divisors: quantval << 3
  uint32_t qm[64];    // their reciprocals: ceil(2^32 / qv)
};
struct QuantTables {  // what a colour JPEG needs
  QuantTable luma, chroma;
};
inline void fill_quant_table(const uint16_t* qt_host, QuantTable* t) {
  for (int i = 0; i < 64; i++) {
    t->qv[i] = (uint32_t)qt_host[i] << 3;
    t->qm[i] = (uint32_t)((0x100000000ull + t->qv[i] - 1) / t->qv[i]);
  }
}

// Where the column-pass lane (block cb, column cc) finds the {divisor, reciprocal} of row r -- a compile-time choice per kernel:
// QuantLds: the table's 64 pairs in LDS, read where they are used instead of living in 16 registers per table (map_blocks_kernel:
//   133 -> ~100 VGPRs).  stage_quant_tables fills uint2 s_q[2][64] (luma, chroma); the caller's __syncthreads() publishes it.
// QuantRegs: the lane's eight pairs, loaded from the kernel arguments before the tile loop (they never change).
struct QuantLds {
  const uint2* tab;
  __device__ __forceinline__ uint2 pair(int r, int cc) const { return tab[r * 8 + cc]; }
};
struct QuantRegs {
  uint32_t qv[8], qm[8];
  __device__ __forceinline__ QuantRegs(const QuantTable& t, int cc) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      qv[r] = t.qv[r * 8 + cc];
      qm[r] = t.qm[r * 8 + cc];
    }
  }
  __device__ __forceinline__ uint2 pair(int r, int) const { return uint2{qv[r], qm[r]}; }
};
__device__ __forceinline__ void stage_quant_tables(uint2 (*s_q)[64], const QuantTables& q, uint32_t tid) {
  if (tid < 128) {
    const QuantTable& t = tid < 64 ? q.luma : q.chroma;
    s_q[tid >> 6][tid & 63] = uint2{t.qv[tid & 63], t.qm[tid & 63]};
  }
}

// ---- the wave's LDS workspace: 8 blocks x 8 rows x 9 (padded) words ------------------------------------------------------------
constexpr int kWsWords = 8 * 8 * 9;
// Row role: lane (row rr, block rb) touches ws_at(rb, rr, 0..7).  Column role: lane (block cb, column cc) touches ws_at(cb, 0..7, cc).
__device__ __forceinline__ int ws_at(int block, int row, int col) { return block * 72 + row * 9 + col; }

// One wave, up to eight blocks: row pass results `row_out` of lane (row rr, block rb) -> transposed through the wave's workspace
// -> column pass + quantizer with lane (block cb, column cc) -> transposed back -> lane (rr, rb) holds one coefficient row of
// its block in v[0..7].  On return the workspace may be reused.
template <class Q>
__device__ __forceinline__ void column_pass_and_quantize(int* ws, int lane, const int row_out[8], const Q& q, int v[8]) {
  const int cb = lane >> 3, cc = lane & 7, rr = lane >> 3, rb = lane & 7;
  int in[8], out[8];
#pragma unroll
  for (int c = 0; c < 8; c++) ws[ws_at(rb, rr, c)] = row_out[c];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS writes of this wave have landed
#pragma unroll
  for (int r = 0; r < 8; r++) in[r] = ws[ws_at(cb, r, cc)];
  fdct_1d<1>(in, out);
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint2 qe = q.pair(r, cc);
    out[r] = quantize(out[r], qe.x, qe.y);
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 8; r++) ws[ws_at(cb, r, cc)] = out[r];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
  for (int c = 0; c < 8; c++) v[c] = ws[ws_at(rb, rr, c)];
  __builtin_amdgcn_wave_barrier();
}

// eight coefficients -> one 16-byte store
__device__ __forceinline__ void store_coef_row(int16_t* dst, const int v[8]) {
  uint4 o;
  o.x = (uint32_t)(v[0] & 0xffff) | ((uint32_t)v[1] << 16);
  o.y = (uint32_t)(v[2] & 0xffff) | ((uint32_t)v[3] << 16);
  o.z = (uint32_t)(v[4] & 0xffff) | ((uint32_t)v[5] << 16);
  o.w = (uint32_t)(v[6] & 0xffff) | ((uint32_t)v[7] << 16);
  *(uint4*)dst = o;
}

// eight packed bytes -> level-shifted samples
__device__ __forceinline__ void unpack8_level_shift(uint32_t lo, uint32_t hi, int in[8]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    in[c] = (int)((lo >> (8 * c)) & 0xff) - 128;
    in[4 + c] = (int)((hi >> (8 * c)) & 0xff) - 128;
  }
}

// jccolor.c rgb_ycc_convert of one pixel (jpeg_decode.hip: both published constant sets give these bytes), level-shifted into
// sample k of the three components
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }
__device__ __forceinline__ void rgb_ycc_level_shift(int r, int g, int b, int (&comp)[3][8], int k) {
  const int half = 1 << 15, off = 128 << 16;
  comp[0][k] = ((__mul24(fix16(0.29900), r) + __mul24(fix16(0.58700), g) + __mul24(fix16(0.11400), b) + half) >> 16) - 128;
  comp[1][k] = ((__mul24(-fix16(0.16874), r) + __mul24(-fix16(0.33126), g) + __mul24(fix16(0.50000), b) + off + half - 1) >> 16) - 128;
  comp[2][k] = ((__mul24(fix16(0.50000), r) + __mul24(-fix16(0.41869), g) + __mul24(-fix16(0.08131), b) + off + half - 1) >> 16) - 128;
}

// The NCH transforms of a strip of eight horizontally adjacent blocks on a bw-block-wide coefficient grid: lane (row lane / 8,
// block bx) holds the level-shifted samples of its row of each component in comp; `active`: the lane's block exists (bx < bw) --
// inactive lanes take part in the transposes only.  Luma table for component 0, chroma table for the others.
template <int NCH, class Q>
__device__ __forceinline__ void strip_transform(const int (&comp)[3][8], bool active, int16_t* const coef[3], int bw, int by, int bx, int lane, int* ws,
                                                const Q& luma, const Q& chroma) {
#pragma unroll
  for (int ci = 0; ci < NCH; ci++) {
    int out[8], v[8];
    if (active) {
      fdct_1d<0>(comp[ci], out);
    } else {
#pragma unroll
      for (int c = 0; c < 8; c++) out[c] = 0;
    }
    column_pass_and_quantize(ws, lane, out, ci == 0 ? luma : chroma, v);
    if (active) store_coef_row(coef[ci] + ((size_t)by * bw + bx) * 64 + (lane >> 3) * 8, v);
  }
}

}  // namespace fdct
}  // namespace uhdr
