// 4:2:2 JPEG (2x1 / 1x1 / 1x1) -> packed RGB888 / RGBA8888 on gfx950, libjpeg-exact (what JpegDecoderHelper::decompressImage
// returns for DECODE_TO_RGB_CS, jpegdecoderhelper.cpp:349-375, jpeg_read_scanlines of a YCbCr 4:2:2 file).  The two libjpeg
// families rebuild the chroma differently (tests/upsample422_port.py restates both in numpy):
//   variant 0, libjpeg-turbo (jdsample.c h2v1_fancy_upsample): 8x8 islow IDCT of the chroma blocks, then each chroma sample
//     becomes two output samples of the same row: left (3 this + left + 1) >> 2, right (3 this + right + 2) >> 2; the
//     context columns replicate the last REAL chroma column, i.e. the neighbour's index is clamped to 0 .. ceil(w/2) - 1.
//     No vertical mixing.  ceil(w/2) <= 2: plain replication (h2v1_upsample).
//   variant 1, IJG libjpeg 9 (jdmaster.c, jidctint.c jpeg_idct_16x8): with do_fancy_upsampling each 8x8 chroma block is
//     rebuilt as 16 x 8 samples by the scaled islow IDCT and the upsampler is 1:1 -- no context across blocks.
// Both then run ycc_rgb_convert with their family's green constants (jpeg_decode.hip).
//
// Mapping: one wavefront = 2 x 2 MCUs of 16 x 8 (32 x 16 pixels), the tile of the 4:2:0 kernel (jpeg_upsample.hip).  Its
// eight luma blocks go through the shared islow wave IDCT (idct_core.h); the samples are parked in LDS as three 16 x 32 byte
// tiles (Y, Cb, Cr), and lane (row r, segment s) converts and stores pixels [s*8, s*8+8) of row r: 32 (24) contiguous bytes
// per lane, a row of a tile in four lanes.
//   variant 1: the eight chroma blocks of the four MCUs (Cb and Cr) are transformed inside the wave with all 64 lanes busy
//     in both passes -- the 8-point column pass on (block, column), the 16-point row pass on (block, row) -- into the tiles.
//   variant 0: the chroma needs one sample of context across MCU edges; the 8x8 chroma planes come from
//     idct_dequant_kernel (jpeg_decode.hip) through HBM (1 B/px written and read), and the lane reads its 6 samples of the
//     ONE chroma row it needs with clamped indices.
#include "idct_core.h"
#include "uhdr_types.h"
#include "upsample_core.h"

namespace uhdr {
namespace {

using namespace idct;
using namespace upsample;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct Upsample422Args {
  const int16_t* coef[3];
  const uint8_t* cplane[2];  // variant 0: the 8x8-IDCT chroma planes (pitch cpitch)
  uint8_t* rgb;
  size_t pitch;              // output row pitch, bytes
  size_t cpitch;
  uint32_t w, h;             // pixels stored
  int bw[3], bh[3];          // block grids as stored (libjpeg's width_in_blocks or up to MCU-padded)
  int tiles_x, tiles_y;      // 32 x 16 pixel tiles
  int cw;                    // real chroma samples per row: ceil(w/2)
  int box;                   // variant 0: ceil(w/2) <= 2 -> h2v1_upsample
  int k_cr_g, k_cb_g;
  uint16_t q[3][64];         // natural order
};

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

struct WaveLds {
  int ws[8 * 8 * 9];               // 8 blocks x 8 x 9 words: luma, then chroma (variant 1)
  uint8_t tile[3][16][32];         // Y, Cb, Cr of the four MCUs
};

template <int BPP, int VARIANT>
__global__ __launch_bounds__(kBlock) void idct_upsample_rgb422_kernel(const Upsample422Args a) {
  __shared__ WaveLds s_lds[kWaves];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  WaveLds& L = s_lds[wv];
  const int total = a.tiles_x * a.tiles_y;
  const int gwave = blockIdx.x * kWaves + wv, nwaves = gridDim.x * kWaves;
  const int rr = lane >> 3, rb = lane & 7;        // IDCT roles: (row, block) for loads and row passes, (block rr, column rb) for column passes
  const int lby = rb >> 2, lbx = rb & 3;          // luma block rb: block row lby, block column lbx of the tile
  const int cc = rb >> 2, cby = (rb >> 1) & 1, cbx = rb & 1;  // chroma block rb: component 1 + cc, block (cby, cbx) of the tile
  int ql[8];
#pragma unroll
  for (int c = 0; c < 8; c++) ql[c] = a.q[0][rr * 8 + c];
  int qc[8];
  if constexpr (VARIANT == 1) {
#pragma unroll
    for (int c = 0; c < 8; c++) qc[c] = a.q[1 + cc][rr * 8 + c];
  }
  const int orow = lane >> 2, oseg = lane & 3;    // conversion: tile row, 8-pixel segment
  const bool vec_ok = ((a.pitch | (uintptr_t)a.rgb) & (BPP == 4 ? 15 : 7)) == 0;

  for (int t = gwave; t < total; t += nwaves) {
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    // ---- luma: 2 x 4 blocks ----
    {
      const int by = ty * 2 + lby, bx = tx * 4 + lbx;
      int v[8];
      int big = 0;
      load_dequant_row(a.coef[0], a.bw[0], by, bx, rr, ql, v, big, by < a.bh[0]);
      uint32_t s[8];
      idct_wave(L.ws, v, big, rr, rb, s);
      const uint32_t lo = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
      const uint32_t hi = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
      *(uint2*)&L.tile[0][lby * 8 + rr][lbx * 8] = make_uint2(lo, hi);
    }
    if constexpr (VARIANT == 1) {
      // ---- chroma: eight 16x8 IDCTs, Cb and Cr of 2 x 2 MCUs ----
      const int by = ty * 2 + cby, bx = tx * 2 + cbx;
      int v[8];
      int big = 0;
      load_dequant_row(a.coef[1 + cc], a.bw[1 + cc], by, bx, rr, qc, v, big, by < a.bh[1 + cc]);
      const bool fast = __builtin_amdgcn_ballot_w64(big != 0) == 0;  // wave-uniform
      wave_sync();  // idct_wave's last reads of ws
#pragma unroll
      for (int c = 0; c < 8; c++) L.ws[rb * 72 + rr * 9 + c] = v[c];
      wave_sync();
      int in[8], col[8];
#pragma unroll
      for (int r = 0; r < 8; r++) in[r] = L.ws[rr * 72 + r * 9 + rb];
      if (fast) idct_1d<0, true>(in, col); else idct8_columns_exact(in, col);
      wave_sync();
#pragma unroll
      for (int r = 0; r < 8; r++) L.ws[rr * 72 + r * 9 + rb] = col[r];
      wave_sync();
#pragma unroll
      for (int c = 0; c < 8; c++) in[c] = L.ws[rb * 72 + rr * 9 + c];
      int out[16];
      idct16_1d<false, int>(in, out);
      uint32_t wds[4];
#pragma unroll
      for (int k = 0; k < 4; k++)
        wds[k] = (uint32_t)out[4 * k] | ((uint32_t)out[4 * k + 1] << 8) | ((uint32_t)out[4 * k + 2] << 16) | ((uint32_t)out[4 * k + 3] << 24);
      *(uint4*)&L.tile[1 + cc][cby * 8 + rr][cbx * 16] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    }
    wave_sync();
    // ---- colour conversion + store: lane (row, segment) ----
    const uint32_t y = (uint32_t)(ty * 16 + orow), x0 = (uint32_t)(tx * 32 + oseg * 8);
    if (y < a.h && x0 < a.w) {
      const uint2 yv = *(const uint2*)&L.tile[0][orow][oseg * 8];
      uint32_t ys[8], cb[8], cr[8];
#pragma unroll
      for (int c = 0; c < 4; c++) { ys[c] = (yv.x >> (8 * c)) & 0xff; ys[4 + c] = (yv.y >> (8 * c)) & 0xff; }
      if constexpr (VARIANT == 1) {
        const uint2 bv = *(const uint2*)&L.tile[1][orow][oseg * 8];
        const uint2 rv = *(const uint2*)&L.tile[2][orow][oseg * 8];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          cb[c] = (bv.x >> (8 * c)) & 0xff; cb[4 + c] = (bv.y >> (8 * c)) & 0xff;
          cr[c] = (rv.x >> (8 * c)) & 0xff; cr[4 + c] = (rv.y >> (8 * c)) & 0xff;
        }
      } else {
        const int cx0 = (int)(x0 >> 1);
#pragma unroll
        for (int comp = 0; comp < 2; comp++) {
          const uint8_t* p = a.cplane[comp] + (size_t)y * a.cpitch;
          int cs[6];  // chroma columns cx0 - 1 .. cx0 + 4 (clamped to the real samples)
#pragma unroll
          for (int k = 0; k < 6; k++) cs[k] = (int)p[min(max(cx0 - 1 + k, 0), a.cw - 1)];
          uint32_t* dst = comp ? cr : cb;
          if (a.box) {
#pragma unroll
            for (int k = 0; k < 4; k++) dst[2 * k] = dst[2 * k + 1] = (uint32_t)cs[k + 1];
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
              dst[2 * k] = (uint32_t)((3 * cs[k + 1] + cs[k] + 1) >> 2);
              dst[2 * k + 1] = (uint32_t)((3 * cs[k + 1] + cs[k + 2] + 2) >> 2);
            }
          }
        }
      }
      uint32_t px[8];
#pragma unroll
      for (int c = 0; c < 8; c++) px[c] = ycc_px(ys[c], cb[c], cr[c], a.k_cr_g, a.k_cb_g);
      uint8_t* dst = a.rgb + (size_t)y * a.pitch + (size_t)x0 * BPP;
      if (vec_ok && x0 + 8 <= a.w) {
        if constexpr (BPP == 4) {
          *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]);
          *(uint4*)(dst + 16) = make_uint4(px[4], px[5], px[6], px[7]);
        } else {
          uint32_t d[6];
#pragma unroll
          for (int hh = 0; hh < 2; hh++) {
            const uint32_t* q4 = px + 4 * hh;
            d[3 * hh + 0] = (q4[0] & 0xffffff) | (q4[1] << 24);
            d[3 * hh + 1] = ((q4[1] >> 8) & 0xffff) | (q4[2] << 16);
            d[3 * hh + 2] = ((q4[2] >> 16) & 0xff) | (q4[3] << 8);
          }
          *(uint2*)dst = make_uint2(d[0], d[1]);
          *(uint2*)(dst + 8) = make_uint2(d[2], d[3]);
          *(uint2*)(dst + 16) = make_uint2(d[4], d[5]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 8; c++) {
          if (x0 + c < a.w) {
            dst[c * BPP] = (uint8_t)px[c]; dst[c * BPP + 1] = (uint8_t)(px[c] >> 8); dst[c * BPP + 2] = (uint8_t)(px[c] >> 16);
            if constexpr (BPP == 4) dst[c * BPP + 3] = 255;
          }
        }
      }
    }
    wave_sync();  // the tiles are rewritten by the next iteration
  }
}

int grid_for(uint32_t waves) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  const uint32_t blocks = (waves + kWaves - 1) / kWaves, r = (uint32_t)cus * 8;
  return (int)(blocks < r ? (blocks ? blocks : 1u) : r);
}

}  // namespace

// chroma_scratch: variant 0 only, at least upsample422_scratch_bytes() bytes of device memory for the two chroma planes
size_t upsample422_scratch_bytes(const int bw[3], const int bh[3]) {
  const size_t p1 = (((size_t)bw[1] * 8 + 63) & ~(size_t)63) * (size_t)bh[1] * 8;
  const size_t p2 = (((size_t)bw[2] * 8 + 63) & ~(size_t)63) * (size_t)bh[2] * 8;
  return p1 + p2;
}

// The chroma grids hold at least the real samples, ceil(w/2) x h (the caller checks): variant 0 reads the planes there.
hipError_t launch_idct_upsample_rgb422(const int16_t* const coef[3], const int bw[3], const int bh[3], const uint16_t* const qt_host[3],
                                       int variant, const ImageViewMut& rgb, uint8_t* chroma_scratch, hipStream_t s) {
  Upsample422Args a = {};
  const int bpp = rgb.fmt == UHDR_IMG_FMT_32bppRGBA8888 ? 4 : 3;
  a.rgb = (uint8_t*)rgb.p[0];
  a.pitch = (size_t)rgb.stride[0] * bpp;
  a.w = rgb.w; a.h = rgb.h;
  for (int c = 0; c < 3; c++) {
    a.coef[c] = coef[c]; a.bw[c] = bw[c]; a.bh[c] = bh[c];
    for (int i = 0; i < 64; i++) a.q[c][i] = qt_host[c][i];
  }
  a.tiles_x = (int)((rgb.w + 31) / 32); a.tiles_y = (int)((rgb.h + 15) / 16);
  a.cw = (int)((rgb.w + 1) / 2);
  a.box = a.cw <= 2;
  a.k_cr_g = variant ? FIX16(0.714136286) : FIX16(0.71414);
  a.k_cb_g = variant ? FIX16(0.344136286) : FIX16(0.34414);
  if (variant == 0) {
    size_t off = 0;
    for (int c = 1; c < 3; c++) {
      const size_t pitch = ((size_t)bw[c] * 8 + 63) & ~(size_t)63;
      // both chroma planes share one pitch (Cb and Cr grids are equal: the caller checks)
      a.cpitch = pitch;
      a.cplane[c - 1] = chroma_scratch + off;
      hipError_t e = launch_idct_dequant(coef[c], bw[c], bh[c], qt_host[c], chroma_scratch + off, pitch, s);
      if (e != hipSuccess) return e;
      off += pitch * (size_t)bh[c] * 8;
    }
  }
  const uint32_t waves = (uint32_t)a.tiles_x * (uint32_t)a.tiles_y;
  const int grid = grid_for(waves);
  if (variant == 0) {
    if (bpp == 4) hipLaunchKernelGGL((idct_upsample_rgb422_kernel<4, 0>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((idct_upsample_rgb422_kernel<3, 0>), dim3(grid), dim3(kBlock), 0, s, a);
  } else {
    if (bpp == 4) hipLaunchKernelGGL((idct_upsample_rgb422_kernel<4, 1>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((idct_upsample_rgb422_kernel<3, 1>), dim3(grid), dim3(kBlock), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace uhdr
