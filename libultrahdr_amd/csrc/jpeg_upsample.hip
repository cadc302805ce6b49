// 4:2:0 and 4:2:2 JPEG (2x2 or 2x1 / 1x1 / 1x1) -> packed RGB888 / RGBA8888 on gfx950, libjpeg-exact (what
// JpegDecoderHelper::decompressImage returns for DECODE_TO_RGB_CS, jpegdecoderhelper.cpp:349-375, jpeg_read_scanlines of a YCbCr
// file of that sampling).  VSAMP is the luma vertical sampling factor: 2 for 4:2:0, 1 for 4:2:2.  The two libjpeg families
// rebuild the chroma differently (tests/upsample_port.py and tests/upsample422_port.py restate both in numpy):
//   variant 0, libjpeg-turbo (jdsample.c): 8x8 islow IDCT of the chroma blocks, then fancy upsampling; the context rows /
//     columns replicate the last REAL chroma row / column, i.e. the neighbour's index is clamped to the ceil(w/2) [x ceil(h/2)]
//     real samples.  ceil(w/2) <= 2: plain replication (h2v2_upsample / h2v1_upsample).
//       4:2:0, h2v2_fancy_upsample: each chroma sample becomes 2x2 output samples: colsum = 3 near + far (far: the chroma row
//         above / below), left output (3 this + left + 8) >> 4, right (3 this + right + 7) >> 4.
//       4:2:2, h2v1_fancy_upsample: two output samples of the same row, left (3 this + left + 1) >> 2, right
//         (3 this + right + 2) >> 2; no vertical mixing.
//   variant 1, IJG libjpeg 9 (jdmaster.c, jidctint.c jpeg_idct_16x16 / jpeg_idct_16x8): with do_fancy_upsampling each 8x8
//     chroma block is rebuilt as 16x16 (4:2:0) or 16 wide x 8 high (4:2:2) samples by the scaled islow IDCT and the upsampler
//     is 1:1 -- no context across blocks.
// Both then run ycc_rgb_convert with their family's green constants (upsample_core.h).
//
// Mapping: one wavefront = a tile of 32 x 16 pixels: two horizontally adjacent 16x16 MCUs (4:2:0) or 2 x 2 MCUs of 16x8
// (4:2:2).  Its eight luma blocks go through the shared islow wave IDCT (idct_core.h); the samples are parked in LDS as three
// 16 x 32 byte tiles (Y, Cb, Cr), and lane (row r, segment s) converts and stores pixels [s*8, s*8+8) of row r: 32 (24)
// contiguous bytes per lane, a row of a tile in four lanes.
//   variant 1: the chroma blocks of the tile (Cb and Cr) are transformed inside the wave into the tiles.  4:2:0, four blocks:
//     column pass on 32 lanes (one column of one block each, 16 outputs), row pass on 64 lanes (one of 16 rows of one block).
//     4:2:2, eight blocks, all 64 lanes busy in both passes: the 8-point column pass on (block, column), the 16-point row pass
//     on (block, row).
//   variant 0: the chroma needs one sample of context across MCU edges; the 8x8 chroma planes come from idct_dequant_kernel
//     (jpeg_decode.hip) through HBM (0.5 B/px written and read for 4:2:0, 1 B/px for 4:2:2), and the lane reads its 6 samples
//     of each chroma row it needs (two for 4:2:0, ONE for 4:2:2) with clamped indices.
#include "coef_tile.h"
#include "uhdr_types.h"
#include "upsample_core.h"

namespace uhdr {
namespace {

using namespace idct;
using namespace upsample;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct UpsampleArgs {
  const int16_t* coef[3];
  const uint8_t* cplane[2];  // variant 0: the 8x8-IDCT chroma planes (pitch cpitch)
  uint8_t* rgb;
  size_t pitch;              // output row pitch, bytes
  size_t cpitch;
  uint32_t w, h;             // pixels stored
  int bw[3], bh[3];          // block grids as stored (libjpeg's width_in_blocks or up to MCU-padded)
  int tiles_x, tiles_y;      // 32 x 16 pixel tiles
  int cw, ch;                // real chroma samples: ceil(w/2), ceil(h/2) (4:2:0) or h (4:2:2)
  int box;                   // variant 0: ceil(w/2) <= 2 -> h2v2_upsample / h2v1_upsample
  int k_cr_g, k_cb_g;
  uint16_t q[3][64];         // natural order
};

struct WaveLds {
  int ws[8 * 8 * 9];               // 8 blocks x 8 x 9 words: luma, then the chroma passes (variant 1)
  uint8_t tile[3][16][32];         // Y, Cb, Cr of the tile
};

// the 16-point row pass of one chroma block row from its eight workspace words, as 16 bytes of a tile row
__device__ __forceinline__ void chroma_row_pass(const int* wsrow, uint8_t* dst) {
  int in[8], out[16];
#pragma unroll
  for (int c = 0; c < 8; c++) in[c] = wsrow[c];
  idct16_1d<false, int>(in, out);
  uint32_t wds[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    wds[k] = (uint32_t)out[4 * k] | ((uint32_t)out[4 * k + 1] << 8) | ((uint32_t)out[4 * k + 2] << 16) | ((uint32_t)out[4 * k + 3] << 24);
  *(uint4*)dst = make_uint4(wds[0], wds[1], wds[2], wds[3]);
}

// variant 1, 4:2:0: the four 16x16 IDCTs of tile (ty, tx) (MCU m = blk >> 1, component 1 + (blk & 1)) into tile[1], tile[2]
__device__ __forceinline__ void chroma_idct_16x16(const UpsampleArgs& a, WaveLds& L, int lane, int ty, int tx) {
  const int lb = lane >> 3, lr = lane & 7;   // load / column-pass role: (block, row | column) on lanes 0..31
  const int cm = lb >> 1, cc = lb & 1;
  int v[8];
  int big = 0;
  if (lane < 32) {
    int q[8];
#pragma unroll
    for (int c = 0; c < 8; c++) q[c] = a.q[1 + cc][lr * 8 + c];
    load_dequant_row(a.coef[1 + cc], a.bw[1 + cc], ty, tx * 2 + cm, lr, q, v, big, ty < a.bh[1 + cc]);
  }
  // pass 1 is exact in 32 bits when every dequantized input is below 2^11 in magnitude: the sums stay below 2^31
  int mx = 0;
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < 8; c++) mx = max(mx, abs(v[c]));
  }
  const bool fast = __builtin_amdgcn_ballot_w64(mx > 2047) == 0;
  wave_sync();
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < 8; c++) L.ws[lb * 72 + lr * 9 + c] = v[c];
  }
  wave_sync();
  int in[8], out[16];
  if (lane < 32) {
#pragma unroll
    for (int r = 0; r < 8; r++) in[r] = L.ws[lb * 72 + r * 9 + lr];
    if (fast) idct16_1d<true, int>(in, out); else idct16_1d<true, long long>(in, out);
  }
  wave_sync();
  if (lane < 32) {
#pragma unroll
    for (int r = 0; r < 16; r++) L.ws[lb * 144 + r * 9 + lr] = out[r];
  }
  wave_sync();
  const int pb = lane >> 4, pr = lane & 15;  // row-pass role: (block, row)
  chroma_row_pass(&L.ws[pb * 144 + pr * 9], &L.tile[1 + (pb & 1)][pr][(pb >> 1) * 16]);
}

// variant 1, 4:2:2: the eight 16x8 IDCTs of tile (ty, tx), Cb and Cr of 2 x 2 MCUs, into tile[1], tile[2].  Lane roles as in
// idct_wave: (row rr, block rb) for loads and row passes, (block rr, column rb) for the column pass
__device__ __forceinline__ void chroma_idct_16x8(const UpsampleArgs& a, WaveLds& L, int rr, int rb, int ty, int tx) {
  const int cc = rb >> 2, cby = (rb >> 1) & 1, cbx = rb & 1;  // chroma block rb: component 1 + cc, block (cby, cbx) of the tile
  int qc[8];
#pragma unroll
  for (int c = 0; c < 8; c++) qc[c] = a.q[1 + cc][rr * 8 + c];
  const int by = ty * 2 + cby, bx = tx * 2 + cbx;
  int v[8];
  int big = 0;
  load_dequant_row(a.coef[1 + cc], a.bw[1 + cc], by, bx, rr, qc, v, big, by < a.bh[1 + cc]);
  const bool fast = __builtin_amdgcn_ballot_w64(big != 0) == 0;  // wave-uniform; the bound: idct8_columns_exact
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
  chroma_row_pass(&L.ws[rb * 72 + rr * 9], &L.tile[1 + cc][cby * 8 + rr][cbx * 16]);
}

// variant 0, 4:2:0: Cb, Cr of pixels [x0, x0 + 8) of row y from the chroma planes (h2v2_fancy_upsample / h2v2_upsample)
__device__ __forceinline__ void chroma_h2v2(const UpsampleArgs& a, uint32_t y, uint32_t x0, uint32_t cb[8], uint32_t cr[8]) {
  const int cy = (int)(y >> 1);
  const int fy = min(max(cy + ((y & 1) ? 1 : -1), 0), a.ch - 1);
  const int cx0 = (int)(x0 >> 1);
#pragma unroll
  for (int comp = 0; comp < 2; comp++) {
    const uint8_t* pn = a.cplane[comp] + (size_t)cy * a.cpitch;
    const uint8_t* pf = a.cplane[comp] + (size_t)fy * a.cpitch;
    int cs[6];  // column sums of chroma columns cx0 - 1 .. cx0 + 4 (clamped to the real samples)
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int cx = min(max(cx0 - 1 + k, 0), a.cw - 1);
      cs[k] = 3 * (int)pn[cx] + (int)pf[cx];
    }
    uint32_t* dst = comp ? cr : cb;
    if (a.box) {
#pragma unroll
      for (int k = 0; k < 4; k++) dst[2 * k] = dst[2 * k + 1] = pn[min(cx0 + k, a.cw - 1)];
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        dst[2 * k] = (uint32_t)((3 * cs[k + 1] + cs[k] + 8) >> 4);
        dst[2 * k + 1] = (uint32_t)((3 * cs[k + 1] + cs[k + 2] + 7) >> 4);
      }
    }
  }
}

// variant 0, 4:2:2: the same from the one chroma row y (h2v1_fancy_upsample / h2v1_upsample)
__device__ __forceinline__ void chroma_h2v1(const UpsampleArgs& a, uint32_t y, uint32_t x0, uint32_t cb[8], uint32_t cr[8]) {
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

template <int BPP, int VARIANT, int VSAMP>
__global__ __launch_bounds__(kBlock) void idct_upsample_rgb_kernel(const UpsampleArgs a) {
  __shared__ WaveLds s_lds[kWaves];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  WaveLds& L = s_lds[wv];
  const int total = a.tiles_x * a.tiles_y;
  const int gwave = blockIdx.x * kWaves + wv, nwaves = gridDim.x * kWaves;
  const int rr = lane >> 3, rb = lane & 7;        // IDCT roles: (row, block) for loads and row passes, (block rr, column rb) for column passes
  const int lby = rb >> 2, lbx = rb & 3;          // luma block rb: block row lby, block column lbx of the tile
  int ql[8];
#pragma unroll
  for (int c = 0; c < 8; c++) ql[c] = a.q[0][rr * 8 + c];
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
      *(uint2*)&L.tile[0][lby * 8 + rr][lbx * 8] = coef_tile::pack8(s);
    }
    if constexpr (VARIANT == 1) {
      if constexpr (VSAMP == 2) chroma_idct_16x16(a, L, lane, ty, tx);
      else chroma_idct_16x8(a, L, rr, rb, ty, tx);
    }
    wave_sync();
    // ---- colour conversion + store: lane (row, segment) ----
    const uint32_t y = (uint32_t)(ty * 16 + orow), x0 = (uint32_t)(tx * 32 + oseg * 8);
    if (y < a.h && x0 < a.w) {
      uint32_t ys[8], cb[8], cr[8];
      unpack8(*(const uint2*)&L.tile[0][orow][oseg * 8], ys);
      if constexpr (VARIANT == 1) {
        unpack8(*(const uint2*)&L.tile[1][orow][oseg * 8], cb);
        unpack8(*(const uint2*)&L.tile[2][orow][oseg * 8], cr);
      } else if constexpr (VSAMP == 2) {
        chroma_h2v2(a, y, x0, cb, cr);
      } else {
        chroma_h2v1(a, y, x0, cb, cr);
      }
      uint32_t px[8];
#pragma unroll
      for (int c = 0; c < 8; c++) px[c] = ycc_px(ys[c], cb[c], cr[c], a.k_cr_g, a.k_cb_g);
      store_px8<BPP>(a.rgb + (size_t)y * a.pitch + (size_t)x0 * BPP, px, x0, a.w, vec_ok);
    }
    wave_sync();  // the tiles are rewritten by the next iteration
  }
}

}  // namespace

// chroma_scratch of launch_idct_upsample_rgb, variant 0 only: the two 8x8-IDCT chroma planes
size_t upsample_scratch_bytes(const int bw[3], const int bh[3]) {
  const size_t p1 = (((size_t)bw[1] * 8 + 63) & ~(size_t)63) * (size_t)bh[1] * 8;
  const size_t p2 = (((size_t)bw[2] * 8 + 63) & ~(size_t)63) * (size_t)bh[2] * 8;
  return p1 + p2;
}

// vsamp 1: the chroma grids hold at least the real samples, ceil(w/2) x h (the caller checks): variant 0 reads the planes there.
hipError_t launch_idct_upsample_rgb(const int16_t* const coef[3], const int bw[3], const int bh[3], const uint16_t* const qt_host[3],
                                    int variant, int vsamp, const ImageViewMut& rgb, uint8_t* chroma_scratch, hipStream_t s) {
  UpsampleArgs a = {};
  const int bpp = rgb.fmt == UHDR_IMG_FMT_32bppRGBA8888 ? 4 : 3;
  a.rgb = (uint8_t*)rgb.p[0];
  a.pitch = (size_t)rgb.stride[0] * bpp;
  a.w = rgb.w; a.h = rgb.h;
  for (int c = 0; c < 3; c++) {
    a.coef[c] = coef[c]; a.bw[c] = bw[c]; a.bh[c] = bh[c];
    for (int i = 0; i < 64; i++) a.q[c][i] = qt_host[c][i];
  }
  a.tiles_x = (int)((rgb.w + 31) / 32); a.tiles_y = (int)((rgb.h + 15) / 16);
  a.cw = (int)((rgb.w + 1) / 2); a.ch = (int)((rgb.h + vsamp - 1) / vsamp);
  a.box = a.cw <= 2;
  ycc_green_constants(variant, &a.k_cr_g, &a.k_cb_g);
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
  using K = void (*)(const UpsampleArgs);
  static const K kernels[2][2][2] = {  // [bpp == 4][variant][vsamp == 2]
      {{idct_upsample_rgb_kernel<3, 0, 1>, idct_upsample_rgb_kernel<3, 0, 2>}, {idct_upsample_rgb_kernel<3, 1, 1>, idct_upsample_rgb_kernel<3, 1, 2>}},
      {{idct_upsample_rgb_kernel<4, 0, 1>, idct_upsample_rgb_kernel<4, 0, 2>}, {idct_upsample_rgb_kernel<4, 1, 1>, idct_upsample_rgb_kernel<4, 1, 2>}}};
  const uint32_t waves = (uint32_t)a.tiles_x * (uint32_t)a.tiles_y;
  const int grid = resident_grid((waves + kWaves - 1) / kWaves, 8);
  hipLaunchKernelGGL(kernels[bpp == 4][variant != 0][vsamp == 2], dim3(grid), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace uhdr
