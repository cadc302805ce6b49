// 4:2:0 JPEG -> packed RGB888 / RGBA8888 on gfx950, libjpeg-exact (what JpegDecoderHelper::decompressImage returns for
// DECODE_TO_RGB_CS, jpegdecoderhelper.cpp:349-375, jpeg_read_scanlines of a YCbCr 4:2:0 file).  The two libjpeg families
// rebuild the chroma differently (tests/upsample_port.py restates both in numpy):
//   variant 0, libjpeg-turbo (jdsample.c h2v2_fancy_upsample): 8x8 islow IDCT of the chroma blocks, then each chroma sample
//     becomes 2x2 output samples: colsum = 3 near + far (far: the chroma row above / below), left output
//     (3 this + left + 8) >> 4, right (3 this + right + 7) >> 4; the context rows / columns replicate the last REAL chroma
//     row / column, i.e. the neighbour's index is clamped.  ceil(w/2) <= 2: plain 2x2 replication (h2v2_upsample).
//   variant 1, IJG libjpeg 9 (jdmaster.c, jidctint.c jpeg_idct_16x16): with do_fancy_upsampling each 8x8 chroma block is
//     rebuilt as 16x16 samples by the scaled islow IDCT and the upsampler is 1:1 -- no context across blocks.
// Both then run ycc_rgb_convert with their family's green constants (jpeg_decode.hip).
//
// Mapping: one wavefront = two horizontally adjacent MCUs (32 x 16 pixels).  Its eight luma blocks go through the shared
// islow wave IDCT (idct_core.h); the samples are parked in LDS as three 16 x 32 byte tiles (Y, Cb, Cr), and lane
// (row r, segment s) converts and stores pixels [s*8, s*8+8) of row r: 32 (24) contiguous bytes per lane, a row of a tile
// in four lanes.
//   variant 1: the four chroma blocks of the two MCUs (Cb, Cr) are transformed inside the wave -- column pass on 32 lanes
//     (one column of one block each, 16 outputs), row pass on 64 lanes (one of 16 rows of one block) -- into the tiles.
//   variant 0: the chroma needs one sample of context across MCU edges; the 8x8 chroma planes come from
//     idct_dequant_kernel (jpeg_decode.hip) through HBM (0.5 B/px written and read), and the lane reads its 6 + 6 samples
//     of the two chroma rows it needs with clamped indices.
#include "idct_core.h"
#include "uhdr_types.h"
#include "upsample_core.h"

namespace uhdr {
namespace {

using namespace idct;
using namespace upsample;  // wave_sync, idct16_1d (jidctint.c jpeg_idct_16x16's 16-point pass), ycc_px

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct Upsample420Args {
  const int16_t* coef[3];
  const uint8_t* cplane[2];  // variant 0: the 8x8-IDCT chroma planes (pitch cpitch)
  uint8_t* rgb;
  size_t pitch;              // output row pitch, bytes
  size_t cpitch;
  uint32_t w, h;             // pixels stored
  int bw[3], bh[3];          // block grids as stored (libjpeg's width_in_blocks or up to MCU-padded)
  int mcus_x, mcus_y;
  int cw, ch;                // real chroma samples: ceil(w/2), ceil(h/2)
  int box;                   // variant 0: ceil(w/2) <= 2 -> h2v2_upsample
  int k_cr_g, k_cb_g;
  uint16_t q[3][64];         // natural order
};

struct WaveLds {
  int ws[4 * 16 * 9];              // luma 8x8 workspace (8 x 8 x 9 words) / chroma 16-point workspace
  uint8_t tile[3][16][32];         // Y, Cb, Cr of the two MCUs
};

template <int BPP, int VARIANT>
__global__ __launch_bounds__(kBlock) void idct_upsample_rgb_kernel(const Upsample420Args a) {
  __shared__ WaveLds s_lds[kWaves];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  WaveLds& L = s_lds[wv];
  const int pairs_x = (a.mcus_x + 1) >> 1, total = pairs_x * a.mcus_y;
  const int gwave = blockIdx.x * kWaves + wv, nwaves = gridDim.x * kWaves;
  const int rr = lane >> 3, rb = lane & 7;        // luma: (row, block); block rb = MCU (rb >> 2), position (rb & 3)
  const int om = rb >> 2, oby = (rb >> 1) & 1, obx = rb & 1;
  int ql[8];
#pragma unroll
  for (int c = 0; c < 8; c++) ql[c] = a.q[0][rr * 8 + c];
  const int orow = lane >> 2, oseg = lane & 3;    // conversion: tile row, 8-pixel segment
  const bool vec_ok = ((a.pitch | (uintptr_t)a.rgb) & (BPP == 4 ? 15 : 7)) == 0;

  for (int t = gwave; t < total; t += nwaves) {
    const int my = t / pairs_x, mx0 = (t - my * pairs_x) * 2;
    // ---- luma: four blocks per MCU, eight per wave ----
    {
      const int by = my * 2 + oby, bx = (mx0 + om) * 2 + obx;
      int v[8];
      int big = 0;
      load_dequant_row(a.coef[0], a.bw[0], by, bx, rr, ql, v, big, by < a.bh[0]);
      uint32_t s[8];
      idct_wave(L.ws, v, big, rr, rb, s);
      const uint32_t lo = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
      const uint32_t hi = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
      *(uint2*)&L.tile[0][oby * 8 + rr][om * 16 + obx * 8] = make_uint2(lo, hi);
    }
    if constexpr (VARIANT == 1) {
      // ---- chroma: four 16x16 IDCTs (MCU m = blk >> 1, component 1 + (blk & 1)) ----
      const int lb = lane >> 3, lr = lane & 7;   // load / column-pass role: (block, row | column) on lanes 0..31
      const int cm = lb >> 1, cc = lb & 1;
      int v[8];
      int big = 0;
      if (lane < 32) {
        int q[8];
#pragma unroll
        for (int c = 0; c < 8; c++) q[c] = a.q[1 + cc][lr * 8 + c];
        load_dequant_row(a.coef[1 + cc], a.bw[1 + cc], my, mx0 + cm, lr, q, v, big, my < a.bh[1 + cc]);
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
      {
        const int pb = lane >> 4, pr = lane & 15;  // row-pass role: (block, row)
#pragma unroll
        for (int c = 0; c < 8; c++) in[c] = L.ws[pb * 144 + pr * 9 + c];
        idct16_1d<false, int>(in, out);
        uint32_t wds[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
          wds[k] = (uint32_t)out[4 * k] | ((uint32_t)out[4 * k + 1] << 8) | ((uint32_t)out[4 * k + 2] << 16) | ((uint32_t)out[4 * k + 3] << 24);
        *(uint4*)&L.tile[1 + (pb & 1)][pr][(pb >> 1) * 16] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
      }
    }
    wave_sync();
    // ---- colour conversion + store: lane (row, segment) ----
    const uint32_t y = (uint32_t)(my * 16 + orow), x0 = (uint32_t)(mx0 * 16 + oseg * 8);
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

// chroma_scratch: variant 0 only, at least upsample420_scratch_bytes() bytes of device memory for the two chroma planes
size_t upsample420_scratch_bytes(const int bw[3], const int bh[3]) {
  const size_t p1 = (((size_t)bw[1] * 8 + 63) & ~(size_t)63) * (size_t)bh[1] * 8;
  const size_t p2 = (((size_t)bw[2] * 8 + 63) & ~(size_t)63) * (size_t)bh[2] * 8;
  return p1 + p2;
}

hipError_t launch_idct_upsample_rgb(const int16_t* const coef[3], const int bw[3], const int bh[3], const uint16_t* const qt_host[3],
                                    int variant, const ImageViewMut& rgb, uint8_t* chroma_scratch, hipStream_t s) {
  Upsample420Args a = {};
  const int bpp = rgb.fmt == UHDR_IMG_FMT_32bppRGBA8888 ? 4 : 3;
  a.rgb = (uint8_t*)rgb.p[0];
  a.pitch = (size_t)rgb.stride[0] * bpp;
  a.w = rgb.w; a.h = rgb.h;
  for (int c = 0; c < 3; c++) {
    a.coef[c] = coef[c]; a.bw[c] = bw[c]; a.bh[c] = bh[c];
    for (int i = 0; i < 64; i++) a.q[c][i] = qt_host[c][i];
  }
  a.mcus_x = (int)((rgb.w + 15) / 16); a.mcus_y = (int)((rgb.h + 15) / 16);
  a.cw = (int)((rgb.w + 1) / 2); a.ch = (int)((rgb.h + 1) / 2);
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
  const uint32_t waves = (uint32_t)((a.mcus_x + 1) / 2) * (uint32_t)a.mcus_y;
  const int grid = grid_for(waves);
  if (variant == 0) {
    if (bpp == 4) hipLaunchKernelGGL((idct_upsample_rgb_kernel<4, 0>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((idct_upsample_rgb_kernel<3, 0>), dim3(grid), dim3(kBlock), 0, s, a);
  } else {
    if (bpp == 4) hipLaunchKernelGGL((idct_upsample_rgb_kernel<4, 1>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((idct_upsample_rgb_kernel<3, 1>), dim3(grid), dim3(kBlock), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace uhdr
