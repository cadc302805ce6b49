// 8x8 forward DCT + quantize on gfx950, bit-exact to libjpeg's JDCT_ISLOW path: the stand-alone kernels.
//
// The transform itself -- provenance, lane mapping, the reciprocal quantizer and the 24-bit multiply argument -- is
// fdct_core.h.  Here a wavefront takes 8 horizontally adjacent blocks (64 x 8 samples): lane (row rr = lane/8, block
// rb = lane%8) loads its 8 samples with one 8-byte load -- 8 consecutive lanes read 64 contiguous bytes -- and the wave
// writes 1 KiB of coefficients contiguous in libjpeg's JBLOCK order.  The lane's divisors and reciprocals live in registers.
// A wave keeps walking tiles (grid = resident waves) so the set-up is paid once.
#include <string.h>

#include "cu_count.h"
#include "fdct_core.h"
#include "uhdr_types.h"

namespace uhdr {
using namespace fdct;
namespace {

constexpr int kBlock = 256;  // 4 waves = 32 blocks per workgroup iteration

// The eight samples of row y, columns x0 .. x0 + 7 of a block that reaches beyond the plane's w x h valid samples, by
// JpegEncoderHelper::compressYCbCr's rules (jpegencoderhelper.cpp:246-309; FdctEdge in uhdr_types.h):
//   the caller's row pitch covers the block-aligned width (col_mode 0): columns >= w are the bytes that sit there (the
//     helper hands libjpeg pointers into the caller's rows), rows >= h are a constant row of `fill` (mPlanesMCURow);
//   it does not (col_mode 1): the helper copies every row into a scratch MCU row whose tail is `fill`; rows >= h are never
//     written, they still hold what the PREVIOUS MCU row copied there -- row y - mcu_rows of the plane (zeros in the first).
//   col_mode 2 is col_mode 0 for a plane the library allocated itself (API-0: uhdr_raw_image_ext_t zero-fills, stride ALIGN(w, 64)):
//     columns >= w are 0 whatever the component, and nothing is loaded there -- the device copy's bytes behind the width are not the
//     allocation's; rows >= h are the constant `fill` row.
__device__ __forceinline__ void load8_edge(const uint8_t* plane, size_t stride, int x0, int y, const FdctEdge& e, int in[8]) {
  int ys = y;
  bool row_const = false;
  if (y >= e.h) {
    if (e.col_mode != 1) row_const = true;
    else ys = y - e.mcu_rows;
  }
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int x = x0 + c;
    int v;
    if (row_const) v = e.fill;
    else if (x >= e.w) v = e.col_mode == 0 ? (int)plane[(size_t)ys * stride + x] : (e.col_mode == 2 ? 0 : e.fill);
    else v = ys < 0 ? 0 : (int)plane[(size_t)ys * stride + x];
    in[c] = v - 128;
  }
}

__global__ __launch_bounds__(kBlock) void fdct_quant_kernel(const uint8_t* __restrict__ plane,
                                                            size_t stride, int bw, int bh,
                                                            const QuantTable qa,
                                                            int16_t* __restrict__ coef, const FdctEdge edge) {
  __shared__ int s_ws[kBlock / 64][kWsWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* ws = s_ws[wv];
  const int groups_x = (bw + 7) >> 3;              // groups of 8 blocks per block-row
  const int total = groups_x * bh;
  const int gwave = blockIdx.x * (kBlock / 64) + wv;
  const int nwaves = gridDim.x * (kBlock / 64);
  const QuantRegs q(qa, lane & 7);
  const int rr = lane >> 3, rb = lane & 7;  // row-pass / store role: lane = (row rr, block rb)

  for (int t = gwave; t < total; t += nwaves) {
    const int by = t / groups_x, gx = t - by * groups_x;
    const int bx = gx * 8 + rb;
    int in[8], out[8], v[8];
    if (bx < bw && edge.on && (bx * 8 + 8 > edge.w || by * 8 + 8 > edge.h)) {  // a partial block of the right / bottom edge
      load8_edge(plane, stride, bx * 8, by * 8 + rr, edge, in);
      fdct_1d<0>(in, out);
    } else if (bx < bw) {
      const uint8_t* src = plane + (size_t)(by * 8 + rr) * stride + (size_t)bx * 8;
      uint32_t lo, hi;
      if (((uintptr_t)src & 3) == 0) {
        lo = ((const uint32_t*)src)[0];
        hi = ((const uint32_t*)src)[1];
      } else {
        lo = src[0] | (src[1] << 8) | (src[2] << 16) | ((uint32_t)src[3] << 24);
        hi = src[4] | (src[5] << 8) | (src[6] << 16) | ((uint32_t)src[7] << 24);
      }
      unpack8_level_shift(lo, hi, in);
      fdct_1d<0>(in, out);
    } else {
#pragma unroll
      for (int c = 0; c < 8; c++) out[c] = 0;
    }
    column_pass_and_quantize(ws, lane, out, q, v);
    if (bx < bw) store_coef_row(coef + ((size_t)by * bw + bx) * 64 + rr * 8, v);
  }
}

// ---- 3-channel gain map: libjpeg's JCS_RGB -> YCbCr conversion + FDCT + quantize in one pass -----------------
// What jpeg_write_scanlines does to an RGB888 gain map (jpegencoderhelper.cpp:165-167, 212-225): jccolor.c
// rgb_ycc_convert, then the islow FDCT and the quantizer per component (luma table for Y, chroma table for
// Cb / Cr, 4:4:4).  Unfused that is uhdr_hip_jpeg_rgb_to_ycc (3 B in, 3 B out) followed by three
// uhdr_hip_fdct_quant launches (1 B in, 2 B out each): 15 B/px.  Here a lane reads its 8 pixels once
// (24 or 32 bytes), converts them in registers and runs the three transforms back to back through the same
// LDS workspace: 3 (4) B/px in, 6 B/px out.
template <int BPP>
__global__ __launch_bounds__(kBlock) void fdct_quant_rgb_kernel(const uint8_t* __restrict__ rgb, size_t pitch /* bytes */, int bw, int bh,
                                                                const QuantTables qa, int16_t* __restrict__ coef_y,
                                                                int16_t* __restrict__ coef_cb, int16_t* __restrict__ coef_cr, int vw, int vh) {
  // vw x vh: the image's valid pixels.  Blocks that reach beyond them repeat the last column / row -- what libjpeg's
  // jpeg_write_scanlines pipeline does to an RGB gain map (jcsample.c expand_right_edge, jcprepct.c expand_bottom_edge;
  // the colour conversion is per pixel, so replicating before or after it is the same).
  __shared__ int s_ws[kBlock / 64][kWsWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* ws = s_ws[wv];
  const int groups_x = (bw + 7) >> 3, total = groups_x * bh;
  const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);
  const int rr = lane >> 3, rb = lane & 7;  // row-pass / store role
  const QuantRegs qy(qa.luma, lane & 7), qc(qa.chroma, lane & 7);
  int16_t* const coef[3] = {coef_y, coef_cb, coef_cr};
  for (int t = gwave; t < total; t += nwaves) {
    const int by = t / groups_x, gx = t - by * groups_x;
    const int bx = gx * 8 + rb;
    int comp[3][8];
    const bool partial = bx * 8 + 8 > vw || by * 8 + 8 > vh;
    if (bx < bw && partial) {
      const int y = min(by * 8 + rr, vh - 1);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint8_t* q = rgb + (size_t)y * pitch + (size_t)min(bx * 8 + k, vw - 1) * BPP;
        rgb_ycc_level_shift(q[0], q[1], q[2], comp, k);
      }
    } else if (bx < bw) {
      const uint8_t* src = rgb + (size_t)(by * 8 + rr) * pitch + (size_t)bx * 8 * BPP;
      uint32_t w[2 * BPP];
      if constexpr (BPP == 4) {
        const uint4 a = ((const uint4*)src)[0], b = ((const uint4*)src)[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      } else {
        const uint2 a = ((const uint2*)src)[0], b = ((const uint2*)src)[1], c = ((const uint2*)src)[2];
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y; w[4] = c.x; w[5] = c.y;
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        int r, g, b;
        if constexpr (BPP == 4) {
          r = w[k] & 0xff; g = (w[k] >> 8) & 0xff; b = (w[k] >> 16) & 0xff;
        } else {  // byte 3k, 3k+1, 3k+2 of the 24-byte run
          auto byte_at = [&](int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xff); };
          r = byte_at(3 * k); g = byte_at(3 * k + 1); b = byte_at(3 * k + 2);
        }
        rgb_ycc_level_shift(r, g, b, comp, k);
      }
    }
    strip_transform<3>(comp, bx < bw, coef, bw, by, bx, lane, ws, qy, qc);
  }
}

}  // namespace

hipError_t launch_fdct_quant(const uint8_t* plane, size_t stride, int bw, int bh,
                             const uint16_t* qt_host, int16_t* coef, hipStream_t s, const FdctEdge* edge) {
  FdctEdge e;
  memset(&e, 0, sizeof e);
  if (edge) e = *edge;
  QuantTable qa;
  fill_quant_table(qt_host, &qa);
  const int total = ((bw + 7) / 8) * bh;
  const int cus = device_cu_count();
  int grid = (total + 3) / 4;
  if (grid > cus * 8) grid = cus * 8;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(fdct_quant_kernel, dim3(grid), dim3(kBlock), 0, s, plane, stride, bw, bh, qa, coef, e);
  return hipGetLastError();
}

// bpp 3 (RGB888) or 4 (RGBA8888, alpha ignored); pitch in bytes; rows and base 8- (bpp 3) / 16-byte (bpp 4) aligned
hipError_t launch_fdct_quant_rgb(const uint8_t* rgb, size_t pitch, int bpp, int bw, int bh, const uint16_t* qt_luma_host,
                                 const uint16_t* qt_chroma_host, int16_t* coef_y, int16_t* coef_cb, int16_t* coef_cr, hipStream_t s, int vw, int vh) {
  if (vw <= 0) vw = bw * 8;
  if (vh <= 0) vh = bh * 8;
  QuantTables qa;
  fill_quant_table(qt_luma_host, &qa.luma);
  fill_quant_table(qt_chroma_host, &qa.chroma);
  const int total = ((bw + 7) / 8) * bh;
  const int cus = device_cu_count();
  int grid = (total + 3) / 4;
  if (grid > cus * 6) grid = cus * 6;
  if (grid < 1) grid = 1;
  if (bpp == 4) hipLaunchKernelGGL((fdct_quant_rgb_kernel<4>), dim3(grid), dim3(kBlock), 0, s, rgb, pitch, bw, bh, qa, coef_y, coef_cb, coef_cr, vw, vh);
  else hipLaunchKernelGGL((fdct_quant_rgb_kernel<3>), dim3(grid), dim3(kBlock), 0, s, rgb, pitch, bw, bh, qa, coef_y, coef_cb, coef_cr, vw, vh);
  return hipGetLastError();
}

}  // namespace uhdr
