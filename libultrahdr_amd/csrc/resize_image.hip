// resize_image on gfx950: the reference's interpolating resize (editorhelper.cpp:88-146), which UltraHdr::applyGainMap runs on
// a gain map whose aspect ratio differs from the base image's (jpegr.cpp:1651-1671).  8bppYCbCr400, 24bppRGB888 and
// 32bppRGBA8888; the arithmetic is resize_core.h's.
//
// A lane owns a run of kRun = 4 consecutive destination pixels of one row -- one dword of a Y400 row, three dwords of an
// RGB888 row, 16 bytes of an RGBA8888 row -- so a wave's stores are consecutive; a workgroup walks tiles of 256 x 4 pixels of
// one row.  The x side of a pixel (p0.x, p1.x, the four weights: ~15 FP64 operations) is computed once per column and
// serves every channel; the four neighbours are gathered from the source, which is a gain map: small, re-read by every
// destination row that maps onto it, resident in L2.  Per channel the blend is 7 FP64 operations, so the kernel is bound by
// its stores, not by the FP64 rate.  Rows whose address or pitch does not allow the wide store take byte / dword stores.
#include "resize_core.h"
#include "uhdr_types.h"

namespace uhdr {
namespace {

constexpr uint32_t kRun = 4;
constexpr uint32_t kTileW = 256u * kRun;

// BPP: bytes per pixel (1 Y400, 3 RGB888, 4 RGBA8888); the colour channels are the first min(BPP, 3) bytes
template <int BPP>
__global__ __launch_bounds__(256) void resize_image_kernel(const ResizePlane p) {
  constexpr int NCH = BPP == 1 ? 1 : 3;
  // get_pixel's normalisation of a byte: getYuv400Pixel multiplies by (1 / 255.0f), getRgb888Pixel / getRgba8888Pixel divide
  // by 255.0f (gainmapmath.cpp:389-396, 450-470) -- not the same float for every byte.  The quotient is taken in double and
  // rounded once more: for float operands that equals the correctly rounded float quotient.
  __shared__ float s_norm[256];
  s_norm[threadIdx.x] = BPP == 1 ? (float)threadIdx.x * (1 / 255.0f) : (float)((double)threadIdx.x / 255.0);
  __syncthreads();
  const uint8_t* __restrict__ src = (const uint8_t*)p.src;
  uint8_t* __restrict__ dst = (uint8_t*)p.dst;
  const uint32_t tiles_x = (p.dst_w + kTileW - 1) / kTileW, tiles = tiles_x * p.rows;
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t i = t / tiles_x, j = (t - i * tiles_x) * kTileW + threadIdx.x * kRun;
    if (j >= p.dst_w) continue;
    double unused;
    const ResizeAxis ry = resize_axis(i + p.y0, p.scale_y, p.src_h, &unused);
    const uint8_t* r0 = src + (size_t)ry.lo * p.src_pitch;
    const uint8_t* r1 = src + (size_t)ry.hi * p.src_pitch;
    const uint32_t n = p.dst_w - j < kRun ? p.dst_w - j : kRun;
    uint8_t out[kRun * BPP];
#pragma unroll
    for (uint32_t k = 0; k < kRun; k++) {
      // a column beyond the row's end repeats the last one: computed, never stored
      const uint32_t x = j + (k < n ? k : n - 1);
      double frac;
      const ResizeAxis rx = resize_axis(x, p.scale_x, p.src_w, &frac);
      const ResizeWeights w = resize_weights(frac);
      const uint32_t a = rx.lo * BPP, b = rx.hi * BPP;
#pragma unroll
      for (int c = 0; c < NCH; c++)
        out[k * BPP + c] = (uint8_t)resize_byte(w, s_norm[r0[a + c]], s_norm[r0[b + c]], s_norm[r1[a + c]], s_norm[r1[b + c]]);
      if (BPP == 4) out[k * BPP + 3] = 255;  // putRgba8888Pixel: alpha 1.0
    }
    uint8_t* q = dst + (size_t)i * p.dst_pitch + (size_t)j * BPP;
    if (n == kRun && ((uintptr_t)q % (BPP == 4 ? 16 : 4)) == 0) {
      uint32_t d[BPP];
#pragma unroll
      for (int m = 0; m < BPP; m++) d[m] = out[4 * m] | (out[4 * m + 1] << 8) | (out[4 * m + 2] << 16) | ((uint32_t)out[4 * m + 3] << 24);
      if (BPP == 1) *(uint32_t*)q = d[0];
      else if (BPP == 3) { ((uint32_t*)q)[0] = d[0]; ((uint32_t*)q)[1] = d[1]; ((uint32_t*)q)[2] = d[2]; }
      else *(uint4*)q = make_uint4(d[0], d[1 % BPP], d[2 % BPP], d[3 % BPP]);
    } else {
#pragma unroll
      for (uint32_t m = 0; m < kRun * BPP; m++)  // unrolled: `out` stays in registers
        if (m < n * BPP) q[m] = out[m];
    }
  }
}

}  // namespace

hipError_t launch_resize_image(const ResizePlane& p, int bpp, hipStream_t s) {
  const uint64_t tiles = (uint64_t)((p.dst_w + kTileW - 1) / kTileW) * p.rows;
  if (tiles == 0) return hipSuccess;
  if (tiles > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const int grid = (int)(tiles < 16384u ? tiles : 16384u);
  switch (bpp) {
    case 1: hipLaunchKernelGGL((resize_image_kernel<1>), dim3(grid), dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL((resize_image_kernel<3>), dim3(grid), dim3(256), 0, s, p); break;
    case 4: hipLaunchKernelGGL((resize_image_kernel<4>), dim3(grid), dim3(256), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace uhdr
