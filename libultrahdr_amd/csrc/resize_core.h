// resize_core.h -- the arithmetic of the reference's resize_image (editorhelper.cpp:88-146), shared by the stand-alone
// resize kernel (resize_image.hip) and the sampler inside the applyGainMap kernel (apply_gainmap.hip: sample_map_resized).
//
// For destination pixel (x, y) of a dst_w x dst_h image made from a src_w x src_h one:
//   ori_x = x * ((double)src_w / dst_w), ori_y = y * ((double)src_h / dst_h)
//   p0 = (floor(ori_x), floor(ori_y)) clipped to the source, p1 = right of p0, p2 = below p0, p3 = right of p2, each
//   clipped to the last column / row
//   t = ori_x - p0.x -- the vertical position takes no part in the weights (the reference's "bicubic" is a cubic Bernstein
//   blend of the four neighbours along x only)
//   result = w0*p0 + w1*p1 + w2*p2 + w3*p3 in double (products and sums left to right), cast to float, stored as
//   clip(v * 255.0f + 0.5f, 0, 255) truncated (putYuv400Pixel / putRgb888Pixel / putRgba8888Pixel, gainmapmath.cpp:538-577)
// Every step is one IEEE operation in source order (the library is built with -ffp-contract=off), so the bytes are the
// reference's bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uhdr {

struct ResizeAxis {
  uint32_t lo, hi;  // p0's and p1's column (or p0's and p2's row)
};
struct ResizeWeights {
  double w0, w1, w2, w3;
};

// p0 / p0 + 1 along one axis, and the position's distance from p0 (meaningful along x only)
__device__ __forceinline__ ResizeAxis resize_axis(uint32_t i, double scale, uint32_t src_n, double* frac) {
  const double ori = (double)(int)i * scale;
  int lo = (int)floor(ori);
  lo = lo < 0 ? 0 : (lo > (int)src_n - 1 ? (int)src_n - 1 : lo);
  const int hi = lo + 1 > (int)src_n - 1 ? (int)src_n - 1 : lo + 1;
  *frac = ori - (double)lo;
  return {(uint32_t)lo, (uint32_t)hi};
}

// bicubic_interpolate's weights (editorhelper.cpp:89-94)
__device__ __forceinline__ ResizeWeights resize_weights(double t) {
  const double u = 1 - t;
  ResizeWeights w;
  w.w0 = u * u * u;
  w.w1 = 3 * t * u * u;
  w.w2 = 3 * t * t * u;
  w.w3 = t * t * t;
  return w;
}

// the four normalised samples -> the stored byte
__device__ __forceinline__ uint32_t resize_byte(const ResizeWeights& w, float p0, float p1, float p2, float p3) {
  const double r = w.w0 * (double)p0 + w.w1 * (double)p1 + w.w2 * (double)p2 + w.w3 * (double)p3;
  float v = (float)r;
  v = v * 255.0f;
  v = v + 0.5f;
  v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
  return (uint32_t)(int)v;
}

}  // namespace uhdr
