// API-1 encode chain with its round trips removed (MI355X extension, round 4; not reference operators).
//
// JpegR::encodeJPEGR API-1 (/root/reference/lib/src/jpegr.cpp:253-316) runs generateGainMap, compresses the map, converts the
// base image's YUV encoding (convertYuv, jpegr.cpp:436-518) and compresses it.  As separate kernels that was seven launches:
// pass 1, min/max reduce, pass 2 (writes 3 B/px of map), rgb->ycc + FDCT of the map (reads them back), convertYuv (rewrites
// 1.5 B/px), three FDCT launches over the base planes (read them back; a 4K chroma plane is too small to fill the part).
// Two kernels here replace five of them:
//
//   map_blocks_kernel   pass 2 of generateGainMap (ratio -> byte through the per-channel step tables, generate_gainmap.hip)
//                       + libjpeg's rgb_ycc_convert + the three FDCT / quantize transforms in one pass: 12 B/px of gain ratios in,
//                       6 B/px of coefficients out (+ 3 B/px if the caller wants the 8-bit map itself)
//   base_blocks_kernel  convertYuv + FDCT / quantize of Y, Cb, Cr in ONE launch: a wave takes two 16 x 16 MCUs, converts their
//                       128 quads (transformYuv420's arithmetic, gainmapmath.cpp:686-748) into an LDS tile and transforms
//                       the 8 luma + 4 chroma blocks from there; the converted planes never exist in HBM
//   base_blocks_rgba_kernel  the same for a packed RGBA8888 intent, whose base image is 4:4:4: convert_raw_input_to_ycbcr + convertYuv +
//                       FDCT / quantize from registers (below; tests/test_gpu_api1_rgba.py)
//
// Coefficients are bit-identical to the unfused chain (tests/test_gpu_parity.py::test_api1_fused_chain_equals_the_operators).
#include <stdlib.h>
#include <string.h>
#include "lds_copy.h"

#include "cu_count.h"
#include "encode_core.h"
#include "fdct_core.h"

namespace uhdr {
using namespace fdct;
namespace {

constexpr int kBlock = 256;  // 4 waves

// The block side of a gain map, shared by map_blocks_kernel and map_blocks_onepass_kernel: an ACTIVE lane (row rr, block rb) holds the
// 8 * NCH map bytes of its row of its block in w, packed as they come; libjpeg's rgb_ycc_convert for three channels, level shift.  Then
// fdct_core.h's strip_transform.  (The optional 8-byte stores of the map itself stay in the kernels: inside a helper they cost
// map_blocks_kernel<3> 14 VGPRs and a workgroup per CU.)
template <int NCH>
__device__ __forceinline__ void map_row_samples(const uint32_t (&w)[2 * NCH], int (&comp)[3][8]) {
  auto byte_at = [&](int e) -> int { return (int)((w[e >> 2] >> (8 * (e & 3))) & 0xffu); };
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (NCH == 3) rgb_ycc_level_shift(byte_at(3 * k), byte_at(3 * k + 1), byte_at(3 * k + 2), comp, k);
    else comp[0][k] = byte_at(k) - 128;
  }
}

// ---- the gain map: ratio plane -> coefficients ------------------------------------------------------------------------------------
struct MapBlocksParams {
  const float* ratio;      // map_w * map_h * nch gain ratios (pass 1)
  const AffineDev* dev;    // final range + step tables (minmax_table_kernel)
  const double* math_tab;  // per-sample evaluation when a channel has no table
  uint8_t* map_out;        // optional: the 8-bit map, nch bytes per pixel
  uint32_t out_stride;     // pixels
  int bw, bh;              // blocks (map_w / 8, map_h / 8)
  int16_t* coef[3];
  QuantTables q;
  const float* gamma_thr;  // the two-pass byte thresholds of a gamma != 1 (gamma_code.h), global memory; null: gamma is 1
  uint32_t map_w, map_h;   // EDGE: the map's samples; bw, bh are ceil(map_w / 8), ceil(map_h / 8)
};

// EDGE kernels: how many of the eight samples of row y, columns x0 .. x0 + 7 lie inside the map
__device__ __forceinline__ uint32_t map_row_valid(uint32_t x0, uint32_t y, uint32_t map_w, uint32_t map_h) {
  return y < map_h ? min(8u, map_w - x0) : 0u;
}
// EDGE, one channel: the map goes to compressYCbCr in a zero-initialised allocation whose stride covers the block-aligned width
// (uhdr_memory_block_t, ultrahdr_api.cpp:46), so every sample outside map_w x map_h is byte 0
__device__ __forceinline__ void map_row_zero_outside(uint32_t (&w)[2], uint32_t nv) {
  const unsigned long long m = nv >= 8 ? ~0ull : ((1ull << (8 * nv)) - 1);
  w[0] &= (uint32_t)m;
  w[1] &= (uint32_t)(m >> 32);
}
// EDGE: the nv * NCH map bytes of a lane's row, one by one (any pitch, nothing beside them touched)
template <int NCH>
__device__ __forceinline__ void map_row_store_bytes(uint8_t* o, const uint32_t (&w)[2 * NCH], uint32_t nv) {
#pragma unroll
  for (int e = 0; e < 8 * NCH; e++)
    if ((uint32_t)(e / NCH) < nv) o[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
}

constexpr int kMapBlock = 512;  // eight waves share one copy of the step tables (24 KB): three workgroups = 24 waves per CU
// EDGE: maps that are not whole blocks.  A three-channel map (RGB888 through jpeg_write_scanlines) repeats its last column and row, as
// fdct_quant_rgb_kernel does -- the clamped sample's byte --, a one-channel map is zero outside; the ratio plane keeps pitch map_w, so a
// row is read float by float; the optional 8-bit map is stored byte by byte, map_w x map_h of them.
template <int NCH, bool EDGE = false>
__global__ __launch_bounds__(kMapBlock) void map_blocks_kernel(const MapBlocksParams p) {
  constexpr int kBlock = kMapBlock;  // (shadows the file's 256 inside this kernel)
  __shared__ int s_ws[kBlock / 64][kWsWords];
  __shared__ uint2 s_tab[NCH][kAffTabMax];
  __shared__ uint2 s_q[2][64];
  stage_quant_tables(s_q, p.q, threadIdx.x);
  StepTab st[3];
  bool tabs = true;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const AffineTabDev& td = p.dev->tab[c];
    st[c].tab = nullptr;
    st[c].n = td.n; st[c].base8 = td.base8; st[c].shm3 = td.shm3; st[c].lo_bits = td.lo_bits; st[c].hi_bits = td.hi_bits;
    tabs = tabs && td.ok != 0;
  }
  if (tabs) {
    const uint2* src = (const uint2*)((const char*)p.dev + kAffineTablesOff);
#pragma unroll
    for (int c = 0; c < NCH; c++)
      copy_to_lds(s_tab[c], src + (size_t)c * kAffTabMax, st[c].n * 2u, threadIdx.x, kBlock);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* ws = s_ws[wv];
  const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;
  const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);
  const int rr = lane >> 3, rb = lane & 7;
  const uint32_t map_w = EDGE ? p.map_w : (uint32_t)p.bw * 8;
  for (int t = gwave; t < total; t += nwaves) {
    const int by = t / groups_x, gx = t - by * groups_x;
    const int bx = gx * 8 + rb;
    const bool active = bx < p.bw;
    int comp[3][8];
    if (EDGE && active) {
      const uint32_t y = by * 8 + rr, x0 = bx * 8;
      const float* row = p.ratio + (size_t)min(y, p.map_h - 1) * map_w * NCH;
      auto ratio_at = [&](int e) -> float { return row[(size_t)min(x0 + (uint32_t)(e / NCH), map_w - 1) * NCH + e % NCH]; };
      uint32_t w[2 * NCH];
      if (tabs) {
#pragma unroll
        for (int k = 0; k < 2 * NCH; k++) {
          uint32_t acc = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) acc |= step_code(ratio_at(4 * k + i), s_tab[(4 * k + i) % NCH], st[(4 * k + i) % NCH]) << (8 * i);
          w[k] = acc;
        }
      } else {  // (the per-sample evaluation below, on the clamped samples)
#pragma unroll 1
        for (int k = 0; k < 2 * NCH; k++) {
          uint32_t acc = 0;
#pragma unroll 1
          for (int i = 0; i < 4; i++) {
            const int c = (4 * k + i) % NCH;
            const float lg = gain_log2_of_ratio(ratio_at(4 * k + i), p.math_tab);
            float m = div_by_rcp64(lg - p.dev->mn[c], p.dev->range_rcp[c]);
            if (p.gamma_thr) {
              acc |= gamma_code(m, p.gamma_thr) << (8 * i);
              continue;
            }
            m *= 255.0f;
            float t2 = m + 0.5f;
            t2 = (t2 < 0.0f) ? 0.0f : ((t2 > 255.0f) ? 255.0f : t2);
            acc |= (uint32_t)t2 << (8 * i);
          }
          ws[lane * 9 + k] = (int)acc;
        }
#pragma unroll
        for (int k = 0; k < 2 * NCH; k++) w[k] = (uint32_t)ws[lane * 9 + k];
      }
      const uint32_t nv = map_row_valid(x0, y, map_w, p.map_h);
      if constexpr (NCH == 1) map_row_zero_outside(w, nv);
      if (p.map_out && nv) map_row_store_bytes<NCH>(p.map_out + ((size_t)y * p.out_stride + x0) * NCH, w, nv);
      map_row_samples<NCH>(w, comp);
    } else if (active) {
      const uint32_t y = by * 8 + rr, x0 = bx * 8;
      const float4* src = (const float4*)(p.ratio + ((size_t)y * map_w + x0) * NCH);
      float4 g[2 * NCH];
#pragma unroll
      for (int k = 0; k < 2 * NCH; k++) g[k] = src[k];
      uint32_t w[2 * NCH];  // the 8 * NCH map bytes of this row, packed as they come
      if (tabs) {
#pragma unroll
        for (int k = 0; k < 2 * NCH; k++) {
          const float f[4] = {g[k].x, g[k].y, g[k].z, g[k].w};
          uint32_t acc = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) acc |= step_code(f[i], s_tab[(4 * k + i) % NCH], st[(4 * k + i) % NCH]) << (8 * i);
          w[k] = acc;
        }
      } else {  // a channel without a table (gamma is 1 here, or comes with its thresholds): the per-sample evaluation of generate_gainmap.hip,
                // as a rolled loop that parks its words in the wave's (idle) LDS workspace -- its float64 arithmetic must not
                // set the register count of the table path
        const float* gp = (const float*)src;
#pragma unroll 1
        for (int k = 0; k < 2 * NCH; k++) {
          uint32_t acc = 0;
#pragma unroll 1
          for (int i = 0; i < 4; i++) {
            const int c = (4 * k + i) % NCH;
            const float lg = gain_log2_of_ratio(gp[4 * k + i], p.math_tab);
            float m = div_by_rcp64(lg - p.dev->mn[c], p.dev->range_rcp[c]);
            if (p.gamma_thr) {  // (wave-uniform) the pow, the scaling and the clip as a search over the host's thresholds
              acc |= gamma_code(m, p.gamma_thr) << (8 * i);
              continue;
            }
            m *= 255.0f;
            float t2 = m + 0.5f;
            t2 = (t2 < 0.0f) ? 0.0f : ((t2 > 255.0f) ? 255.0f : t2);
            acc |= (uint32_t)t2 << (8 * i);
          }
          ws[lane * 9 + k] = (int)acc;
        }
#pragma unroll
        for (int k = 0; k < 2 * NCH; k++) w[k] = (uint32_t)ws[lane * 9 + k];
      }
      if (p.map_out) {
        uint8_t* o = p.map_out + ((size_t)y * p.out_stride + x0) * NCH;
#pragma unroll
        for (int k = 0; k < NCH; k++) *(uint2*)(o + 8 * k) = uint2{w[2 * k], w[2 * k + 1]};
      }
      map_row_samples<NCH>(w, comp);
    }
    strip_transform<NCH>(comp, active, p.coef, p.bw, by, bx, lane, ws, QuantLds{s_q[0]}, QuantLds{s_q[1]});
  }
}

// ---- the gain map in one pass: the two intents -> coefficients --------------------------------------------------------------------
// The one-pass (UHDR_USAGE_REALTIME) generateGainMap (jpegr.cpp:719-835) knows its gain range before it reads a pixel, so nothing has to
// wait between the pixel side and the block side: generate_kernel<.., TWO_PASS = false>'s pixel (generate_gainmap.hip) and
// map_blocks_kernel's strip in one kernel.  Lane (row rr, block rb) computes the eight map pixels of row rr of block rb -- sample_box
// over the s x s box of both intents, yuv -> rgb, the inverse-OETF tables, gamut matrix + clipNegatives, gain, byte through the gain8
// step table -- packs them into the words map_blocks_kernel builds and goes on with map_row_samples / strip_transform.  The 8-bit map reaches HBM only when
// the caller wants it (g.out != null).  A call without a gain8 table (host_tables.cpp declined the boost range) evaluates encode_gain's
// float64 form per sample, as a rolled loop that parks its bytes in the wave's idle workspace, as map_blocks_kernel does.
// FAST: 4:2:0 + P010 at scale 1 with rows the vector loads can take (map_onepass_fast_layout) -- a lane's row is one 8-byte luma load,
// two 4-byte chroma loads and two 16-byte P010 loads instead of forty scalar ones; fetch_pixel's normalisation, the same floats.
// LDS: sRGB 4 KB + HDR table 16 KB + unorm 5 KB + gain8 16 KB + 8 workspaces 18 KB + quantiser 1 KB = 60 KB: two workgroups per CU.
struct MapOnepassParams {
  GenParams g;             // g.out / g.out_stride: the optional 8-bit map
  int bw, bh;              // blocks (map_w / 8, map_h / 8)
  int16_t* coef[3];
  QuantTables q;
};
struct OnepassLds {
  float srgb[kSrgbN];
  float hdr[kInvOetfN];
  UnormTables unorm;
};

// one map pixel from the two box means: generate_kernel's sequence, with gain_of_pixel<false>'s bytes (encode_core.h) kept in registers
template <int NCH>
__device__ __forceinline__ void onepass_codes(Color3 s, Color3 h, const GenParams& p, const OnepassLds& L, const uint2* gain8, bool hdr_lut,
                                              bool hdr_lut_4096, uint32_t code[NCH]) {
  if (!p.sdr_is_rgb) s = yuv_to_rgb(s.r, s.g, s.b, p.sdr_yuv);
  Color3 sl = linearise_hdr(s, L.srgb, true, false);
  if (p.sdr_gamut_on) {
    sl = mat3_apply(sl, p.sdr_gamut);
    sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
  }
  if (!p.hdr_is_rgb) h = yuv_to_rgb(h.r, h.g, h.b, p.hdr_yuv);
  Color3 hl = linearise_hdr(h, L.hdr, hdr_lut, hdr_lut_4096);
  if (p.hdr_gamut_on) {
    hl = mat3_apply(hl, p.hdr_gamut);
    hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
  }
  if (NCH == 3) {
    code[0] = encode_gain(sl.r * 203.0f, hl.r * p.hdr_nits, p, p.math_tab, gain8);
    code[1] = encode_gain(sl.g * 203.0f, hl.g * p.hdr_nits, p, p.math_tab, gain8);
    code[2] = encode_gain(sl.b * 203.0f, hl.b * p.hdr_nits, p, p.math_tab, gain8);
  } else {
    float sy, hy;
    if (p.use_luminance) {
      sy = (p.lum[0] * sl.r + p.lum[1] * sl.g + p.lum[2] * sl.b) * 203.0f;
      hy = (p.lum[0] * hl.r + p.lum[1] * hl.g + p.lum[2] * hl.b) * p.hdr_nits;
    } else {
      sy = fmaxf(sl.r, fmaxf(sl.g, sl.b)) * 203.0f;
      hy = fmaxf(hl.r, fmaxf(hl.g, hl.b)) * p.hdr_nits;
    }
    code[0] = encode_gain(sy, hy, p, p.math_tab, gain8);
  }
}

// EDGE (never with FAST): maps that are not whole blocks, by map_blocks_kernel<.., EDGE>'s rules -- a lane computes the clamped map pixel.
template <int SDRF, int HDRF, int NCH, bool FAST, bool EDGE = false>
__global__ __launch_bounds__(kMapBlock, 4) void map_blocks_onepass_kernel(const MapOnepassParams p) {
  static_assert(!(FAST && EDGE), "the vector fetch reads whole blocks");
  constexpr int kBlock = kMapBlock;
  __shared__ int s_ws[kBlock / 64][kWsWords];
  __shared__ OnepassLds L;
  __shared__ alignas(16) uint2 s_gain8[kStepTabMax];
  __shared__ uint2 s_q[2][64];
  const uint32_t tid = threadIdx.x;
  stage_quant_tables(s_q, p.q, tid);
  const GenParams& g = p.g;
  stage_step_tab(s_gain8, g.gain8, tid, kBlock);
  copy_to_lds(L.srgb, g.srgb_lut, (uint32_t)kSrgbN, tid, kBlock);
  if (g.hdr_inv_lut) copy_to_lds(L.hdr, g.hdr_inv_lut, (uint32_t)g.hdr_inv_n, tid, kBlock);
  fill_unorm_tables(L.unorm, tid, kBlock);
  __syncthreads();
  const bool hdr_lut = g.hdr_inv_lut != nullptr, hdr_lut_4096 = g.hdr_inv_n == kInvOetfN;
  const bool tab = g.gain8.tab != nullptr;
  const int lane = tid & 63, wv = tid >> 6;
  int* ws = s_ws[wv];
  const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;
  const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);
  const int rr = lane >> 3, rb = lane & 7;
  for (int t = gwave; t < total; t += nwaves) {
    const int by = t / groups_x, gx = t - by * groups_x;
    const int bx = gx * 8 + rb;
    const bool active = bx < p.bw;
    int comp[3][8];
    if (active) {
      const uint32_t y = by * 8 + rr, x0 = bx * 8;
      const uint32_t ys = EDGE ? min(y, g.map_h - 1) : y, x_last = g.map_w - 1;  // (sample_box below: column min(x0 + k, x_last) for EDGE)
      uint32_t w[2 * NCH];  // the 8 * NCH map bytes of this row, packed as they come
#pragma unroll
      for (int i = 0; i < 2 * NCH; i++) w[i] = 0;
      if (FAST) {  // (the launcher comes here with a gain8 table only)
        const uint2 yl = *(const uint2*)((const uint8_t*)g.sdr.p[0] + (size_t)y * g.sdr.stride[0] + x0);
        const uint32_t ub = *(const uint32_t*)((const uint8_t*)g.sdr.p[1] + (size_t)(y >> 1) * g.sdr.stride[1] + (x0 >> 1));
        const uint32_t vb = *(const uint32_t*)((const uint8_t*)g.sdr.p[2] + (size_t)(y >> 1) * g.sdr.stride[2] + (x0 >> 1));
        const uint4 hyv = *(const uint4*)((const uint16_t*)g.hdr.p[0] + (size_t)y * g.hdr.stride[0] + x0);
        const uint4 hcv = *(const uint4*)((const uint16_t*)g.hdr.p[1] + (size_t)(y >> 1) * g.hdr.stride[1] + x0);
        const uint32_t yw[2] = {yl.x, yl.y}, hy2[4] = {hyv.x, hyv.y, hyv.z, hyv.w}, hc2[4] = {hcv.x, hcv.y, hcv.z, hcv.w};
        const bool full = g.hdr.range == UHDR_CR_FULL_RANGE;
#pragma unroll
        for (int k = 0; k < 8; k++) {  // fetch_pixel's normalisation of both formats (pixel_io.h)
          const int yy = (int)((yw[k >> 2] >> (8 * (k & 3))) & 0xff), uu = (int)((ub >> (8 * (k >> 1))) & 0xff), vv = (int)((vb >> (8 * (k >> 1))) & 0xff);
          const Color3 s = {(float)yy * (1 / 255.0f), (float)(uu - 128) * (1 / 255.0f), (float)(vv - 128) * (1 / 255.0f)};
          const int hy = (int)(((hy2[k >> 1] >> (16 * (k & 1))) & 0xffff) >> 6), hu = (int)((hc2[k >> 1] & 0xffff) >> 6), hv = (int)(hc2[k >> 1] >> 22);
          Color3 h;
          if (full) h = {L.unorm.u10[hy], L.unorm.u10[hu] - 0.5f, L.unorm.u10[hv] - 0.5f};
          else h = {(float)(hy - 64) * (1 / 876.0f), (float)(hu - 64) * (1 / 896.0f) - 0.5f, (float)(hv - 64) * (1 / 896.0f) - 0.5f};
          uint32_t code[NCH];
          onepass_codes<NCH>(s, h, g, L, s_gain8, hdr_lut, hdr_lut_4096, code);
#pragma unroll
          for (int c = 0; c < NCH; c++) w[(k * NCH + c) >> 2] |= code[c] << (8 * ((k * NCH + c) & 3));
        }
      } else if (HDRF >= 0 && tab) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const uint32_t xs = EDGE ? min(x0 + k, x_last) : x0 + k;
          const Color3 s = sample_box<SDRF>(g.sdr, g.scale, xs, ys, &L.unorm), h = sample_box<HDRF>(g.hdr, g.scale, xs, ys, &L.unorm);
          uint32_t code[NCH];
          onepass_codes<NCH>(s, h, g, L, s_gain8, hdr_lut, hdr_lut_4096, code);
#pragma unroll
          for (int c = 0; c < NCH; c++) w[(k * NCH + c) >> 2] |= code[c] << (8 * ((k * NCH + c) & 3));
        }
      } else {  // no gain8 table for this boost range: encode_gain's own per-sample evaluation, rolled, bytes parked in the idle workspace
                // (and the HDR formats without an instantiation of their own -- 30-bit 4:4:4, half float: eight copies of the format
                // switch are not worth their registers)
        uint8_t* park = (uint8_t*)(ws + lane * 9);
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
          const uint32_t xs = EDGE ? min(x0 + k, x_last) : x0 + k;
          const Color3 s = sample_box<SDRF>(g.sdr, g.scale, xs, ys, &L.unorm), h = sample_box<HDRF>(g.hdr, g.scale, xs, ys, &L.unorm);
          uint32_t code[NCH];
          onepass_codes<NCH>(s, h, g, L, tab ? s_gain8 : nullptr, hdr_lut, hdr_lut_4096, code);
#pragma unroll
          for (int c = 0; c < NCH; c++) park[k * NCH + c] = (uint8_t)code[c];
        }
#pragma unroll
        for (int i = 0; i < 2 * NCH; i++) w[i] = (uint32_t)ws[lane * 9 + i];
      }
      if constexpr (EDGE) {
        const uint32_t nv = map_row_valid(x0, y, g.map_w, g.map_h);
        if constexpr (NCH == 1) map_row_zero_outside(w, nv);
        if (g.out && nv) map_row_store_bytes<NCH>(g.out + ((size_t)y * g.out_stride + x0) * NCH, w, nv);
      } else if (g.out) {
        uint8_t* o = g.out + ((size_t)y * g.out_stride + x0) * NCH;
#pragma unroll
        for (int k = 0; k < NCH; k++) *(uint2*)(o + 8 * k) = uint2{w[2 * k], w[2 * k + 1]};
      }
      map_row_samples<NCH>(w, comp);
    }
    strip_transform<NCH>(comp, active, p.coef, p.bw, by, bx, lane, ws, QuantLds{s_q[0]}, QuantLds{s_q[1]});
  }
}

// ---- the base image: convertYuv + FDCT of Y, Cb, Cr in one launch -------------------------------------------------------------------
struct BaseBlocksParams {
  const uint8_t* y;
  const uint8_t* u;
  const uint8_t* v;
  uint32_t sy, su, sv;     // strides in bytes
  int mcus_x, mcus_y;      // 16 x 16 MCUs (w / 16, h / 16)
  int convert;             // 0: the planes go to the FDCT as they are
  Mat3 c;                  // convertYuv's coefficients (host_tables.cpp: yuv_encoding_matrix)
  int16_t* coef[3];
  QuantTables q;
  // EDGE: the frame's w x h samples (even), ALIGN(w, 8), and per plane compressYCbCr's column mode (FdctEdge, uhdr_types.h);
  // mcus_x, mcus_y are ceil(w / 16), ceil(h / 16)
  int w, h, aw_y;
  int cm[3];
};

__device__ __forceinline__ uint32_t st8(float v) { return (uint32_t)__builtin_amdgcn_fmed3f(v, 0.0f, 255.0f); }  // static_cast<uint8_t>(CLIP3(v, 0, 255)), convert.hip

// One quad (luma columns gx, gx + 1 of rows gy, gy + 1, the chroma sample under them) of an MCU that reaches beyond the frame, as
// JpegEncoderHelper::compressYCbCr (jpegencoderhelper.cpp:246-309) hands it to libjpeg after convertYuv ran in place on w x h only -- FdctEdge's
// rules, per plane.  Column mode 0 (the stride covers the block-aligned width): columns past the width are the caller's bytes, unconverted;
// rows past the height are 0 (Y) / 128 (Cb, Cr).  Column mode 1: columns past the width are 0 / 128, rows past the height still hold what the
// MCU row above copied into the helper's scratch rows -- the converted row 16 (chroma: 8) rows up, zeros in the first MCU row.
// Column mode 2 (API-0: planes the library allocated zero-filled, whose device copy is not): mode 0 with columns past the width 0 in every
// plane, and no load there.
// w and h are even: a quad lies inside or outside as a whole, in each direction.
__device__ __forceinline__ void base_edge_quad(const BaseBlocksParams& p, int gy, int gx, uint32_t& o0, uint32_t& o1, uint32_t& ou, uint32_t& ov) {
  const bool in_x = gx < p.w, in_y = gy < p.h;
  const int sgy = in_y ? gy : gy - 16;  // (a row of the MCU row above: all of its rows are inside)
  uint32_t c0 = 0, c1 = 0, cu = 0, cv = 0;  // the converted quad at (sgy, gx)
  if (in_x && sgy >= 0) {
    const uint32_t r0 = *(const uint16_t*)(p.y + (size_t)sgy * p.sy + gx), r1 = *(const uint16_t*)(p.y + (size_t)(sgy + 1) * p.sy + gx);
    const uint32_t ub = p.u[(size_t)(sgy >> 1) * p.su + (gx >> 1)], vb = p.v[(size_t)(sgy >> 1) * p.sv + (gx >> 1)];
    c0 = r0; c1 = r1; cu = ub; cv = vb;
    if (p.convert) {  // (base_blocks_kernel's arithmetic)
      const float u = (float)((int)ub - 128) * (1 / 255.0f), v = (float)((int)vb - 128) * (1 / 255.0f);
      const Color3 a = mat3_apply({(float)(r0 & 0xff) * (1 / 255.0f), u, v}, p.c);
      const Color3 b = mat3_apply({(float)(r0 >> 8) * (1 / 255.0f), u, v}, p.c);
      const Color3 c = mat3_apply({(float)(r1 & 0xff) * (1 / 255.0f), u, v}, p.c);
      const Color3 d = mat3_apply({(float)(r1 >> 8) * (1 / 255.0f), u, v}, p.c);
      const float nu = (((a.g + b.g) + c.g) + d.g) / 4.0f;
      const float nv = (((a.b + b.b) + c.b) + d.b) / 4.0f;
      c0 = st8(a.r * 255.0f + 0.5f) | (st8(b.r * 255.0f + 0.5f) << 8);
      c1 = st8(c.r * 255.0f + 0.5f) | (st8(d.r * 255.0f + 0.5f) << 8);
      cu = st8(nu * 255.0f + 128.0f + 0.5f);
      cv = st8(nv * 255.0f + 128.0f + 0.5f);
    }
  }
  o0 = o1 = 0;
  if (in_x) {
    if (in_y || p.cm[0] == 1) { o0 = c0; o1 = c1; }
  } else if (in_y && p.cm[0] == 0 && gx < p.aw_y) {  // (luma blocks past aw_y only complete an MCU: never written)
    o0 = *(const uint16_t*)(p.y + (size_t)gy * p.sy + gx);
    o1 = *(const uint16_t*)(p.y + (size_t)(gy + 1) * p.sy + gx);
  }
  auto chroma = [&](const uint8_t* plane, uint32_t stride, int cm, uint32_t conv) -> uint32_t {
    if (in_x) return (in_y || cm == 1) ? conv : 128u;
    if (in_y && cm == 2) return 0u;
    return (in_y && cm == 0) ? (uint32_t)plane[(size_t)(gy >> 1) * stride + (gx >> 1)] : 128u;
  };
  ou = chroma(p.u, p.su, p.cm[1], cu);
  ov = chroma(p.v, p.sv, p.cm[2], cv);
}

// EDGE: frames that are not whole MCUs -- ceil(w / 16) x ceil(h / 16) MCUs, the luma blocks of libjpeg's width_in_blocks grid
// (ceil(w / 8) x ceil(h / 8): a luma block that only completes an MCU is the entropy coder's to make up).  A pair that reaches beyond the
// frame (wave-uniform) builds its quads with base_edge_quad; every other pair takes the loads of the whole-MCU kernel.
template <bool EDGE>
__global__ __launch_bounds__(kBlock) void base_blocks_kernel(const BaseBlocksParams p) {
  __shared__ int s_ws[kBlock / 64][kWsWords];
  // per wave: the converted samples of two MCUs -- luma 16 rows x 32, Cb and Cr 8 rows x 16 each
  __shared__ __attribute__((aligned(16))) uint8_t s_y[kBlock / 64][16 * 32];
  __shared__ __attribute__((aligned(16))) uint8_t s_c[kBlock / 64][2][8 * 16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* ws = s_ws[wv];
  uint8_t* ty = s_y[wv];
  uint8_t* tcb = s_c[wv][0];
  uint8_t* tcr = s_c[wv][1];
  const int pairs_x = (p.mcus_x + 1) >> 1, total = pairs_x * p.mcus_y;
  const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);
  const int rr = lane >> 3, rb = lane & 7;
  __shared__ uint2 s_q[2][64];
  stage_quant_tables(s_q, p.q, threadIdx.x);
  __syncthreads();
  const int bw_y = EDGE ? (p.w + 7) >> 3 : p.mcus_x * 2, bw_c = p.mcus_x;
  const int bh_y = (p.h + 7) >> 3;  // (EDGE)
  for (int t = gwave; t < total; t += nwaves) {
    const int my = t / pairs_x, mp = t - my * pairs_x;
    const int mx0 = mp * 2;
    const int n_mcu = (mx0 + 1 < p.mcus_x) ? 2 : 1;
    const bool edge_pair = EDGE && (my * 16 + 16 > p.h || (mx0 + n_mcu) * 16 > p.w);  // (wave-uniform)
    // ---- phase A: the pair's 128 quads (8 quad rows x 16 quad columns), two per lane, through convertYuv into the tile ----
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int q = lane + 64 * h, qr = q >> 4, qc = q & 15;  // quad row / column inside the pair
      if (qc < n_mcu * 8) {
        const size_t gy = (size_t)my * 16 + qr * 2, gx = (size_t)mx0 * 16 + qc * 2;
        if (edge_pair) {
          uint32_t e0, e1, eu, ev;
          base_edge_quad(p, (int)gy, (int)gx, e0, e1, eu, ev);
          *(uint16_t*)(ty + (qr * 2) * 32 + qc * 2) = (uint16_t)e0;
          *(uint16_t*)(ty + (qr * 2 + 1) * 32 + qc * 2) = (uint16_t)e1;
          tcb[qr * 16 + qc] = (uint8_t)eu;
          tcr[qr * 16 + qc] = (uint8_t)ev;
          continue;
        }
        const uint32_t r0 = *(const uint16_t*)(p.y + gy * p.sy + gx), r1 = *(const uint16_t*)(p.y + (gy + 1) * p.sy + gx);
        const uint32_t ub = p.u[(gy >> 1) * p.su + (gx >> 1)], vb = p.v[(gy >> 1) * p.sv + (gx >> 1)];
        uint32_t o0 = r0, o1 = r1, ou = ub, ov = vb;
        if (p.convert) {  // transformYuv420 (gainmapmath.cpp:686-748), the arithmetic of convert.hip: transform_yuv420_kernel
          const float u = (float)((int)ub - 128) * (1 / 255.0f), v = (float)((int)vb - 128) * (1 / 255.0f);
          const Color3 a = mat3_apply({(float)(r0 & 0xff) * (1 / 255.0f), u, v}, p.c);
          const Color3 b = mat3_apply({(float)(r0 >> 8) * (1 / 255.0f), u, v}, p.c);
          const Color3 c = mat3_apply({(float)(r1 & 0xff) * (1 / 255.0f), u, v}, p.c);
          const Color3 d = mat3_apply({(float)(r1 >> 8) * (1 / 255.0f), u, v}, p.c);
          const float nu = (((a.g + b.g) + c.g) + d.g) / 4.0f;
          const float nv = (((a.b + b.b) + c.b) + d.b) / 4.0f;
          o0 = st8(a.r * 255.0f + 0.5f) | (st8(b.r * 255.0f + 0.5f) << 8);
          o1 = st8(c.r * 255.0f + 0.5f) | (st8(d.r * 255.0f + 0.5f) << 8);
          ou = st8(nu * 255.0f + 128.0f + 0.5f);
          ov = st8(nv * 255.0f + 128.0f + 0.5f);
        }
        *(uint16_t*)(ty + (qr * 2) * 32 + qc * 2) = (uint16_t)o0;
        *(uint16_t*)(ty + (qr * 2 + 1) * 32 + qc * 2) = (uint16_t)o1;
        tcb[qr * 16 + qc] = (uint8_t)ou;
        tcr[qr * 16 + qc] = (uint8_t)ov;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    // ---- phase B: the 8 luma blocks.  Block rb = (MCU m, block row byy, block column bxx) ------------------------------------
    {
      const int m = rb >> 2, byy = (rb >> 1) & 1, bxx = rb & 1;
      const bool active = m < n_mcu && (!EDGE || ((mx0 + m) * 2 + bxx < bw_y && my * 2 + byy < bh_y));
      int in[8], out[8], v[8];
      if (active) {
        const uint8_t* src = ty + (byy * 8 + rr) * 32 + m * 16 + bxx * 8;
        unpack8_level_shift(((const uint32_t*)src)[0], ((const uint32_t*)src)[1], in);
        fdct_1d<0>(in, out);
      } else {
#pragma unroll
        for (int c = 0; c < 8; c++) out[c] = 0;
      }
      column_pass_and_quantize(ws, lane, out, QuantLds{s_q[0]}, v);
      if (active) {
        const size_t bx = (size_t)(mx0 + m) * 2 + bxx, by = (size_t)my * 2 + byy;
        store_coef_row(p.coef[0] + (by * bw_y + bx) * 64 + rr * 8, v);
      }
    }
    // ---- phase C: the 4 chroma blocks (Cb of MCU 0, 1, Cr of MCU 0, 1): lanes with rb < 4 ------------------------------------
    {
      const int comp = (rb >> 1) & 1, m = rb & 1;
      const bool active = rb < 4 && m < n_mcu;
      int in[8], out[8], v[8];
      if (active) {
        const uint8_t* src = (comp ? tcr : tcb) + rr * 16 + m * 8;
        unpack8_level_shift(((const uint32_t*)src)[0], ((const uint32_t*)src)[1], in);
        fdct_1d<0>(in, out);
      } else {
#pragma unroll
        for (int c = 0; c < 8; c++) out[c] = 0;
      }
      column_pass_and_quantize(ws, lane, out, QuantLds{s_q[1]}, v);
      if (active) store_coef_row(p.coef[1 + comp] + ((size_t)my * bw_c + (mx0 + m)) * 64 + rr * 8, v);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- the base image from a packed RGBA8888 intent: convert_raw_input_to_ycbcr + convertYuv + FDCT of Y, Cb, Cr in one launch ----------
// API-1 with an RGBA8888 SDR intent (jpegr.cpp:247-291) compresses a YCbCr 4:4:4 rendition of it: convert_raw_input_to_ycbcr
// (gainmapmath.cpp:1447-1474) writes full-range bytes in the intent's own gamut, convertYuv (transformYuv444) rewrites them in the base
// encoding -- a second rounding to bytes -- and the three planes go to the FDCT.  Staged, that is three launches and 22 B/px; here a wave
// owns a strip of eight horizontally adjacent 8 x 8 blocks, lane (row rr, block rb) loads the eight pixels of row rr of block rb, converts
// them in registers with the staged kernels' arithmetic (convert.hip: rgb_to_ycbcr444_wide_kernel<false>, transform_yuv444_kernel; both
// roundings kept) and is the lane that runs the row pass of that block row: the samples never touch LDS or HBM, only the transposes of
// column_pass_and_quantize use the wave's workspace, three times per strip.  4 B/px in, 6 B/px out.
// Rows whose base address and pitch are multiples of 16 bytes are read with two 16-byte loads per lane (VEC); any other pitch takes the
// same kernel with eight dword loads (pixels are 32-bit words: the base address is a multiple of 4, the launcher's caller checks).
// EDGE: frames that are not whole blocks, on the ceil(w / 8) x ceil(h / 8) grid.  The reference converts an RGBA intent into an image it
// allocated itself -- zero-filled, stride ALIGN(w, 64) (gainmapmath.cpp:1447-1449, ultrahdr_api.cpp:50-95) --, convertYuv rewrites w x h of it,
// and compressYCbCr (jpegencoderhelper.cpp:246-309) sees a stride that covers the block-aligned width: columns past the width are the
// allocation's zeros in all three planes (never converted), rows past the height are the helper's zero Y row and its memset(128) chroma row
// over the whole aligned width.  A strip that touches the right or bottom edge (wave-uniform) loads pixel by pixel, predicated per lane --
// nothing past w pixels of a row or past row h - 1 is read --, every other strip takes the loads of the whole-block kernel.
struct BaseBlocksRgbaParams {
  const uint32_t* src;     // packed RGBA8888
  uint32_t stride;         // pixels
  int bw, bh;              // blocks (w / 8, h / 8)
  int convert;             // 0: convert_raw_input_to_ycbcr's bytes go to the FDCT as they are
  Rgb2Yuv k;               // the intent's gamut (host_tables.cpp: rgb2yuv_coeffs)
  Mat3 c;                  // convertYuv's coefficients (host_tables.cpp: yuv_encoding_matrix)
  int16_t* coef[3];
  QuantTables q;
  uint32_t w, h;           // EDGE: the frame's pixels; bw, bh are ceil(w / 8), ceil(h / 8)
};

__device__ __forceinline__ float clipf255(float v) { return (v < 0.0f) ? 0.0f : ((v > 255.0f) ? 255.0f : v); }  // convert.hip: clipf

template <bool VEC, bool EDGE = false>
__global__ __launch_bounds__(kBlock) void base_blocks_rgba_kernel(const BaseBlocksRgbaParams p) {
  __shared__ int s_ws[kBlock / 64][kWsWords];
  __shared__ uint2 s_q[2][64];
  __shared__ float s_u8[256];  // i / 255.0f, the device's correctly rounded division (pixel_io.h: UnormTables)
  stage_quant_tables(s_q, p.q, threadIdx.x);
  for (uint32_t i = threadIdx.x; i < 256; i += kBlock) s_u8[i] = (float)i / 255.0f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* ws = s_ws[wv];
  const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;
  const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);
  const int rr = lane >> 3, rb = lane & 7;
  const Rgb2Yuv k = p.k;
  const float k255 = 1 / 255.0f;
  for (int t = gwave; t < total; t += nwaves) {
    const int by = t / groups_x, gx = t - by * groups_x;
    const int bx = gx * 8 + rb;
    const bool active = bx < p.bw;
    int comp[3][8];
    if (active) {
      const uint32_t* s0 = p.src + ((size_t)(by * 8 + rr) * p.stride + (size_t)bx * 8);
      uint32_t px[8];
      bool edge_strip = false;  // (wave-uniform)
      uint32_t nv = 8;          // EDGE: the pixels of this lane's row that lie inside the frame
      bool row_in = true;
      if constexpr (EDGE) {
        edge_strip = (uint32_t)by * 8 + 8 > p.h || (uint32_t)gx * 64 + 64 > p.w;
        row_in = (uint32_t)(by * 8 + rr) < p.h;
        nv = row_in ? min(8u, p.w - (uint32_t)bx * 8) : 0u;
      }
      if (EDGE && edge_strip) {
#pragma unroll
        for (int j = 0; j < 8; j++) px[j] = (uint32_t)j < nv ? s0[j] : 0u;
      } else if (VEC) {
        const uint4 a = *(const uint4*)s0, b = *(const uint4*)(s0 + 4);
        px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w; px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) px[j] = s0[j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const Color3 e = {s_u8[px[j] & 0xff], s_u8[(px[j] >> 8) & 0xff], s_u8[(px[j] >> 16) & 0xff]};
        const Color3 q = rgb_to_yuv(e, k);
        int yy = (int)(uint32_t)clipf255(q.r * 255.0f + 0.5f);
        int uu = (int)(uint32_t)clipf255(q.g * 255.0f + 0.5f + 128.0f);
        int vv = (int)(uint32_t)clipf255(q.b * 255.0f + 0.5f + 128.0f);
        if (p.convert) {  // transformYuv444 on those bytes
          const Color3 o = mat3_apply({(float)yy * k255, (float)(uu - 128) * k255, (float)(vv - 128) * k255}, p.c);
          yy = (int)st8(o.r * 255.0f + 0.5f);
          uu = (int)st8(o.g * 255.0f + 128.0f + 0.5f);
          vv = (int)st8(o.b * 255.0f + 128.0f + 0.5f);
        }
        comp[0][j] = yy - 128;
        comp[1][j] = uu - 128;
        comp[2][j] = vv - 128;
      }
      if (EDGE && edge_strip) {
        const int c_out = row_in ? -128 : 0;  // byte 0 of the zero-filled allocation / byte 128 of the helper's chroma row
#pragma unroll
        for (int j = 0; j < 8; j++)
          if ((uint32_t)j >= nv) {
            comp[0][j] = -128;
            comp[1][j] = c_out;
            comp[2][j] = c_out;
          }
      }
    }
    // fdct_core.h's strip_transform, spelled out: behind the helper call the compiler packs the conversion above into v_pk_* pairs
    // with 36 more register moves, and the 4K launch went from 34.1 to 36.4 us
#pragma unroll
    for (int ci = 0; ci < 3; ci++) {
      int out[8], v[8];
      if (active) {
        fdct_1d<0>(comp[ci], out);
      } else {
#pragma unroll
        for (int c = 0; c < 8; c++) out[c] = 0;
      }
      column_pass_and_quantize(ws, lane, out, QuantLds{s_q[ci == 0 ? 0 : 1]}, v);
      if (active) store_coef_row(p.coef[ci] + ((size_t)by * p.bw + bx) * 64 + rr * 8, v);
    }
  }
}

int resident_grid(int total_wave_items, int per_cu) {
  const int cus = device_cu_count();
  int grid = (total_wave_items + kBlock / 64 - 1) / (kBlock / 64);
  if (grid > cus * per_cu) grid = cus * per_cu;
  return grid < 1 ? 1 : grid;
}

}  // namespace

// ratio plane (pass 1) + AffineDev (launch_minmax_table) -> quantized coefficients of the map's JPEG (+ the 8-bit map when map_out != null).
// nch 3: packed RGB semantics (rgb_ycc_convert, 4:4:4, luma table for Y, chroma table for Cb / Cr); nch 1: a Y400 map.
hipError_t launch_map_blocks(const float* ratio, const AffineDev* dev, const double* math_tab, int nch, int bw, int bh, const uint16_t* qt_luma,
                             const uint16_t* qt_chroma, int16_t* const coef[3], uint8_t* map_out, uint32_t out_stride, hipStream_t s,
                             const float* gamma_thr, uint32_t edge_w, uint32_t edge_h) {
  // edge_w x edge_h != 0: the map's samples, bw x bh = ceil(edge_w / 8) x ceil(edge_h / 8) -- the EDGE kernel (any size, any map_out pitch)
  MapBlocksParams p;
  memset(&p, 0, sizeof p);
  p.gamma_thr = gamma_thr;
  p.map_w = edge_w; p.map_h = edge_h;
  p.ratio = ratio; p.dev = dev; p.math_tab = math_tab; p.map_out = map_out; p.out_stride = out_stride; p.bw = bw; p.bh = bh;
  for (int i = 0; i < nch; i++) p.coef[i] = coef[i];
  fill_quant_table(qt_luma, &p.q.luma);
  fill_quant_table(qt_chroma, &p.q.chroma);
  int grid = (((bw + 7) / 8) * bh + kMapBlock / 64 - 1) / (kMapBlock / 64);
  const int cap = resident_grid(1 << 30, 3);  // 44 KB of LDS (tables + workspaces) per 512 threads: three workgroups per CU
  if (grid > cap) grid = cap;
  if (edge_w && edge_h) {
    if (nch == 3) hipLaunchKernelGGL((map_blocks_kernel<3, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
    else hipLaunchKernelGGL((map_blocks_kernel<1, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
  } else if (nch == 3) hipLaunchKernelGGL((map_blocks_kernel<3>), dim3(grid), dim3(kMapBlock), 0, s, p);
  else hipLaunchKernelGGL((map_blocks_kernel<1>), dim3(grid), dim3(kMapBlock), 0, s, p);
  return hipGetLastError();
}

// do the vector loads of map_blocks_onepass_kernel<.., FAST> stay aligned?  4:2:0 + P010 at scale 1: 8 luma bytes, 4 + 4 chroma bytes,
// 16 + 16 bytes of P010 per lane and row
static bool map_onepass_fast_layout(const GenParams& g) {
  if (g.scale != 1 || g.sdr.fmt != UHDR_IMG_FMT_12bppYCbCr420 || g.hdr.fmt != UHDR_IMG_FMT_24bppYCbCrP010 || g.sdr.h % 2) return false;
  if (((uintptr_t)g.sdr.p[0] | g.sdr.stride[0]) & 7) return false;
  if (((uintptr_t)g.sdr.p[1] | (uintptr_t)g.sdr.p[2] | g.sdr.stride[1] | g.sdr.stride[2]) & 3) return false;
  if (((uintptr_t)g.hdr.p[0] | (uintptr_t)g.hdr.p[1]) & 15) return false;
  return g.hdr.stride[0] % 8 == 0 && g.hdr.stride[1] % 8 == 0;  // (strides in 16-bit samples)
}
template <int SDRF, int HDRF>
static void launch_onepass_n(const MapOnepassParams& p, int nch, int grid, hipStream_t s, bool edges) {
  if (edges) {
    if (nch == 3) hipLaunchKernelGGL((map_blocks_onepass_kernel<SDRF, HDRF, 3, false, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
    else hipLaunchKernelGGL((map_blocks_onepass_kernel<SDRF, HDRF, 1, false, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
  } else if (nch == 3) hipLaunchKernelGGL((map_blocks_onepass_kernel<SDRF, HDRF, 3, false>), dim3(grid), dim3(kMapBlock), 0, s, p);
  else hipLaunchKernelGGL((map_blocks_onepass_kernel<SDRF, HDRF, 1, false>), dim3(grid), dim3(kMapBlock), 0, s, p);
}

// The one-pass gain map of the two intents in g (fill_gen_params + the one-pass range + gain8; g.out: the optional 8-bit map, g.out_stride
// pixels) -> quantized coefficients of the map's JPEG.  map_w, map_h multiples of 8, gamma 1; SDR 4:2:0 or RGBA8888, every HDR format
// fill_gen_params takes; nch as in launch_map_blocks.  edges: any map size and any map_out pitch (the EDGE kernel).
hipError_t launch_map_blocks_onepass(const GenParams& g, int nch, const uint16_t* qt_luma, const uint16_t* qt_chroma, int16_t* const coef[3],
                                     uint8_t* map_out, uint32_t out_stride, hipStream_t s, bool edges) {
  MapOnepassParams p;
  memset(&p, 0, sizeof p);
  p.g = g;
  p.g.out = map_out; p.g.out_stride = out_stride;
  p.bw = (int)(g.map_w / 8); p.bh = (int)(g.map_h / 8);
  if (edges) { p.bw = (int)((g.map_w + 7) / 8); p.bh = (int)((g.map_h + 7) / 8); }
  for (int i = 0; i < nch; i++) p.coef[i] = coef[i];
  fill_quant_table(qt_luma, &p.q.luma);
  fill_quant_table(qt_chroma, &p.q.chroma);
  int grid = (((p.bw + 7) / 8) * p.bh + kMapBlock / 64 - 1) / (kMapBlock / 64);
  const int cap = resident_grid(1 << 30, 2);  // 60 KB of LDS (tables + workspaces) per 512 threads: two workgroups per CU
  if (grid > cap) grid = cap;
  constexpr int k420 = UHDR_IMG_FMT_12bppYCbCr420, kRgba = UHDR_IMG_FMT_32bppRGBA8888, kP010 = UHDR_IMG_FMT_24bppYCbCrP010, k1010102 = UHDR_IMG_FMT_32bppRGBA1010102;
  // UHDR_HIP_ONEPASS_NO_VECTOR_FETCH=1: the per-sample fetch on every layout (tools/api1_onepass_time.py times the two against each other)
  if (!edges && g.gain8.tab && map_onepass_fast_layout(g) && !getenv("UHDR_HIP_ONEPASS_NO_VECTOR_FETCH")) {
    if (nch == 3) hipLaunchKernelGGL((map_blocks_onepass_kernel<k420, kP010, 3, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
    else hipLaunchKernelGGL((map_blocks_onepass_kernel<k420, kP010, 1, true>), dim3(grid), dim3(kMapBlock), 0, s, p);
  } else if (g.sdr.fmt == k420) {
    if (g.hdr.fmt == kP010) launch_onepass_n<k420, kP010>(p, nch, grid, s, edges);
    else launch_onepass_n<k420, -1>(p, nch, grid, s, edges);
  } else if (g.sdr.fmt == kRgba) {
    if (g.hdr.fmt == k1010102) launch_onepass_n<kRgba, k1010102>(p, nch, grid, s, edges);
    else launch_onepass_n<kRgba, -1>(p, nch, grid, s, edges);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// 4:2:0 planes (w, h multiples of 16) -> [convertYuv with matrix c ->] quantized coefficients of Y, Cb, Cr
// edges: any even w, h -- ceil(w / 16) x ceil(h / 16) MCUs, luma on its ceil(w / 8) x ceil(h / 8) grid, the samples beyond the frame by
// compressYCbCr's rules (base_edge_quad); a whole-MCU frame takes the kernel it takes without the flag.  col_mode >= 0: every plane's
// column mode is that one, whatever the strides (2: the API-0 chain's scratch planes)
hipError_t launch_base_blocks(const ImageView& yuv420, const Mat3* c, const uint16_t* qt_luma, const uint16_t* qt_chroma, int16_t* const coef[3],
                              hipStream_t s, bool edges, int col_mode) {
  BaseBlocksParams p;
  memset(&p, 0, sizeof p);
  p.y = (const uint8_t*)yuv420.p[0]; p.u = (const uint8_t*)yuv420.p[1]; p.v = (const uint8_t*)yuv420.p[2];
  p.sy = yuv420.stride[0]; p.su = yuv420.stride[1]; p.sv = yuv420.stride[2];
  p.mcus_x = (int)(yuv420.w / 16); p.mcus_y = (int)(yuv420.h / 16);
  p.convert = c ? 1 : 0;
  if (c) p.c = *c;
  for (int i = 0; i < 3; i++) p.coef[i] = coef[i];
  fill_quant_table(qt_luma, &p.q.luma);
  fill_quant_table(qt_chroma, &p.q.chroma);
  if (edges && (yuv420.w % 16 || yuv420.h % 16)) {
    p.mcus_x = (int)((yuv420.w + 15) / 16); p.mcus_y = (int)((yuv420.h + 15) / 16);
    p.w = (int)yuv420.w; p.h = (int)yuv420.h; p.aw_y = (p.w + 7) & ~7;
    p.cm[0] = p.sy >= (uint32_t)p.aw_y ? 0 : 1;  // jpegencoderhelper.cpp:256: strides[i] < alignedPlaneWidth[i] copies rows into a scratch MCU row
    p.cm[1] = p.su >= (uint32_t)p.mcus_x * 8 ? 0 : 1;
    p.cm[2] = p.sv >= (uint32_t)p.mcus_x * 8 ? 0 : 1;
    if (col_mode >= 0) p.cm[0] = p.cm[1] = p.cm[2] = col_mode;
    const int grid = resident_grid(((p.mcus_x + 1) / 2) * p.mcus_y, 8);
    hipLaunchKernelGGL(base_blocks_kernel<true>, dim3(grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  const int grid = resident_grid(((p.mcus_x + 1) / 2) * p.mcus_y, 8);
  hipLaunchKernelGGL(base_blocks_kernel<false>, dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

// packed RGBA8888 (w, h multiples of 8; stride in pixels; base address a multiple of 4) -> convert_raw_input_to_ycbcr with the coefficients k
// of the image's gamut -> [convertYuv with matrix c ->] quantized coefficients of Y, Cb, Cr, each on a (w / 8) x (h / 8) grid
// edges: any w, h >= 1 and any stride >= w -- the ceil(w / 8) x ceil(h / 8) grid, the samples beyond the frame by the rules at
// BaseBlocksRgbaParams; a whole-block frame takes the kernel it takes without the flag
hipError_t launch_base_blocks_rgba(const ImageView& rgba, const Rgb2Yuv& k, const Mat3* c, const uint16_t* qt_luma, const uint16_t* qt_chroma,
                                   int16_t* const coef[3], hipStream_t s, bool edges) {
  BaseBlocksRgbaParams p;
  memset(&p, 0, sizeof p);
  p.src = (const uint32_t*)rgba.p[0];
  p.stride = rgba.stride[0];
  p.bw = (int)(rgba.w / 8); p.bh = (int)(rgba.h / 8);
  p.k = k;
  p.convert = c ? 1 : 0;
  if (c) p.c = *c;
  for (int i = 0; i < 3; i++) p.coef[i] = coef[i];
  fill_quant_table(qt_luma, &p.q.luma);
  fill_quant_table(qt_chroma, &p.q.chroma);
  const int grid = resident_grid(((p.bw + 7) / 8) * p.bh, 7);  // 66 VGPRs: seven waves per SIMD, i.e. seven 4-wave workgroups per CU are resident
  const bool vec = ((uintptr_t)rgba.p[0] % 16) == 0 && rgba.stride[0] % 4 == 0;
  if (edges && (rgba.w % 8 || rgba.h % 8)) {
    p.bw = (int)((rgba.w + 7) / 8); p.bh = (int)((rgba.h + 7) / 8);
    p.w = rgba.w; p.h = rgba.h;
    const int edge_grid = resident_grid(((p.bw + 7) / 8) * p.bh, 7);  // (the EDGE instantiations: 70 VGPRs, seven waves per SIMD as well)
    if (vec) hipLaunchKernelGGL((base_blocks_rgba_kernel<true, true>), dim3(edge_grid), dim3(kBlock), 0, s, p);
    else hipLaunchKernelGGL((base_blocks_rgba_kernel<false, true>), dim3(edge_grid), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  }
  if (vec) hipLaunchKernelGGL((base_blocks_rgba_kernel<true>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((base_blocks_rgba_kernel<false>), dim3(grid), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

}  // namespace uhdr
