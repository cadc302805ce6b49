// API-0 encode front end in ONE pass over the HDR image (MI355X extension, not a reference operator).
//
// JpegR::encodeJPEGR API-0 (/root/reference/lib/src/jpegr.cpp:202-251) runs three full-image loops
// back to back: toneMap (HDR -> 8-bit SDR RGBA8888), generateGainMap (reads both images again) and
// convert_raw_input_to_ycbcr (reads the SDR image a third time to make the base JPEG's planes).
// Unfused that is 4+4, 4+4+3 and 4+3 bytes per pixel of HBM traffic and every HDR pixel is unpacked
// and linearised twice.  Here one thread carries a pixel through all three stages in registers:
// 4 bytes in (RGBA1010102; 8 for RGBA-F16), 3 (base YCbCr 4:4:4) + 3 (map, or 12 of float gains in
// two-pass mode) out, + 4 if the caller also wants the RGBA8888 SDR rendition.
//
// The arithmetic is the same sequence of IEEE operations as the three kernels (encode_core.h), and
// the 8-bit quantisation between the stages is kept: the gain map is computed from the QUANTISED SDR
// bytes exactly as generateGainMap would read them back.  tests/test_gpu_parity.py checks the fused
// outputs against tone_map -> generate_gainmap -> convert_raw_input_to_ycbcr, bit for bit.
// Conditions: RGB HDR input (RGBA1010102 / RGBA-F16), gain map at full resolution (scale 1).
#include "cu_count.h"
#include "encode_core.h"
#include "lds_copy.h"

namespace uhdr {
int fused_grid(uint32_t tiles, int per_cu);
namespace {

constexpr int kBlock = 512;  // 8 waves share one table set in LDS -> 3 workgroups = 24 waves per CU

template <int HDRF>
struct FusedLds {
  float srgb_of_byte[256];  // byte -> byte / 255.0f -> sRGB inverse-OETF table value (host_tables.cpp)
  // RGBA1010102 input: 10-bit code -> linear value (the host always provides it); RGBA-F16: the inverse-OETF table, if any
  float hdr[HDRF == UHDR_IMG_FMT_32bppRGBA1010102 ? 1024 : kInvOetfN];
  UnormTables unorm;
  uint2 srgb8[kStepTabMax];  // tone map: clamped linear value -> sRGB byte
  uint2 gain8[kStepTabMax];  // one pass: clamped gain -> map byte
};

__device__ __forceinline__ float clipf(float v, float hi) { return (v < 0.0f) ? 0.0f : ((v > hi) ? hi : v); }

template <int HDRF, bool TWO_PASS>
__global__ __launch_bounds__(kBlock) void encode_api0_fused_kernel(const FusedParams p, float* partials) {
  __shared__ FusedLds<HDRF> L;
  const uint32_t tid = threadIdx.x;
  copy_to_lds(L.srgb_of_byte, p.gen.srgb_of_byte, 256u, tid, kBlock);
  constexpr bool code_lin = HDRF == UHDR_IMG_FMT_32bppRGBA1010102;  // launch_encode_api0_fused checks that lin10 is there
  if constexpr (code_lin) {
    copy_to_lds(L.hdr, p.tm.lin10, 1024u, tid, kBlock);
  } else {
    if (p.tm.hdr_inv_lut) copy_to_lds(L.hdr, p.tm.hdr_inv_lut, (uint32_t)p.tm.hdr_inv_n, tid, kBlock);
  }
  stage_step_tab(L.srgb8, p.tm.srgb8, tid, kBlock);
  stage_step_tab(L.gain8, p.gen.gain8, tid, kBlock);
  fill_unorm_tables(L.unorm, tid, kBlock);
  __syncthreads();

  const uint32_t w = p.tm.hdr.w, h = p.tm.hdr.h;
  const uint32_t tiles_x = (w + kBlock - 1) / kBlock, tiles = tiles_x * h;
  const bool hdr_lut = p.tm.hdr_inv_lut != nullptr, hdr_lut_4096 = p.tm.hdr_inv_n == kInvOetfN;
  float mn[3] = {UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT}, mx[3] = {UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT};
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t y = t / tiles_x, x = (t - y * tiles_x) * kBlock + tid;
    if (x >= w) continue;
    // ---- toneMap (jpegr.cpp:2147-2203) -------------------------------------------------------------------------
    Color3 l;
    if constexpr (code_lin) {  // unpack + inverse OETF (+ OOTF) of a 10-bit code is one table entry
      const uint32_t v = ((const uint32_t*)p.tm.hdr.p[0])[x + (size_t)y * p.tm.hdr.stride[0]];
      l = Color3{L.hdr[v & 0x3ffu], L.hdr[(v >> 10) & 0x3ffu], L.hdr[(v >> 20) & 0x3ffu]};
    } else {
      const Color3 g = fetch_pixel<HDRF>(p.tm.hdr, x, y, &L.unorm);
      l = linearise_hdr(g, L.hdr, hdr_lut, hdr_lut_4096);
    }
    uint32_t r8, g8, b8;  // putRgba8888Pixel's bytes
    tone_curve_bytes(l, p.tm, p.tm.math_tab + kPowDirOff, L.srgb8, r8, g8, b8);  // (the pow table stays in global memory: a call without the byte table is the exception)
    if (p.tm.sdr.p[0]) ((uint32_t*)p.tm.sdr.p[0])[x + (size_t)y * p.tm.sdr.stride[0]] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
    // ---- generateGainMap on the quantised SDR pixel (jpegr.cpp:753-818 / 866-931), scale 1 ---------------------------
    const Color3 e = {L.unorm.u8[r8], L.unorm.u8[g8], L.unorm.u8[b8]};  // getRgba8888Pixel: byte / 255.0f
    Color3 sl = {L.srgb_of_byte[r8], L.srgb_of_byte[g8], L.srgb_of_byte[b8]};  // the sRGB inverse OETF of e, per byte value
    if (p.gen.sdr_gamut_on) {  // clipNegatives can only bite behind a matrix: table outputs are never negative
      sl = mat3_apply(sl, p.gen.sdr_gamut);
      sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
    }
    Color3 hl = l;  // the same inverse OETF (+ OOTF) the tone mapper just applied
    if (p.gen.hdr_gamut_on) {
      hl = mat3_apply(hl, p.gen.hdr_gamut);
      hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
    }
    gain_of_pixel<TWO_PASS>(sl, hl, p.gen, p.gen.math_tab, x, y, mn, mx, L.gain8);
    // ---- convert_raw_input_to_ycbcr(sdr, 4:4:4) (gainmapmath.cpp:1446-1472) ----------------------------------------------
    const Color3 q = rgb_to_yuv(e, p.base_k);
    ((uint8_t*)p.ycc.p[0])[(size_t)y * p.ycc.stride[0] + x] = (uint8_t)__builtin_amdgcn_fmed3f(q.r * 255.0f + 0.5f, 0.0f, 255.0f);
    ((uint8_t*)p.ycc.p[1])[(size_t)y * p.ycc.stride[1] + x] = (uint8_t)__builtin_amdgcn_fmed3f(q.g * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f);
    ((uint8_t*)p.ycc.p[2])[(size_t)y * p.ycc.stride[2] + x] = (uint8_t)__builtin_amdgcn_fmed3f(q.b * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f);
  }
  if constexpr (TWO_PASS) reduce_block_minmax<kBlock>(mn, mx, partials);
}


// ---- four pixels per lane (round 4) -----------------------------------------------------------------------------------------------
// The kernel above spends a third of its issue slots on per-pixel loop control and wave-uniform branches (61 scalar
// instructions per pixel next to 188 vector ones) and moves single bytes.  Here a lane owns FOUR consecutive pixels of a row:
// one 16-byte load of RGBA1010102, 4-byte stores per base plane, 12 bytes of map (or three 16-byte stores of gain
// ratios), 16 bytes of RGBA8888; gamut mode and channel count are template parameters, so the four pixels are one basic
// block.  Same operations per pixel in the same order -- tests/test_gpu_parity.py holds both kernels to the three operators.
// Requires: RGBA1010102 input, the sRGB byte table (and, one pass, the gain byte table), widths and strides that keep the
// vector accesses aligned (launch_encode_api0_fused checks; anything else runs the kernel above).
struct Fused4Lds {
  float srgb_of_byte[256];
  float hdr[1024];  // 10-bit code -> linear value (unpack + inverse OETF [+ OOTF])
  float u8[256];
  uint2 srgb8[kStepTabMax];
  uint2 gain8[kStepTabMax];
};
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
template <bool TWO_PASS, int GM, int MC, int TG>  // GM: 0 no gamut conversion on the gain side, 1 SDR side, 2 HDR side; TG: tone-map gamut conversion
__global__ __launch_bounds__(kBlock) void encode_api0_fused4_kernel(const FusedParams p, float* partials) {
  __shared__ Fused4Lds L;
  const uint32_t tid = threadIdx.x;
  copy_to_lds(L.srgb_of_byte, p.gen.srgb_of_byte, 256u, tid, kBlock);
  for (uint32_t i = tid; i < 256; i += kBlock) L.u8[i] = (float)i / 255.0f;
  copy_to_lds(L.hdr, p.tm.lin10, 1024u, tid, kBlock);
  stage_step_tab(L.srgb8, p.tm.srgb8, tid, kBlock);
  if constexpr (!TWO_PASS) stage_step_tab(L.gain8, p.gen.gain8, tid, kBlock);
  __syncthreads();
  const uint32_t w4 = p.tm.hdr.w / 4, h = p.tm.hdr.h;
  const uint32_t tiles_x = (w4 + 63) / 64, tiles = tiles_x * h;
  const float inv_tx = 1.0f / (float)tiles_x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (tid >> 6));
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  float mn[3] = {UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT}, mx[3] = {UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT};
  constexpr int NCH = MC ? 3 : 1;
  for (uint32_t t = wave; t < tiles; t += nwaves) {
    uint32_t y = (uint32_t)((float)t * inv_tx);  // t / tiles_x for t < 2^24: the float estimate is off by at most one
    if (y * tiles_x > t) y--;
    if ((y + 1) * tiles_x <= t) y++;
    const uint32_t x4 = (t - y * tiles_x) * 64 + lane;
    if (x4 >= w4) continue;
    const uint32_t x = x4 * 4;
    const u4v in = *(const u4v*)((const uint32_t*)p.tm.hdr.p[0] + (size_t)y * p.tm.hdr.stride[0] + x);
    const uint32_t px[4] = {in.x, in.y, in.z, in.w};
    uint32_t rgba[4], oy = 0, ocb = 0, ocr = 0;
    uint32_t mapb[NCH * 4];   // one pass: the map bytes of the four pixels
    float ratio[NCH * 4];     // two pass: their gain ratios
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // ---- toneMap (jpegr.cpp:2147-2203): unpack + inverse OETF (+ OOTF) of a 10-bit code is one table entry -----------------
      const uint32_t v = px[k];
      const Color3 l = Color3{L.hdr[v & 0x3ffu], L.hdr[(v >> 10) & 0x3ffu], L.hdr[(v >> 20) & 0x3ffu]};
      const Color3 o = tone_curve_linear<TG>(l, p.tm);
      const uint32_t r8 = step_code(o.r, L.srgb8, p.tm.srgb8), g8 = step_code(o.g, L.srgb8, p.tm.srgb8), b8 = step_code(o.b, L.srgb8, p.tm.srgb8);
      rgba[k] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
      // ---- generateGainMap on the quantised SDR pixel (jpegr.cpp:753-818 / 866-931), scale 1 ---------------------------------
      Color3 sl = {L.srgb_of_byte[r8], L.srgb_of_byte[g8], L.srgb_of_byte[b8]};
      if (GM == 1) {
        sl = mat3_apply(sl, p.gen.sdr_gamut);
        sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
      }
      Color3 hl = l;
      if (GM == 2) {
        hl = mat3_apply(hl, p.gen.hdr_gamut);
        hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
      }
      float sn[3], hn[3];
      if (MC) {
        sn[0] = sl.r * 203.0f; sn[1] = sl.g * 203.0f; sn[2] = sl.b * 203.0f;
        hn[0] = hl.r * p.gen.hdr_nits; hn[1] = hl.g * p.gen.hdr_nits; hn[2] = hl.b * p.gen.hdr_nits;
      } else if (p.gen.use_luminance) {  // SDR-gamut luminance coefficients for BOTH images (jpegr.cpp:803-805)
        sn[0] = (p.gen.lum[0] * sl.r + p.gen.lum[1] * sl.g + p.gen.lum[2] * sl.b) * 203.0f;
        hn[0] = (p.gen.lum[0] * hl.r + p.gen.lum[1] * hl.g + p.gen.lum[2] * hl.b) * p.gen.hdr_nits;
      } else {
        sn[0] = fmaxf(sl.r, fmaxf(sl.g, sl.b)) * 203.0f;
        hn[0] = fmaxf(hl.r, fmaxf(hl.g, hl.b)) * p.gen.hdr_nits;
      }
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        if constexpr (!TWO_PASS) {  // encode_gain with its step table (encode_core.h)
          float gain = div_rn(hn[c], __builtin_fmaxf(sn[c], 0x1p-100f));
          gain = sn[c] > 0.0f ? gain : 1.0f;
          mapb[k * NCH + c] = step_code(gain, L.gain8, p.gen.gain8);
        } else {
          const float q = gain_ratio(sn[c], hn[c], p.gen.gain_cap);
          ratio[k * NCH + c] = q;
          mn[c] = __builtin_fminf(mn[c], q);
          mx[c] = __builtin_fmaxf(mx[c], q);
        }
      }
      // ---- convert_raw_input_to_ycbcr(sdr, 4:4:4) (gainmapmath.cpp:1446-1472) ------------------------------------------------
      const Color3 e = {L.u8[r8], L.u8[g8], L.u8[b8]};  // getRgba8888Pixel: byte / 255.0f
      const Color3 q = rgb_to_yuv(e, p.base_k);
      oy |= (uint32_t)__builtin_amdgcn_fmed3f(q.r * 255.0f + 0.5f, 0.0f, 255.0f) << (8 * k);
      ocb |= (uint32_t)__builtin_amdgcn_fmed3f(q.g * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f) << (8 * k);
      ocr |= (uint32_t)__builtin_amdgcn_fmed3f(q.b * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f) << (8 * k);
    }
    if (p.tm.sdr.p[0]) *(u4v*)((uint32_t*)p.tm.sdr.p[0] + (size_t)y * p.tm.sdr.stride[0] + x) = (u4v){rgba[0], rgba[1], rgba[2], rgba[3]};
    *(uint32_t*)((uint8_t*)p.ycc.p[0] + (size_t)y * p.ycc.stride[0] + x) = oy;
    *(uint32_t*)((uint8_t*)p.ycc.p[1] + (size_t)y * p.ycc.stride[1] + x) = ocb;
    *(uint32_t*)((uint8_t*)p.ycc.p[2] + (size_t)y * p.ycc.stride[2] + x) = ocr;
    if constexpr (!TWO_PASS) {
      uint8_t* o = p.gen.out + ((size_t)y * p.gen.out_stride + x) * NCH;
      if (MC) {
        uint32_t wds[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 12; j++) wds[j / 4] |= mapb[j] << (8 * (j & 3));
        *(uint32_t*)o = wds[0]; *(uint32_t*)(o + 4) = wds[1]; *(uint32_t*)(o + 8) = wds[2];
      } else {
        *(uint32_t*)o = mapb[0] | (mapb[1] << 8) | (mapb[2] << 16) | (mapb[3] << 24);
      }
    } else {
      float* g = p.gen.gain_log2 + ((size_t)y * p.gen.map_w + x) * NCH;
#pragma unroll
      for (int j = 0; j < NCH; j++) *(float4*)(g + 4 * j) = float4{ratio[4 * j], ratio[4 * j + 1], ratio[4 * j + 2], ratio[4 * j + 3]};
    }
  }
  if constexpr (TWO_PASS) reduce_block_minmax<kBlock>(mn, mx, partials);
}

template <bool TWO_PASS, int GM, int MC>
void launch_fused4_t(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.tm.gamut_on) hipLaunchKernelGGL((encode_api0_fused4_kernel<TWO_PASS, GM, MC, 1>), dim3(grid), dim3(kBlock), 0, s, p, partials);
  else hipLaunchKernelGGL((encode_api0_fused4_kernel<TWO_PASS, GM, MC, 0>), dim3(grid), dim3(kBlock), 0, s, p, partials);
}
template <bool TWO_PASS, int GM>
void launch_fused4_m(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.gen.multichannel) launch_fused4_t<TWO_PASS, GM, 1>(p, grid, partials, s);
  else launch_fused4_t<TWO_PASS, GM, 0>(p, grid, partials, s);
}
template <bool TWO_PASS>
void launch_fused4(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.gen.sdr_gamut_on) launch_fused4_m<TWO_PASS, 1>(p, grid, partials, s);
  else if (p.gen.hdr_gamut_on) launch_fused4_m<TWO_PASS, 2>(p, grid, partials, s);
  else launch_fused4_m<TWO_PASS, 0>(p, grid, partials, s);
}
// do the 16-byte loads of the intent, the 4-byte stores to the base planes and the 16-byte stores of the rendition stay aligned?
bool fused4_io_aligned(const FusedParams& p) {
  const uint32_t w = p.tm.hdr.w;
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
  if (w % 4 || p.tm.hdr.stride[0] % 4 || !al(p.tm.hdr.p[0], 16)) return false;
  for (int i = 0; i < 3; i++)
    if (p.ycc.stride[i] % 4 || !al(p.ycc.p[i], 4)) return false;
  if (p.tm.sdr.p[0] && (p.tm.sdr.stride[0] % 4 || !al(p.tm.sdr.p[0], 16))) return false;
  return true;
}
bool fused4_ok(const FusedParams& p, bool two_pass) {
  if (p.tm.hdr.fmt != UHDR_IMG_FMT_32bppRGBA1010102 || !p.tm.lin10 || !p.tm.srgb8.tab || !p.gen.srgb_of_byte) return false;
  if (!two_pass && !p.gen.gain8.tab) return false;
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
  if (!fused4_io_aligned(p)) return false;
  const uint32_t nch = p.gen.multichannel ? 3 : 1;
  if (two_pass) return al(p.gen.gain_log2, 16);
  return ((size_t)p.gen.out_stride * nch) % 4 == 0 && al(p.gen.out, 4);
}

// ---- P010 intents: one lane per 2x2 quad ---------------------------------------------------------------------------------------------
// JpegR::encodeJPEGR API-0 on a P010 intent (jpegr.cpp:179-244) is toneMap (P010 -> YCbCr 4:2:0) and generateGainMap; the 4:2:0
// planes are compressed as they are.  Staged that is tonemap_p010_kernel + generate_quad_kernel: 3 + 1.5 bytes per pixel, then
// 1.5 + 3 + 3 again (12 in all for a three-channel map), and every HDR pixel is fetched, converted and linearised twice.  Here a
// lane carries its quad through both: one fetch_quad_p010, yuv_to_rgb + linearisation once per pixel (the gain side's hl IS the
// tone mapper's l, as in the kernels above), tone curve, the four luma bytes and the two mean-chroma bytes of the base image, and
// the gain of each pixel from those QUANTISED bytes with the arithmetic generate_quad_kernel applies to what fetch_quad_420
// returns -- 3 bytes per pixel in, 1.5 + 3 out (7.5 in all), bit for bit the staged route's planes and map
// (tests/test_gpu_api0_p010.py).  A wave walks tiles of 64 consecutive quads of one quad row, like the two staged kernels.
// GAMUT is the HDR intent's gamut as the host's two parameter blocks see it (the SDR rendition is always Display-P3):
//   0 Display-P3: no conversion anywhere; 1 BT.2100: the tone mapper converts to P3 and the gain side converts the SDR pixel
//   to BT.2100; 2 BT.709: the tone mapper converts to P3 and the gain side converts the HDR pixel to P3.
// LDS: HDR linearisation table 16 KB + direct pow table 18 KB + sample normalisation 5 KB + sRGB table 4 KB = 43.2 KB
// (two pass), and one pass adds the gain step table's 16 KB: 59.0 KB.  The staged kernels run four (tone map, 39 KB, 64 VGPRs)
// and three (generate, 25-41 KB, 80 VGPRs) 512-thread workgroups per CU, 32 and 24 waves.  A quad keeps its twelve linear HDR
// values alive across the tone curve, so this kernel needs 69-75 VGPRs: six waves per SIMD, 24 per CU, generate_quad_kernel's
// occupancy, is what the registers allow.  The tables fit that without any of them staying in global memory: two pass,
// three 512-thread workgroups (130 of 160 KB); one pass, two 768-thread workgroups (118 KB) -- twelve waves share a table
// set instead of eight.  (Every table is read several times per pixel, the step and pow tables through address forms that
// exist for LDS only: encode_core.h step_code, srgb_oetf_lds.)  No scratch.
struct alignas(16) FusedQuadLds {  // (16-byte table reads and copies)
  float hdr[kInvOetfN];
  double powt[kPowDirDoubles];
  float srgb[kSrgbN];
  UnormTables unorm;
};
constexpr int quad_block(bool two_pass) { return two_pass ? 512 : 768; }
template <bool TWO_PASS, int GAMUT, int MC, bool LUT>
__global__ __launch_bounds__(quad_block(TWO_PASS)) void encode_api0_p010_fused_kernel(const FusedParams p, float* partials) {
  constexpr int kQuadBlock = quad_block(TWO_PASS);
  __shared__ FusedQuadLds L;
  __shared__ alignas(16) uint2 s_gain8[TWO_PASS ? 1 : kStepTabMax];
  const uint32_t tid = threadIdx.x;
  if constexpr (!TWO_PASS) stage_step_tab(s_gain8, p.gen.gain8, tid, kQuadBlock);
  if (LUT) copy_to_lds(L.hdr, p.tm.hdr_inv_lut, (uint32_t)p.tm.hdr_inv_n, tid, kQuadBlock);
  stage_pow_tab(L.powt, p.tm.math_tab, tid, kQuadBlock);
  copy_to_lds(L.srgb, p.gen.srgb_lut, (uint32_t)kSrgbN, tid, kQuadBlock);
  fill_unorm_tables(L.unorm, tid, kQuadBlock);
  __syncthreads();
  float mn[3] = {UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT}, mx[3] = {UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT};
  const uint32_t qw = p.tm.hdr.w / 2, qh = p.tm.hdr.h / 2;
  const uint32_t tiles_x = (qw + 63) / 64, tiles = tiles_x * qh;
  const float inv_tx = 1.0f / (float)tiles_x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kQuadBlock / 64) + (tid >> 6));
  const uint32_t nwaves = gridDim.x * (kQuadBlock / 64);
  const float lut_scale = (float)(p.tm.hdr_inv_n - 1);  // lut_index: x * (N - 1), round half up (encode_core.h: rpi)
  uint8_t* yp = (uint8_t*)p.tm.sdr.p[0];
  uint8_t* up = (uint8_t*)p.tm.sdr.p[1];
  uint8_t* vp = (uint8_t*)p.tm.sdr.p[2];
  for (uint32_t t = wave; t < tiles; t += nwaves) {
    uint32_t qy = (uint32_t)((float)t * inv_tx);  // t / tiles_x for t < 2^24: the float estimate is off by at most one
    if (qy * tiles_x > t) qy--;
    if ((qy + 1) * tiles_x <= t) qy++;
    const uint32_t qx = (t - qy * tiles_x) * 64 + lane;
    if (qx >= qw) continue;
    const QuadYuv hq = fetch_quad_p010(p.tm.hdr, qx, qy, &L.unorm);
    Color3 l[4];  // linear HDR rgb: the tone mapper's input AND the gain side's HDR pixel
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const Color3 g = yuv_to_rgb(hq.px[k].r, hq.px[k].g, hq.px[k].b, p.tm.hdr_yuv);  // in [0, 1]
      l[k] = g;
      if (LUT) l[k] = Color3{L.hdr[rpi(g.r * lut_scale)], L.hdr[rpi(g.g * lut_scale)], L.hdr[rpi(g.b * lut_scale)]};
    }
    // ---- toneMap (jpegr.cpp:2147-2203), as tonemap_p010_kernel -----------------------------------------------------------------
    float su = 0.0f, sv = 0.0f;
    uint32_t yb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // (row, column) order: the chroma sums accumulate like the reference's
      const Color3 og = tone_curve<(GAMUT != 0) ? 1 : 0>(l[k], p.tm, L.powt);
      Color3 yuv = rgb_to_yuv(og, p.tm.p3);
      yuv.g += 0.5f;
      yuv.b += 0.5f;
      yb[k] = scale_to_8bit(yuv.r);
      su += yuv.g;
      sv += yuv.b;
    }
    su *= 0.25f;  // x / 4.0f == x * 0.25f exactly
    sv *= 0.25f;
    const uint32_t ub = scale_to_8bit(su), vb = scale_to_8bit(sv);
    const size_t sy = p.tm.sdr.stride[0];
    uint8_t* y0 = yp + (size_t)(qy * 2) * sy + qx * 2;  // (the host checked quad_layout_ok: 16-bit stores stay aligned)
    *(uint16_t*)y0 = (uint16_t)(yb[0] | (yb[1] << 8));
    *(uint16_t*)(y0 + sy) = (uint16_t)(yb[2] | (yb[3] << 8));
    up[(size_t)qy * p.tm.sdr.stride[1] + qx] = (uint8_t)ub;
    vp[(size_t)qy * p.tm.sdr.stride[2] + qx] = (uint8_t)vb;
    // ---- generateGainMap on the quantised bytes (jpegr.cpp:753-818 / 866-931), as generate_quad_kernel reads them back ---------
    const float cu = (float)((int)ub - 128) * (1 / 255.0f), cv = (float)((int)vb - 128) * (1 / 255.0f);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const Color3 s = yuv_to_rgb((float)(int)yb[k] * (1 / 255.0f), cu, cv, p.gen.sdr_yuv);  // in [0, 1]
      Color3 sl = lut3_unit<kSrgbN>(s, L.srgb);
      Color3 hl = l[k];
      if (GAMUT == 1) {  // clipNegatives (jpegr.cpp:783-784) can only bite behind a matrix: table outputs are never negative
        sl = mat3_apply(sl, p.gen.sdr_gamut);
        sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
      }
      if (GAMUT == 2) {
        hl = mat3_apply(hl, p.gen.hdr_gamut);
        hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
      }
      gain_of_pixel<TWO_PASS, MC>(sl, hl, p.gen, p.gen.math_tab, 2 * qx + (k & 1), 2 * qy + (k >> 1), mn, mx, TWO_PASS ? nullptr : s_gain8);
    }
  }
  if constexpr (TWO_PASS) reduce_block_minmax<kQuadBlock>(mn, mx, partials);
}

template <bool TWO_PASS, int GAMUT, int MC>
void launch_p010_l(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.tm.hdr_inv_lut) hipLaunchKernelGGL((encode_api0_p010_fused_kernel<TWO_PASS, GAMUT, MC, true>), dim3(grid), dim3(quad_block(TWO_PASS)), 0, s, p, partials);
  else hipLaunchKernelGGL((encode_api0_p010_fused_kernel<TWO_PASS, GAMUT, MC, false>), dim3(grid), dim3(quad_block(TWO_PASS)), 0, s, p, partials);
}
template <bool TWO_PASS, int GAMUT>
void launch_p010_m(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.gen.multichannel) launch_p010_l<TWO_PASS, GAMUT, 1>(p, grid, partials, s);
  else launch_p010_l<TWO_PASS, GAMUT, 0>(p, grid, partials, s);
}
template <bool TWO_PASS>
void launch_p010(const FusedParams& p, int grid, float* partials, hipStream_t s) {
  if (p.gen.sdr_gamut_on) launch_p010_m<TWO_PASS, 1>(p, grid, partials, s);
  else if (p.gen.hdr_gamut_on) launch_p010_m<TWO_PASS, 2>(p, grid, partials, s);
  else launch_p010_m<TWO_PASS, 0>(p, grid, partials, s);
}

// ---- gain maps at scale factor 2 and 4 (one pass) -------------------------------------------------------------------------------------
// A sub-sampled map (kMapDimensionScaleFactorAndroidDefault = 4, ultrahdrcommon.h:425) used to cost three full-image launches: the tone
// map, generate_kernel -- one thread per map pixel, fetching its S x S box of BOTH images one pixel at a time, neighbouring lanes S pixels
// apart -- and, for RGB intents, convert_raw_input_to_ycbcr: about 23 bytes per pixel for RGBA1010102 at S = 4.  The two kernels below are
// the kernels above with the gain side replaced by generate_kernel's: samplePixels (gainmapmath.cpp:494-503) averages the GAMMA-ENCODED
// samples of the box and the mean is linearised, so a lane sums what fetch_pixel would return for the bytes it has just written (u8[byte],
// or y / 255 and (u - 128) / 255) and for the HDR codes it has just read (u10[code], or fetch_quad_p010's values), from 0.0f, dy outer and dx
// inner, divides by S * S and goes on exactly as generate_kernel does from its two sample_box results.  One pass only (API-0 overrides the
// preset to UHDR_USAGE_REALTIME, jpegr.cpp:207).  4 + 3 + 3/16 bytes per pixel (RGBA1010102, S = 4, one channel); the SDR bytes never come
// back from HBM.  GAMUT as in encode_api0_p010_fused_kernel (the SDR rendition is Display-P3, so the tone mapper converts exactly when the
// gain side does).  A call without a gain step table (gamma != 1) evaluates encode_gain per map pixel, as generate_kernel does.
// LDS, RGBA1010102: code -> linear 4 KB + HDR inverse OETF 16 KB + sRGB inverse OETF 4 KB + sample normalisation 5 KB + the two step
// tables 32 KB = 61 KB; P010: FusedQuadLds 43.2 KB + the gain step table 16 KB = 59 KB.  A cell keeps its box sums and S rows of loads alive
// beside the tone curve: 67-116 VGPRs (RGBA1010102 at S = 4 with two rows in flight: 116; all four: 143), so the one-pass P010 kernel's two
// 768-thread workgroups (six waves per SIMD, 80 VGPRs) would leave one resident.  Both kernels: two 512-thread workgroups per CU (16 waves,
// four per SIMD -- __launch_bounds__ holds the allocation to 128 --, 118-122 of 160 KB).  No scratch.
constexpr int kScaledBlock = 512;
struct FusedScaledLds {
  float lin10[1024];     // tone map: 10-bit code -> linear value (unpack + inverse OETF [+ OOTF])
  float hdr[kInvOetfN];  // gain side: the HDR inverse OETF of the box mean (none for a linear intent)
  float srgb[kSrgbN];    // gain side: the sRGB inverse OETF of the box mean
  UnormTables unorm;
  uint2 srgb8[kStepTabMax];
};

// RGBA1010102: a lane owns a cell of 4 consecutive pixels x S rows (one map pixel at S = 4, two at S = 2); a wave walks tiles of 64 cells
// = 256 pixels of one strip of S image rows.
template <int S, int GAMUT, int MC>
__global__ __launch_bounds__(kScaledBlock, 4) void encode_api0_fused4_scaled_kernel(const FusedParams p) {
  __shared__ FusedScaledLds L;
  __shared__ alignas(16) uint2 s_gain8[kStepTabMax];
  const uint32_t tid = threadIdx.x;
  copy_to_lds(L.lin10, p.tm.lin10, 1024u, tid, kScaledBlock);
  if (p.gen.hdr_inv_lut) copy_to_lds(L.hdr, p.gen.hdr_inv_lut, (uint32_t)p.gen.hdr_inv_n, tid, kScaledBlock);
  copy_to_lds(L.srgb, p.gen.srgb_lut, (uint32_t)kSrgbN, tid, kScaledBlock);
  fill_unorm_tables(L.unorm, tid, kScaledBlock);
  stage_step_tab(L.srgb8, p.tm.srgb8, tid, kScaledBlock);
  stage_step_tab(s_gain8, p.gen.gain8, tid, kScaledBlock);
  __syncthreads();
  const uint32_t w4 = p.tm.hdr.w / 4, strips = p.tm.hdr.h / S;
  const uint32_t tiles_x = (w4 + 63) / 64, tiles = tiles_x * strips;
  const float inv_tx = 1.0f / (float)tiles_x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScaledBlock / 64) + (tid >> 6));
  const uint32_t nwaves = gridDim.x * (kScaledBlock / 64);
  const bool hdr_lut = p.gen.hdr_inv_lut != nullptr, hdr_lut_4096 = p.gen.hdr_inv_n == kInvOetfN;
  constexpr int NBOX = 4 / S;  // map pixels per cell
  for (uint32_t t = wave; t < tiles; t += nwaves) {
    uint32_t sy = (uint32_t)((float)t * inv_tx);  // t / tiles_x for t < 2^24: the float estimate is off by at most one
    if (sy * tiles_x > t) sy--;
    if ((sy + 1) * tiles_x <= t) sy++;
    const uint32_t x4 = (t - sy * tiles_x) * 64 + lane;
    if (x4 >= w4) continue;
    const uint32_t x = x4 * 4;
    Color3 ss[NBOX], hs[NBOX];  // samplePixels' sums of the two images
#pragma unroll
    for (int b = 0; b < NBOX; b++) ss[b] = hs[b] = Color3{0.0f, 0.0f, 0.0f};
#pragma unroll 2  // two rows' loads in flight per lane; four rows unrolled need 143 VGPRs
    for (int dy = 0; dy < S; dy++) {
      const uint32_t y = sy * S + dy;
      const u4v in = *(const u4v*)((const uint32_t*)p.tm.hdr.p[0] + (size_t)y * p.tm.hdr.stride[0] + x);
      const uint32_t px[4] = {in.x, in.y, in.z, in.w};
      uint32_t rgba[4], oy = 0, ocb = 0, ocr = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        // ---- toneMap (jpegr.cpp:2147-2203): unpack + inverse OETF (+ OOTF) of a 10-bit code is one table entry -----------------
        const uint32_t v = px[k];
        const uint32_t c0 = v & 0x3ffu, c1 = (v >> 10) & 0x3ffu, c2 = (v >> 20) & 0x3ffu;
        const Color3 l = Color3{L.lin10[c0], L.lin10[c1], L.lin10[c2]};
        const Color3 o = tone_curve_linear<(GAMUT != 0) ? 1 : 0>(l, p.tm);
        const uint32_t r8 = step_code(o.r, L.srgb8, p.tm.srgb8), g8 = step_code(o.g, L.srgb8, p.tm.srgb8), b8 = step_code(o.b, L.srgb8, p.tm.srgb8);
        rgba[k] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
        // ---- convert_raw_input_to_ycbcr(sdr, 4:4:4) (gainmapmath.cpp:1446-1472) ------------------------------------------------
        const Color3 e = {L.unorm.u8[r8], L.unorm.u8[g8], L.unorm.u8[b8]};  // getRgba8888Pixel: byte / 255.0f
        const Color3 q = rgb_to_yuv(e, p.base_k);
        oy |= (uint32_t)__builtin_amdgcn_fmed3f(q.r * 255.0f + 0.5f, 0.0f, 255.0f) << (8 * k);
        ocb |= (uint32_t)__builtin_amdgcn_fmed3f(q.g * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f) << (8 * k);
        ocr |= (uint32_t)__builtin_amdgcn_fmed3f(q.b * 255.0f + 0.5f + 128.0f, 0.0f, 255.0f) << (8 * k);
        // ---- samplePixels (gainmapmath.cpp:494-503) of both images: what fetch_pixel returns for these bytes and these codes -----
        Color3& sb = ss[k / S];  // (a constant index once unrolled)
        Color3& hb = hs[k / S];
        sb.r += e.r; sb.g += e.g; sb.b += e.b;
        hb.r += L.unorm.u10[c0]; hb.g += L.unorm.u10[c1]; hb.b += L.unorm.u10[c2];
      }
      if (p.tm.sdr.p[0]) *(u4v*)((uint32_t*)p.tm.sdr.p[0] + (size_t)y * p.tm.sdr.stride[0] + x) = (u4v){rgba[0], rgba[1], rgba[2], rgba[3]};
      *(uint32_t*)((uint8_t*)p.ycc.p[0] + (size_t)y * p.ycc.stride[0] + x) = oy;
      *(uint32_t*)((uint8_t*)p.ycc.p[1] + (size_t)y * p.ycc.stride[1] + x) = ocb;
      *(uint32_t*)((uint8_t*)p.ycc.p[2] + (size_t)y * p.ycc.stride[2] + x) = ocr;
    }
    // ---- generateGainMap (jpegr.cpp:753-818) from the two box means, as generate_kernel ----------------------------------------------
#pragma unroll
    for (int b = 0; b < NBOX; b++) {
      const float d = (float)(S * S);
      const Color3 s = {ss[b].r / d, ss[b].g / d, ss[b].b / d}, h = {hs[b].r / d, hs[b].g / d, hs[b].b / d};
      Color3 sl = linearise_hdr(s, L.srgb, true, false);  // the 1024-entry sRGB table; box means of RGB samples stay in [0, 1]
      if (GAMUT == 1) {  // clipNegatives (jpegr.cpp:783-784) can only bite behind a matrix: table outputs are never negative
        sl = mat3_apply(sl, p.gen.sdr_gamut);
        sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
      }
      Color3 hl = linearise_hdr(h, L.hdr, hdr_lut, hdr_lut_4096);
      if (GAMUT == 2) {
        hl = mat3_apply(hl, p.gen.hdr_gamut);
        hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
      }
      gain_of_pixel<false, MC>(sl, hl, p.gen, p.gen.math_tab, x4 * NBOX + b, sy, nullptr, nullptr, s_gain8);  // (no extrema in one pass)
    }
  }
}

// P010: a lane owns an S x S box (one quad at S = 2, 2 x 2 quads at S = 4); a wave walks tiles of 64 consecutive boxes of one box row.
template <int S, int GAMUT, int MC, bool LUT>
__global__ __launch_bounds__(kScaledBlock, 4) void encode_api0_p010_fused_scaled_kernel(const FusedParams p) {
  __shared__ FusedQuadLds L;
  __shared__ alignas(16) uint2 s_gain8[kStepTabMax];
  const uint32_t tid = threadIdx.x;
  stage_step_tab(s_gain8, p.gen.gain8, tid, kScaledBlock);
  if (LUT) copy_to_lds(L.hdr, p.tm.hdr_inv_lut, (uint32_t)p.tm.hdr_inv_n, tid, kScaledBlock);
  stage_pow_tab(L.powt, p.tm.math_tab, tid, kScaledBlock);
  copy_to_lds(L.srgb, p.gen.srgb_lut, (uint32_t)kSrgbN, tid, kScaledBlock);
  fill_unorm_tables(L.unorm, tid, kScaledBlock);
  __syncthreads();
  constexpr int Q = S / 2;  // quads per box side
  const uint32_t bw = p.tm.hdr.w / S, bh = p.tm.hdr.h / S;
  const uint32_t tiles_x = (bw + 63) / 64, tiles = tiles_x * bh;
  const float inv_tx = 1.0f / (float)tiles_x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScaledBlock / 64) + (tid >> 6));
  const uint32_t nwaves = gridDim.x * (kScaledBlock / 64);
  const float lut_scale = (float)(p.tm.hdr_inv_n - 1);  // lut_index: x * (N - 1), round half up (encode_core.h: rpi)
  const bool hdr_lut_4096 = p.gen.hdr_inv_n == kInvOetfN;
  uint8_t* yp = (uint8_t*)p.tm.sdr.p[0];
  uint8_t* up = (uint8_t*)p.tm.sdr.p[1];
  uint8_t* vp = (uint8_t*)p.tm.sdr.p[2];
  for (uint32_t t = wave; t < tiles; t += nwaves) {
    uint32_t by = (uint32_t)((float)t * inv_tx);  // t / tiles_x for t < 2^24: the float estimate is off by at most one
    if (by * tiles_x > t) by--;
    if ((by + 1) * tiles_x <= t) by++;
    const uint32_t bx = (t - by * tiles_x) * 64 + lane;
    if (bx >= bw) continue;
    Color3 ss = {0.0f, 0.0f, 0.0f}, hs = {0.0f, 0.0f, 0.0f};  // samplePixels' sums of the two images (y, u, v)
#pragma unroll
    for (int j = 0; j < Q; j++) {  // quad rows of the box
      float sy_[Q][4], hy_[Q][4], scu[Q], scv[Q], hcu[Q], hcv[Q];
#pragma unroll
      for (int i = 0; i < Q; i++) {
        const uint32_t qx = bx * Q + i, qy = by * Q + j;
        const QuadYuv hq = fetch_quad_p010(p.tm.hdr, qx, qy, &L.unorm);
        Color3 l[4];  // linear HDR rgb: the tone mapper's input
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const Color3 g = yuv_to_rgb(hq.px[k].r, hq.px[k].g, hq.px[k].b, p.tm.hdr_yuv);  // in [0, 1]
          l[k] = g;
          if (LUT) l[k] = Color3{L.hdr[rpi(g.r * lut_scale)], L.hdr[rpi(g.g * lut_scale)], L.hdr[rpi(g.b * lut_scale)]};
        }
        // ---- toneMap (jpegr.cpp:2147-2203), as tonemap_p010_kernel -----------------------------------------------------------------
        float su = 0.0f, sv = 0.0f;
        uint32_t yb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {  // (row, column) order: the chroma sums accumulate like the reference's
          const Color3 og = tone_curve<(GAMUT != 0) ? 1 : 0>(l[k], p.tm, L.powt);
          Color3 yuv = rgb_to_yuv(og, p.tm.p3);
          yuv.g += 0.5f;
          yuv.b += 0.5f;
          yb[k] = scale_to_8bit(yuv.r);
          su += yuv.g;
          sv += yuv.b;
        }
        su *= 0.25f;  // x / 4.0f == x * 0.25f exactly
        sv *= 0.25f;
        const uint32_t ub = scale_to_8bit(su), vb = scale_to_8bit(sv);
        const size_t sy = p.tm.sdr.stride[0];
        uint8_t* y0 = yp + (size_t)(qy * 2) * sy + qx * 2;  // (the host checked quad_layout_ok: 16-bit stores stay aligned)
        *(uint16_t*)y0 = (uint16_t)(yb[0] | (yb[1] << 8));
        *(uint16_t*)(y0 + sy) = (uint16_t)(yb[2] | (yb[3] << 8));
        up[(size_t)qy * p.tm.sdr.stride[1] + qx] = (uint8_t)ub;
        vp[(size_t)qy * p.tm.sdr.stride[2] + qx] = (uint8_t)vb;
        // what fetch_pixel returns for the bytes just written, and what fetch_quad_p010 returned
        scu[i] = (float)((int)ub - 128) * (1 / 255.0f);
        scv[i] = (float)((int)vb - 128) * (1 / 255.0f);
        hcu[i] = hq.px[0].g;
        hcv[i] = hq.px[0].b;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          sy_[i][k] = (float)(int)yb[k] * (1 / 255.0f);
          hy_[i][k] = hq.px[k].r;
        }
      }
      // ---- samplePixels (gainmapmath.cpp:494-503): box order is dy outer, dx inner -- row 0 of the left quad, row 0 of the right one, ... ----
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int i = 0; i < Q; i++)
#pragma unroll
          for (int cx = 0; cx < 2; cx++) {
            ss.r += sy_[i][2 * r + cx]; ss.g += scu[i]; ss.b += scv[i];
            hs.r += hy_[i][2 * r + cx]; hs.g += hcu[i]; hs.b += hcv[i];
          }
    }
    // ---- generateGainMap (jpegr.cpp:753-818) from the two box means, as generate_kernel for a YCbCr pair ----------------------------------
    const float d = (float)(S * S);
    const Color3 s = yuv_to_rgb(ss.r / d, ss.g / d, ss.b / d, p.gen.sdr_yuv);
    Color3 sl = linearise_hdr(s, L.srgb, true, false);
    if (GAMUT == 1) {  // clipNegatives (jpegr.cpp:783-784) can only bite behind a matrix: table outputs are never negative
      sl = mat3_apply(sl, p.gen.sdr_gamut);
      sl.r = clip_neg(sl.r); sl.g = clip_neg(sl.g); sl.b = clip_neg(sl.b);
    }
    const Color3 h = yuv_to_rgb(hs.r / d, hs.g / d, hs.b / d, p.gen.hdr_yuv);
    Color3 hl = linearise_hdr(h, L.hdr, LUT, hdr_lut_4096);
    if (GAMUT == 2) {
      hl = mat3_apply(hl, p.gen.hdr_gamut);
      hl.r = clip_neg(hl.r); hl.g = clip_neg(hl.g); hl.b = clip_neg(hl.b);
    }
    gain_of_pixel<false, MC>(sl, hl, p.gen, p.gen.math_tab, bx, by, nullptr, nullptr, s_gain8);  // (no extrema in one pass)
  }
}

template <int S, int GAMUT>
void launch_fused4_scaled_m(const FusedParams& p, int grid, hipStream_t s) {
  if (p.gen.multichannel) hipLaunchKernelGGL((encode_api0_fused4_scaled_kernel<S, GAMUT, 1>), dim3(grid), dim3(kScaledBlock), 0, s, p);
  else hipLaunchKernelGGL((encode_api0_fused4_scaled_kernel<S, GAMUT, 0>), dim3(grid), dim3(kScaledBlock), 0, s, p);
}
template <int S>
void launch_fused4_scaled(const FusedParams& p, int grid, hipStream_t s) {
  if (p.gen.sdr_gamut_on) launch_fused4_scaled_m<S, 1>(p, grid, s);
  else if (p.gen.hdr_gamut_on) launch_fused4_scaled_m<S, 2>(p, grid, s);
  else launch_fused4_scaled_m<S, 0>(p, grid, s);
}
template <int S, int GAMUT, int MC>
void launch_p010_scaled_l(const FusedParams& p, int grid, hipStream_t s) {
  if (p.tm.hdr_inv_lut) hipLaunchKernelGGL((encode_api0_p010_fused_scaled_kernel<S, GAMUT, MC, true>), dim3(grid), dim3(kScaledBlock), 0, s, p);
  else hipLaunchKernelGGL((encode_api0_p010_fused_scaled_kernel<S, GAMUT, MC, false>), dim3(grid), dim3(kScaledBlock), 0, s, p);
}
template <int S, int GAMUT>
void launch_p010_scaled_m(const FusedParams& p, int grid, hipStream_t s) {
  if (p.gen.multichannel) launch_p010_scaled_l<S, GAMUT, 1>(p, grid, s);
  else launch_p010_scaled_l<S, GAMUT, 0>(p, grid, s);
}
template <int S>
void launch_p010_scaled(const FusedParams& p, int grid, hipStream_t s) {
  if (p.gen.sdr_gamut_on) launch_p010_scaled_m<S, 1>(p, grid, s);
  else if (p.gen.hdr_gamut_on) launch_p010_scaled_m<S, 2>(p, grid, s);
  else launch_p010_scaled_m<S, 0>(p, grid, s);
}
// the three gamut modes: the SDR rendition is Display-P3, so the tone mapper converts exactly when the gain side does
bool scaled_gamut_ok(const FusedParams& p) {
  return (p.tm.gamut_on != 0) == (p.gen.sdr_gamut_on || p.gen.hdr_gamut_on) && !(p.gen.sdr_gamut_on && p.gen.hdr_gamut_on);
}

}  // namespace

int fused_grid(uint32_t tiles, int per_cu) {
  const int cus = device_cu_count();
  const int resident = cus * per_cu;  // 512-thread workgroups: 48 KB of LDS tables (RGBA1010102) -> 3 per CU, 60 KB (RGBA-F16) -> 2
  uint32_t g = tiles < (uint32_t)resident ? tiles : (uint32_t)resident;
  if (g > 2048) g = 2048;  // the host layer sizes the min/max partials buffer for 2048 workgroups
  return (int)(g < 1 ? 1 : g);
}

// two_pass: p.gen.gain_log2 / p.gen.minmax set as for launch_generate_gainmap; returns the grid size (= the number of
// ratio-extrema partials at p.gen.minmax + 6) through *grid_out for launch_minmax_table.
hipError_t launch_encode_api0_fused(const FusedParams& p, bool two_pass, int* grid_out, hipStream_t s) {
  float* partials4 = two_pass ? p.gen.minmax + 6 : nullptr;
  if (fused4_ok(p, two_pass)) {
    const uint32_t wave_tiles = ((p.tm.hdr.w / 4 + 63) / 64) * p.tm.hdr.h;
    const int grid = fused_grid((wave_tiles + kBlock / 64 - 1) / (kBlock / 64), 4);  // 39 KB of LDS tables: four 512-thread workgroups per CU
    if (grid_out) *grid_out = grid;
    if (two_pass) launch_fused4<true>(p, grid, partials4, s);
    else launch_fused4<false>(p, grid, partials4, s);
    return hipGetLastError();
  }
  const uint32_t tiles = ((p.tm.hdr.w + kBlock - 1) / kBlock) * p.tm.hdr.h;
  const bool f16 = p.tm.hdr.fmt == UHDR_IMG_FMT_64bppRGBAHalfFloat;
  if (!f16 && !p.tm.lin10) return hipErrorInvalidValue;  // the host layer always builds the code -> linear table
  const int grid = fused_grid(tiles, f16 ? 2 : 3);
  if (grid_out) *grid_out = grid;
  float* partials = two_pass ? p.gen.minmax + 6 : nullptr;
  if (f16) {
    if (two_pass) hipLaunchKernelGGL((encode_api0_fused_kernel<UHDR_IMG_FMT_64bppRGBAHalfFloat, true>), dim3(grid), dim3(kBlock), 0, s, p, partials);
    else hipLaunchKernelGGL((encode_api0_fused_kernel<UHDR_IMG_FMT_64bppRGBAHalfFloat, false>), dim3(grid), dim3(kBlock), 0, s, p, partials);
  } else {
    if (two_pass) hipLaunchKernelGGL((encode_api0_fused_kernel<UHDR_IMG_FMT_32bppRGBA1010102, true>), dim3(grid), dim3(kBlock), 0, s, p, partials);
    else hipLaunchKernelGGL((encode_api0_fused_kernel<UHDR_IMG_FMT_32bppRGBA1010102, false>), dim3(grid), dim3(kBlock), 0, s, p, partials);
  }
  return hipGetLastError();
}

bool encode_api0_p010_layout_ok(const ImageView& hdr, const ImageView& base420) { return quad_layout_ok(hdr) && quad_layout_ok(base420); }

// P010 intent -> p.tm.sdr (YCbCr 4:2:0 planes) + the map; p.ycc / p.base_k are unused.  The caller has checked quad_layout_ok for
// p.tm.hdr and the base planes, scale factor 1 and the tables; two_pass / grid_out as for launch_encode_api0_fused.
hipError_t launch_encode_api0_p010_fused(const FusedParams& p, bool two_pass, int* grid_out, hipStream_t s) {
  if (p.tm.hdr.fmt != UHDR_IMG_FMT_24bppYCbCrP010 || p.tm.sdr.fmt != UHDR_IMG_FMT_12bppYCbCr420 || !quad_layout_ok(p.tm.hdr) || p.tm.sdr.w != p.tm.hdr.w ||
      p.tm.sdr.h != p.tm.hdr.h || p.tm.sdr.stride[0] % 2 || ((uintptr_t)p.tm.sdr.p[0] % 2) || p.gen.scale != 1 || p.gen.map_w != p.tm.hdr.w ||
      p.gen.map_h != p.tm.hdr.h || !p.gen.srgb_lut || !p.tm.math_tab)
    return hipErrorInvalidValue;
  // the three gamut modes: the SDR rendition is Display-P3, so the tone mapper converts exactly when the gain side does
  if ((p.tm.gamut_on != 0) != (p.gen.sdr_gamut_on || p.gen.hdr_gamut_on) || (p.gen.sdr_gamut_on && p.gen.hdr_gamut_on)) return hipErrorInvalidValue;
  const uint32_t wave_tiles = ((p.tm.hdr.w / 2 + 63) / 64) * (p.tm.hdr.h / 2);
  const uint32_t wg_waves = (uint32_t)quad_block(two_pass) / 64;
  const int grid = fused_grid((wave_tiles + wg_waves - 1) / wg_waves, two_pass ? 3 : 2);  // 43 / 59 KB of LDS tables per workgroup: 24 waves per CU either way
  if (grid_out) *grid_out = grid;
  float* partials = two_pass ? p.gen.minmax + 6 : nullptr;
  if (two_pass) launch_p010<true>(p, grid, partials, s);
  else launch_p010<false>(p, grid, partials, s);
  return hipGetLastError();
}

// ---- scale factor 2 / 4, one pass ---------------------------------------------------------------------------------------------------
// what the scaled kernels read and write with vector accesses (the map is stored byte by byte: any stride and base)
bool encode_api0_fused_scaled_layout_ok(const FusedParams& p) { return p.tm.hdr.fmt == UHDR_IMG_FMT_32bppRGBA1010102 && fused4_io_aligned(p); }

static int scaled_grid(uint32_t wave_tiles) {
  const uint32_t wg_waves = (uint32_t)kScaledBlock / 64;
  return fused_grid((wave_tiles + wg_waves - 1) / wg_waves, 2);  // 59-61 KB of LDS tables per 512-thread workgroup: 16 waves per CU
}

// RGBA1010102 intent -> p.ycc (4:4:4 planes), the optional p.tm.sdr rendition and the one-pass map of (w / S) x (h / S) pixels, S = p.gen.scale
// (2 or 4).  The caller has checked encode_api0_fused_scaled_layout_ok, w % 4 == 0 and h % S == 0.
hipError_t launch_encode_api0_fused_scaled(const FusedParams& p, hipStream_t s) {
  const uint32_t S = p.gen.scale, w = p.tm.hdr.w, h = p.tm.hdr.h;
  if ((S != 2 && S != 4) || !encode_api0_fused_scaled_layout_ok(p) || w == 0 || h == 0 || h % S || p.gen.map_w != w / S || p.gen.map_h != h / S ||
      !p.tm.lin10 || !p.tm.srgb8.tab || !p.gen.srgb_lut || !p.gen.out || p.gen.out_stride < p.gen.map_w || !scaled_gamut_ok(p))
    return hipErrorInvalidValue;
  const int grid = scaled_grid(((w / 4 + 63) / 64) * (h / S));
  if (S == 2) launch_fused4_scaled<2>(p, grid, s);
  else launch_fused4_scaled<4>(p, grid, s);
  return hipGetLastError();
}

// P010 intent -> p.tm.sdr (YCbCr 4:2:0 planes) + the one-pass map, S = p.gen.scale (2 or 4).  The caller has checked quad_layout_ok for
// p.tm.hdr and the base planes, w % 4 == 0 and h % S == 0.
hipError_t launch_encode_api0_p010_fused_scaled(const FusedParams& p, hipStream_t s) {
  const uint32_t S = p.gen.scale, w = p.tm.hdr.w, h = p.tm.hdr.h;
  if ((S != 2 && S != 4) || p.tm.hdr.fmt != UHDR_IMG_FMT_24bppYCbCrP010 || p.tm.sdr.fmt != UHDR_IMG_FMT_12bppYCbCr420 || !quad_layout_ok(p.tm.hdr) ||
      p.tm.sdr.w != w || p.tm.sdr.h != h || p.tm.sdr.stride[0] % 2 || ((uintptr_t)p.tm.sdr.p[0] % 2) || w == 0 || h == 0 || w % S || h % S ||
      p.gen.map_w != w / S || p.gen.map_h != h / S || !p.gen.srgb_lut || !p.tm.math_tab || !p.gen.out || p.gen.out_stride < p.gen.map_w || !scaled_gamut_ok(p))
    return hipErrorInvalidValue;
  const int grid = scaled_grid(((w / S + 63) / 64) * (h / S));
  if (S == 2) launch_p010_scaled<2>(p, grid, s);
  else launch_p010_scaled<4>(p, grid, s);
  return hipGetLastError();
}

}  // namespace uhdr
