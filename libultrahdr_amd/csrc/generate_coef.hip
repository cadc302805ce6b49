// generateGainMap with the SDR intent still in JPEG coefficient form: JpegR::encodeJPEGR API-3
// (lib/src/jpegr.cpp:327-385 of the reference) decodes the compressed SDR intent and hands the planes to generateGainMap
// (jpegr.cpp:530-1050).  Here JpegDecoderHelper's dequantize + IDCT stage (jpegdecoderhelper.cpp:468-535) runs inside pass 1
// (or the whole one-pass generation): the 8-bit SDR planes never exist in HBM.  The mirror of apply_quad_body<..., SRC = 1>
// (apply_gainmap.hip) on the encode side.
//
// A WAVE takes a 128 x 16 pixel tile: 32 luma + 8 + 8 chroma blocks at 4:2:0, 32 + 16 + 16 at 4:2:2; at 4:4:4 the tile is an MCU
// row of 128 x 8 pixels, 16 + 16 + 16 blocks (coef_tile::Geom<SAMPLING>).  It dequantises and inverse-transforms them through
// the stage both kernels share (coef_tile.h: the unit layout, the loads, the
// transforms and the stores into the wave's LDS tile; here the luma units, then the chroma units), then produces the tile's
// map pixels with generate_kernel's sequence of operations (generate_gainmap.hip): the SDR sample is what fetch_pixel returns
// for the byte the stand-alone IDCT would have stored, box sums run dy outer / dx inner from 0.0f with one divide, and
// everything behind the sample is the shared code of encode_core.h.  Scale factors 1, 2 and 4 divide the tile, so a box
// never leaves it (the host declines the others).  Pixels of the coefficient grid beyond w x h are transformed and never
// sampled: a map pixel exists only where its whole box lies inside the image.
//
// LDS per 512-thread workgroup: 25 KB of tables (GenLds) + 5.25 KB (4:2:0: 2 KB Y + 1 KB chroma + 2.25 KB workspace; 4:4:4: 1 KB Y +
// 2 KB chroma + 2.25 KB) / 6.25 KB (4:2:2) per wave for the tile and the IDCT workspace = 68 / 76 KB two pass -> two workgroups
// (16 waves) per CU; the one-pass step table adds 16 KB -> one.
#include "cu_count.h"
#include "encode_core.h"
#include "coef_tile.h"
#include "lds_copy.h"

namespace uhdr {
namespace {

constexpr int kCoefBlock = 512;
constexpr int kCoefWaves = kCoefBlock / 64;
constexpr int kCoefMaxGrid = 2048;  // the host layer sizes the partials buffer for this many workgroups

struct GenLds {
  float srgb[kSrgbN];
  float hdr[kInvOetfN];
  UnormTables unorm;  // x / 255.0f, x / 1023.0f
};

// the SDR sample at pixel (lx, ly) of the wave's tile, as fetch_pixel<4:2:0 / 4:2:2 / 4:4:4> returns it for the stored bytes
template <int SAMPLING>
__device__ __forceinline__ Color3 fetch_tile_pixel(const uint8_t* yt, const uint8_t* cbt, const uint8_t* crt, uint32_t lx, uint32_t ly) {
  using G = coef_tile::Geom<SAMPLING>;
  constexpr uint32_t VDIV = G::TROWS / G::CROWS, HDIV = 128 / G::CPITCH;  // luma samples per chroma sample, down and across
  const int yy = yt[ly * 128 + lx];
  const int uu = cbt[(ly / VDIV) * G::CPITCH + lx / HDIV];
  const int vv = crt[(ly / VDIV) * G::CPITCH + lx / HDIV];
  Color3 c;
  c.r = (float)yy * (1 / 255.0f);
  c.g = (float)(uu - 128) * (1 / 255.0f);
  c.b = (float)(vv - 128) * (1 / 255.0f);
  return c;
}
// sample_box (pixel_io.h) over the tile: map pixel (lx, ly) of the tile at scale factor s
template <int SAMPLING>
__device__ __forceinline__ Color3 sample_tile_box(const uint8_t* yt, const uint8_t* cbt, const uint8_t* crt, uint32_t s, uint32_t lx, uint32_t ly) {
  if (s == 1) return fetch_tile_pixel<SAMPLING>(yt, cbt, crt, lx, ly);
  Color3 e = {0.0f, 0.0f, 0.0f};
  for (uint32_t dy = 0; dy < s; ++dy)
    for (uint32_t dx = 0; dx < s; ++dx) {
      const Color3 q = fetch_tile_pixel<SAMPLING>(yt, cbt, crt, lx * s + dx, ly * s + dy);
      e.r += q.r;
      e.g += q.g;
      e.b += q.b;
    }
  const float d = (float)(s * s);
  e.r /= d;
  e.g /= d;
  e.b /= d;
  return e;
}

// (tiles in a row, tiles) of a w x h image in tiles of 128 x TROWS pixels
template <int TROWS>
__device__ __forceinline__ uint2 tile_counts(uint32_t w, uint32_t h) {
  static_assert(TROWS == 16 || TROWS == 8, "an MCU row of a 4:2:0 / 4:2:2 or of a 4:4:4 frame");
  if constexpr (TROWS == 16) {
    const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 15) >> 4, ntiles = tiles_x * tiles_y;
    return make_uint2(tiles_x, ntiles);
  } else {
    const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 7) >> 3, ntiles = tiles_x * tiles_y;
    return make_uint2(tiles_x, ntiles);
  }
}

// SAMPLING: 420, 422 or 444.  HDRF: the HDR format (as generate_kernel's).  QUAD (P010 at scale factor 1 with a layout that
// passes quad_layout_ok): one lane per 2 x 2 quad, the HDR side read with fetch_quad_p010 as generate_quad_kernel does.
template <int SAMPLING, int HDRF, bool TWO_PASS, bool QUAD>
__global__ __launch_bounds__(kCoefBlock) void generate_coef_kernel(const GenParams p, const CoefSrc cs, float* partials) {
  static_assert(!QUAD || HDRF == UHDR_IMG_FMT_24bppYCbCrP010, "the quad fetch is P010's");
  using G = coef_tile::Geom<SAMPLING>;
  __shared__ GenLds L;
  __shared__ uint2 s_gain8[TWO_PASS ? 1 : kStepTabMax];  // one pass: clamped gain -> map byte (host_tables.cpp)
  __shared__ int s_ws[kCoefWaves][8 * 8 * 9];
  __shared__ int s_q[3][64];
  __shared__ __attribute__((aligned(8))) uint8_t s_yt[kCoefWaves][G::TROWS * 128];
  __shared__ __attribute__((aligned(8))) uint8_t s_ct[kCoefWaves][2][G::CROWS * G::CPITCH];
  static_assert(sizeof(GenLds) + sizeof s_gain8 + sizeof s_ws + sizeof s_q + sizeof s_yt + sizeof s_ct + 256 <= (TWO_PASS ? 80 : 160) * 1024,
                "two-pass workgroups are sized for two per CU, one-pass workgroups for one");
  const uint32_t tid = threadIdx.x;
  if constexpr (!TWO_PASS) stage_step_tab(s_gain8, p.gain8, tid, kCoefBlock);
  for (uint32_t i = tid; i < kSrgbN; i += kCoefBlock) L.srgb[i] = p.srgb_lut[i];
  if (p.hdr_inv_lut)
    for (uint32_t i = tid; i < (uint32_t)p.hdr_inv_n; i += kCoefBlock) L.hdr[i] = p.hdr_inv_lut[i];
  fill_unorm_tables(L.unorm, tid, kCoefBlock);
  coef_tile::stage_q(s_q, cs.q, tid);
  __syncthreads();

  const bool hdr_lut = p.hdr_inv_lut != nullptr, hdr_lut_4096 = p.hdr_inv_n == kInvOetfN;
  float mn[3] = {UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT, UHDR_RATIO_MIN_INIT}, mx[3] = {UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT, UHDR_RATIO_MAX_INIT};
  // one map pixel from the two samples: generate_kernel's sequence (the SDR intent of API-3 is never RGB)
  auto emit = [&](Color3 s, Color3 h, uint32_t x, uint32_t y) {
    s = yuv_to_rgb(s.r, s.g, s.b, p.sdr_yuv);
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
    gain_of_pixel<TWO_PASS>(sl, hl, p, p.math_tab, x, y, mn, mx, TWO_PASS ? nullptr : s_gain8);
  };

  const uint32_t lane = tid & 63;
  const int wv = (int)__builtin_amdgcn_readfirstlane(tid >> 6);
  int* ws = s_ws[wv];
  uint8_t* const yt = s_yt[wv];
  uint8_t* const cbt = s_ct[wv][0];
  uint8_t* const crt = s_ct[wv][1];
  uint8_t* const tile[3] = {yt, cbt, crt};
  const int rr = (int)lane >> 3, rb = (int)lane & 7;
  const uint32_t w = p.sdr.w, h = p.sdr.h, mw = p.map_w, mh = p.map_h;
  const uint2 tc = tile_counts<G::TROWS>(w, h);
  const uint32_t tiles_x = tc.x, ntiles = tc.y;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kCoefWaves + (tid >> 6));
  const uint32_t nwaves = gridDim.x * kCoefWaves;
  for (uint32_t t = wave; t < ntiles; t += nwaves) {
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    {  // luma, then chroma (Cb, then Cr): v[4][8] at a time, not v[8][8]
      int v[G::NLUMA][8], big[G::NLUMA] = {};
      coef_tile::load_units<SAMPLING, 0, G::NLUMA>(s_q, cs.coef, cs.bw, cs.bh, tx, ty, rr, rb, v, big);
      coef_tile::transform_units<SAMPLING, 0, G::NLUMA>(ws, tile, rr, rb, v, big);
    }
    {
      int v[G::NU - G::NLUMA][8], big[G::NU - G::NLUMA] = {};
      coef_tile::load_units<SAMPLING, G::NLUMA, G::NU>(s_q, cs.coef, cs.bw, cs.bh, tx, ty, rr, rb, v, big);
      coef_tile::transform_units<SAMPLING, G::NLUMA, G::NU>(ws, tile, rr, rb, v, big);
    }
    coef_tile::tile_ready();
    constexpr uint32_t TROWS = G::TROWS;
    if constexpr (QUAD) {  // eight quad rows of 64 quads (4:4:4: four)
      const uint32_t qx = tx * 64 + lane;
#pragma unroll 1
      for (uint32_t qr = 0; qr < TROWS / 2; qr++) {
        const uint32_t qy = ty * (TROWS / 2) + qr;
        if (qx >= w / 2 || qy >= h / 2) continue;
        const QuadYuv hq = fetch_quad_p010(p.hdr, qx, qy, &L.unorm);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
          emit(fetch_tile_pixel<SAMPLING>(yt, cbt, crt, 2 * lane + (k & 1), 2 * qr + (k >> 1)), hq.px[k], 2 * qx + (k & 1), 2 * qy + (k >> 1));
      }
    } else {  // one lane per map pixel, 64 consecutive pixels of a tile row at a time
      const uint32_t s = p.scale, sh = 7u - (s >> 1);  // a tile is 128 >> (s / 2) map pixels wide: 128, 64, 32
      const uint32_t tw = 1u << sh, npx = tw * (TROWS / s);  // and TROWS / s map rows high
#pragma unroll 1
      for (uint32_t i = lane; i < npx; i += 64) {
        const uint32_t ly = i >> sh, lx = i & (tw - 1);
        const uint32_t x = tx * tw + lx, y = ty * (TROWS / s) + ly;
        if (x >= mw || y >= mh) continue;
        emit(sample_tile_box<SAMPLING>(yt, cbt, crt, s, lx, ly), sample_box<HDRF>(p.hdr, s, x, y, &L.unorm), x, y);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next tile overwrites the LDS tile
  }
  if constexpr (TWO_PASS) reduce_block_minmax<kCoefBlock>(mn, mx, partials);
}

// the tiles of the launch: 128 x 16 pixels, or the eight-row tiles of a 4:4:4 frame
uint32_t coef_tiles(const GenParams& p, int sampling) {
  if (sampling == 444) return coef_tile::tiles_of(p.sdr.w, p.sdr.h, 444);
  const uint32_t tiles = ((p.sdr.w + 127) / 128) * ((p.sdr.h + 15) / 16);
  return tiles;
}

int coef_grid(const GenParams& p, int sampling, bool two_pass) {
  const int cus = device_cu_count();
  const uint32_t tiles = coef_tiles(p, sampling);
  const uint32_t resident = (uint32_t)cus * (two_pass ? 2u : 1u);  // workgroups per CU: the LDS budget at the head of this file
  uint32_t g = (tiles + kCoefWaves - 1) / kCoefWaves;
  if (g > resident) g = resident;
  if (g > (uint32_t)kCoefMaxGrid) g = kCoefMaxGrid;
  if (g < 1) g = 1;
  return (int)g;
}

bool coef_quad_path(const GenParams& p) { return p.scale == 1 && p.hdr.fmt == UHDR_IMG_FMT_24bppYCbCrP010 && quad_layout_ok(p.hdr); }

template <int SAMPLING, int HDRF, bool QUAD>
void launch_coef_p(const GenParams& p, const CoefSrc& cs, bool two_pass, int grid, float* partials, hipStream_t s) {
  if (two_pass) hipLaunchKernelGGL((generate_coef_kernel<SAMPLING, HDRF, true, QUAD>), dim3(grid), dim3(kCoefBlock), 0, s, p, cs, partials);
  else hipLaunchKernelGGL((generate_coef_kernel<SAMPLING, HDRF, false, QUAD>), dim3(grid), dim3(kCoefBlock), 0, s, p, cs, partials);
}
template <int SAMPLING>
void launch_coef_h(const GenParams& p, const CoefSrc& cs, bool two_pass, int grid, float* partials, hipStream_t s) {
  if (coef_quad_path(p)) return launch_coef_p<SAMPLING, UHDR_IMG_FMT_24bppYCbCrP010, true>(p, cs, two_pass, grid, partials, s);
  switch (p.hdr.fmt) {
    case UHDR_IMG_FMT_24bppYCbCrP010: return launch_coef_p<SAMPLING, UHDR_IMG_FMT_24bppYCbCrP010, false>(p, cs, two_pass, grid, partials, s);
    case UHDR_IMG_FMT_32bppRGBA1010102: return launch_coef_p<SAMPLING, UHDR_IMG_FMT_32bppRGBA1010102, false>(p, cs, two_pass, grid, partials, s);
    default: return launch_coef_p<SAMPLING, -1, false>(p, cs, two_pass, grid, partials, s);
  }
}

}  // namespace

int gen_coef_partials_count(const GenParams& p, int sampling) { return coef_grid(p, sampling, true); }

// p.sdr carries the geometry of the image the coefficients decode to (its planes are never dereferenced); sampling is 420, 422 or 444,
// p.scale is 1, 2 or 4 and w, h are even (the host layer declines everything else).  Two pass: the ratio plane p.gain_log2 and
// gen_coef_partials_count(p, sampling) x 6 ratio extrema at p.minmax + 6, the contract of launch_generate_gainmap.
hipError_t launch_generate_gainmap_coef(const GenParams& p, const CoefSrc& cs, int sampling, bool two_pass, hipStream_t s) {
  if ((p.scale != 1 && p.scale != 2 && p.scale != 4) || (sampling != 420 && sampling != 422 && sampling != 444) || p.sdr.w % 2 || p.sdr.h % 2)
    return hipErrorInvalidValue;
  float* partials = two_pass ? p.minmax + 6 : nullptr;
  const int grid = coef_grid(p, sampling, two_pass);
  if (sampling == 420) launch_coef_h<420>(p, cs, two_pass, grid, partials, s);
  else if (sampling == 422) launch_coef_h<422>(p, cs, two_pass, grid, partials, s);
  else launch_coef_h<444>(p, cs, two_pass, grid, partials, s);
  return hipGetLastError();
}

}  // namespace uhdr
