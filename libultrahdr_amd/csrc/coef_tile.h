// The coefficient-tile stage of the kernels that take an image as JPEG coefficient blocks (apply_quad_body<..., SRC = 1> in
// apply_gainmap.hip, generate_coef_kernel in generate_coef.hip): a wave dequantises and inverse-transforms the eight-block
// units of a 128-pixel-wide tile (idct_core.h) into its private LDS tiles Y, Cb, Cr, then reads the samples back.  The layout of
// a tile -- which blocks a unit takes and where its samples land -- is written down once, in Geom::unit, and checked at compile
// time.  The stage is a pair of unit RANGES, not one call: a kernel decides how many units it keeps in registers and what it
// issues between the loads and the transforms.
#pragma once
#include "idct_core.h"

namespace uhdr {
namespace coef_tile {

// eight samples, each below 256 -> their eight bytes, sample 0 lowest
__device__ __forceinline__ uint2 pack8(const uint32_t s[8]) {
  return make_uint2(s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24), s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24));
}

// pixel rows of a tile: an MCU row (a 4:4:4 MCU row is eight rows high)
constexpr int tile_rows(int sampling) { return sampling == 444 ? 8 : 16; }
// host: the 128-pixel-wide tiles of a w x h image
inline uint32_t tiles_of(uint32_t w, uint32_t h, int sampling) {
  const uint32_t rows = (uint32_t)tile_rows(sampling);
  return ((w + 127) / 128) * ((h + rows - 1) / rows);
}

// One eight-block unit: eight horizontally adjacent blocks of component comp, block row vblocks * ty + dy, block columns
// tx * xblocks + xoff + (0..7); its 8 rows x 64 bytes of samples go to LDS tile comp at row dy * 8, byte xoff * 8, rows pitch
// bytes apart.
struct Unit {
  int comp, vblocks, dy, xblocks, xoff, pitch;
};

template <int SAMPLING>
struct Geom {
  static_assert(SAMPLING == 420 || SAMPLING == 422 || SAMPLING == 444, "4:2:0, 4:2:2 or 4:4:4");
  static constexpr int TROWS = tile_rows(SAMPLING);            // rows of the Y tile (pitch 128)
  static constexpr int CROWS = SAMPLING == 420 ? TROWS / 2 : TROWS;  // rows of the Cb and the Cr tile
  static constexpr int CPITCH = SAMPLING == 444 ? 128 : 64;    // bytes of their rows
  static constexpr int NLUMA = (TROWS / 8) * 2;                // units: Y block rows x two halves of sixteen blocks,
  static constexpr int NCHROMA = (CROWS / 8) * (CPITCH / 64);  // then Cb's and Cr's in the same order
  static constexpr int NU = NLUMA + 2 * NCHROMA;

  static constexpr Unit unit(int u) {
    const int comp = u < NLUMA ? 0 : 1 + (u - NLUMA) / NCHROMA;
    const int j = u < NLUMA ? u : (u - NLUMA) % NCHROMA;  // the unit of its component, block row outer / half inner
    const int rows = comp ? CROWS : TROWS, pitch = comp ? CPITCH : 128, halves = pitch / 64;
    return {comp, rows / 8, j / halves, pitch / 8, (j % halves) * 8, pitch};
  }
  // every 8-row x 64-byte cell of the three tiles is some unit's destination exactly once, and no unit leaves its tile
  static constexpr bool covers_tiles_once() {
    int hits[3][4] = {};  // [tile][cell]: at most 2 x 2 cells
    for (int u = 0; u < NU; u++) {
      const Unit g = unit(u);
      const int rows = g.comp ? CROWS : TROWS;
      if (g.comp < 0 || g.comp > 2 || g.pitch != (g.comp ? CPITCH : 128)) return false;
      if (g.dy < 0 || g.dy * 8 + 8 > rows || g.dy >= g.vblocks) return false;
      if (g.xoff < 0 || g.xoff % 8 || g.xoff * 8 + 64 > g.pitch || g.xoff + 8 > g.xblocks) return false;
      hits[g.comp][g.dy * 2 + g.xoff / 8]++;
    }
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 2; r++)
        for (int x = 0; x < 2; x++)
          if (hits[c][r * 2 + x] != (r * 8 < (c ? CROWS : TROWS) && x * 64 < (c ? CPITCH : 128) ? 1 : 0)) return false;
    return true;
  }
  static_assert(covers_tiles_once(), "the units do not tile Y, Cb and Cr");
};
static_assert(Geom<420>::TROWS == 16 && Geom<420>::CROWS == 8 && Geom<420>::CPITCH == 64 && Geom<420>::NU == 6 && Geom<420>::NLUMA == 4, "4:2:0");
static_assert(Geom<422>::TROWS == 16 && Geom<422>::CROWS == 16 && Geom<422>::CPITCH == 64 && Geom<422>::NU == 8 && Geom<422>::NLUMA == 4, "4:2:2");
static_assert(Geom<444>::TROWS == 8 && Geom<444>::CROWS == 8 && Geom<444>::CPITCH == 128 && Geom<444>::NU == 6 && Geom<444>::NLUMA == 2, "4:4:4");

// the three quantiser tables into the workgroup's LDS copy (the caller's barrier follows)
__device__ __forceinline__ void stage_q(int (*s_q)[64], const int (*src)[64], uint32_t tid) {
  if (tid < 192) s_q[tid >> 6][tid & 63] = src[tid >> 6][tid & 63];
}

// Units [U0, U1) of tile (tx, ty): lane (row rr, block rb) requests and dequantises its coefficient row of each into v[u - U0]
// (idct::load_dequant_row; zeros beyond the component's block grid).  A component's divisor row is read from s_q when its
// first unit comes up.
template <int SAMPLING, int U0, int U1>
__device__ __forceinline__ void load_units(const int (*s_q)[64], const int16_t* const coef[3], const int bw[3], const int bh[3], uint32_t tx,
                                           uint32_t ty, int rr, int rb, int (*v)[8], int* big) {
  using G = Geom<SAMPLING>;
  static_assert(0 <= U0 && U0 < U1 && U1 <= G::NU, "a range of the tile's units");
  int q[8];
#pragma unroll
  for (int u = U0; u < U1; u++) {
    const Unit g = G::unit(u);
    if (u == U0 || g.comp != G::unit(u - 1).comp) {
#pragma unroll
      for (int c = 0; c < 8; c++) q[c] = s_q[g.comp][rr * 8 + c];
    }
    const int by = (int)(g.vblocks * ty) + g.dy;
    idct::load_dequant_row(coef[g.comp], bw[g.comp], by, (int)(tx * g.xblocks) + g.xoff + rb, rr, q, v[u - U0], big[u - U0], by < bh[g.comp]);
  }
}

// The same units: inverse transform through the wave's workspace ws, then the lane's eight samples into tile[comp]
template <int SAMPLING, int U0, int U1>
__device__ __forceinline__ void transform_units(int* ws, uint8_t* const tile[3], int rr, int rb, const int (*v)[8], const int* big) {
  using G = Geom<SAMPLING>;
  static_assert(0 <= U0 && U0 < U1 && U1 <= G::NU, "a range of the tile's units");
#pragma unroll
  for (int u = U0; u < U1; u++) {
    const Unit g = G::unit(u);
    uint32_t s[8];
    idct::idct_wave(ws, v[u - U0], big[u - U0], rr, rb, s);
    *(uint2*)(tile[g.comp] + (g.dy * 8 + rr) * g.pitch + (g.xoff + rb) * 8) = pack8(s);
  }
}

// after the last transform_units of a tile: the wave's stores have landed, the tile may be read
__device__ __forceinline__ void tile_ready() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
}

}  // namespace coef_tile
}  // namespace uhdr
