"""Shapes at which the persistent tile loops of the newest kernels take a second trip: a plain helper module for
tests/test_tile_loop_shapes.py (CPU) and tests/test_gpu_tile_loops.py (device), no imports beyond the standard library.

The launchers cap their grids at what is resident on the device, and every wave or workgroup (a "walker") then walks
`for (t = first; t < items; t += walkers)`.  Whether an image makes a walker come round again depends on the number of
compute units, so the grid arithmetic of each launcher is restated here, line by line, and tile_loop() searches a shape with

  * both dimensions at most MAX_DIM, the reference's own limit,
  * an item count strictly between LOW x and HIGH x the number of walkers: some walkers take two trips, some take one,
  * tiles_x (groups_x) at least 3 and not a power of two (every one of these kernels divides the item index by it),
  * a ragged last tile in each row.

NARROW_KERNELS are the per-pixel routes of the oldest launchers (convertYuv, convert_raw_input_to_ycbcr, libjpeg's colour conversions,
toneMap), whose loops are `for (t = blockIdx.x; t < tiles; t += gridDim.x)` under grid_for's cap of 4096 workgroups, resident_grid(..., 8) and
tone_grid(..., 4): the same search, with widths that the vector route of the same operator takes as well.

It raises NoSuchShape where there is none: a device test that cannot reach the second trip has to fail, not pass quietly.
MIRRORED lists the source lines restated here; the CPU test checks that they still read the same."""
from collections import namedtuple

MAX_DIM = 8192
LOW, HIGH = 1.25, 2.5
TARGET = 1.3  # the ratio aimed at: the smallest image that is safely past LOW

KERNELS = ("p010_two_pass", "p010_one_pass", "rgba", "resize", "effects")
# the per-pixel ("narrow") routes of the oldest launchers, which a layout off the vector alignment selects (tests/route_lattice.py): their
# widths are whole vector tiles (8 pixels, 4 for the colour kernels) so that the same samples also run on the vector route
NARROW_KERNELS = ("yuv420", "yuv444", "rgb420", "rgb444", "jpeg_colour", "tone_pixel", "tone_p010")
AT_CAP = ("yuv420", "yuv444", "rgb420", "rgb444")  # kernels whose shape also has to reach grid_for's cap of 4096 workgroups

# (file under libultrahdr_amd/csrc, text): what the functions below restate
MIRRORED = [
    ("encode_fused.hip", "constexpr int quad_block(bool two_pass) { return two_pass ? 512 : 768; }"),
    ("encode_fused.hip", "const uint32_t tiles_x = (qw + 63) / 64, tiles = tiles_x * qh;"),
    ("encode_fused.hip", "const uint32_t nwaves = gridDim.x * (kQuadBlock / 64);"),
    ("encode_fused.hip", "const int resident = cus * per_cu;"),
    ("encode_fused.hip", "uint32_t g = tiles < (uint32_t)resident ? tiles : (uint32_t)resident;"),
    ("encode_fused.hip", "if (g > 2048) g = 2048;"),
    ("encode_fused.hip", "const uint32_t wave_tiles = ((p.tm.hdr.w / 2 + 63) / 64) * (p.tm.hdr.h / 2);"),
    ("encode_fused.hip", "const int grid = fused_grid((wave_tiles + wg_waves - 1) / wg_waves, two_pass ? 3 : 2);"),
    ("encode_api1_fused.hip", "constexpr int kBlock = 256;  // 4 waves"),
    ("encode_api1_fused.hip", "const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;"),
    ("encode_api1_fused.hip", "const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);"),
    ("encode_api1_fused.hip", "int grid = (total_wave_items + kBlock / 64 - 1) / (kBlock / 64);"),
    ("encode_api1_fused.hip", "if (grid > cus * per_cu) grid = cus * per_cu;"),
    ("encode_api1_fused.hip", "p.bw = (int)(rgba.w / 8); p.bh = (int)(rgba.h / 8);"),
    ("encode_api1_fused.hip", "const int grid = resident_grid(((p.bw + 7) / 8) * p.bh, 7);"),
    ("resize_image.hip", "constexpr uint32_t kTileW = 256u * kRun;"),
    ("resize_image.hip", "const uint64_t tiles = (uint64_t)((p.dst_w + kTileW - 1) / kTileW) * p.rows;"),
    ("resize_image.hip", "const int grid = (int)(tiles < 16384u ? tiles : 16384u);"),
    ("effects.hip", "const uint32_t tiles = ((p.dst_w + 255u) / 256u) * p.dst_h;"),
    ("effects.hip", "const int grid = (int)(tiles < 16384u ? tiles : 16384u);"),
    ("convert.hip", "constexpr int kBlock = 256;"),
    ("convert.hip", "const uint32_t tiles_x = (qw + kBlock - 1) / kBlock, tiles = tiles_x * qh;"),
    ("convert.hip", "const uint32_t tiles_x = (w + kBlock - 1) / kBlock, tiles = tiles_x * h;"),
    ("convert.hip", "for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {"),
    ("convert.hip", "size_t g = (total + kBlock - 1) / kBlock;"),
    ("convert.hip", "if (g > 4096) g = 4096;"),
    ("convert.hip", "hipLaunchKernelGGL(transform_yuv420_kernel, dim3(grid_for((size_t)(p.img.w / 2) * (p.img.h / 2))),"),
    ("convert.hip", "hipLaunchKernelGGL(transform_yuv444_kernel, dim3(grid_for((size_t)p.img.w * p.img.h)), dim3(kBlock), 0, s, p);"),
    ("convert.hip", "const int g = grid_for((size_t)(p.src.w / 2) * (p.src.h / 2));"),
    ("convert.hip", "const int g = grid_for((size_t)p.src.w * p.src.h);"),
    ("jpeg_decode.hip", "const uint32_t per_row = VEC ? p.w / 4 : p.w;"),
    ("jpeg_decode.hip", "const uint32_t tiles_x = (per_row + kBlock - 1) / kBlock, tiles = tiles_x * p.h;"),
    ("jpeg_decode.hip", "for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {"),
    ("jpeg_decode.hip", "const int grid = resident_grid(((per_row + kBlock - 1) / kBlock) * p.h, 8);"),
    ("upsample_core.h", "const uint32_t r = (uint32_t)(device_cu_count() * per_cu);"),
    ("upsample_core.h", "return (int)(tiles < r ? (tiles ? tiles : 1u) : r);"),
    ("tonemap.hip", "constexpr int kQuadBlock = 512;"),
    ("tonemap.hip", "const uint32_t tiles_x = (qw + 63) / 64, tiles = tiles_x * qh;"),
    ("tonemap.hip", "const uint32_t nwaves = gridDim.x * (kQuadBlock / 64);"),
    ("tonemap.hip", "for (uint32_t t = wave; t < tiles; t += nwaves) {"),
    ("tonemap.hip", "const uint32_t tiles_x = (w + kBlock - 1) / kBlock, tiles = tiles_x * h;"),
    ("tonemap.hip", "for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {"),
    ("tonemap.hip", "const int resident = cus * per_cu;"),
    ("tonemap.hip", "const uint32_t g = tiles < (uint32_t)resident ? tiles : (uint32_t)resident;"),
    ("tonemap.hip", "const int grid = tone_grid((wave_tiles + kQuadBlock / 64 - 1) / (kQuadBlock / 64), 4);"),
    ("tonemap.hip", "const int grid = tone_grid(((p.hdr.w + kBlock - 1) / kBlock) * p.hdr.h, 4);"),
]

TileLoop = namedtuple("TileLoop", "kernel w h tiles_x items walkers")


class NoSuchShape(ValueError):
    pass


def _ceil_div(a, b):
    return -(-a // b)


# ---- the launchers ------------------------------------------------------------------------------------------------------------------
def fused_grid(cus, tiles, per_cu):
    """encode_fused.hip: fused_grid."""
    resident = cus * per_cu                      # const int resident = cus * per_cu;
    g = tiles if tiles < resident else resident  # uint32_t g = tiles < (uint32_t)resident ? tiles : (uint32_t)resident;
    if g > 2048:                                 # if (g > 2048) g = 2048;
        g = 2048
    return 1 if g < 1 else g                     # return (int)(g < 1 ? 1 : g);


def resident_grid(cus, total_wave_items, per_cu, block=256):
    """encode_api1_fused.hip: resident_grid (kBlock = 256: four waves)."""
    grid = _ceil_div(total_wave_items, block // 64)  # int grid = (total_wave_items + kBlock / 64 - 1) / (kBlock / 64);
    if grid > cus * per_cu:                          # if (grid > cus * per_cu) grid = cus * per_cu;
        grid = cus * per_cu
    return 1 if grid < 1 else grid                   # return grid < 1 ? 1 : grid;


def p010_walk(cus, w, h, two_pass):
    """(tiles_x, items, walkers) of encode_api0_p010_fused_kernel on a w x h P010 intent; a walker is a wave."""
    tiles_x = (w // 2 + 63) // 64                    # const uint32_t tiles_x = (qw + 63) / 64, ...
    wave_tiles = tiles_x * (h // 2)                  # launch_encode_api0_p010_fused: wave_tiles
    wg_waves = (512 if two_pass else 768) // 64      # quad_block(two_pass) / 64
    grid = fused_grid(cus, _ceil_div(wave_tiles, wg_waves), 3 if two_pass else 2)
    return tiles_x, wave_tiles, grid * wg_waves      # nwaves = gridDim.x * (kQuadBlock / 64)


def rgba_walk(cus, w, h):
    """(groups_x, items, walkers) of base_blocks_rgba_kernel on a w x h RGBA8888 intent; a walker is a wave."""
    bw, bh = w // 8, h // 8                          # p.bw = (int)(rgba.w / 8); p.bh = (int)(rgba.h / 8);
    groups_x = (bw + 7) >> 3                         # const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;
    total = groups_x * bh
    grid = resident_grid(cus, total, 7)              # resident_grid(((p.bw + 7) / 8) * p.bh, 7)
    return groups_x, total, grid * (256 // 64)       # nwaves = gridDim.x * (kBlock / 64)


def resize_walk(dst_w, rows):
    """(tiles_x, items, walkers) of resize_image_kernel for `rows` destination rows of dst_w pixels; a walker is a workgroup."""
    tiles_x = (dst_w + 1024 - 1) // 1024             # kTileW = 256u * kRun, kRun = 4
    tiles = tiles_x * rows
    return tiles_x, tiles, (tiles if tiles < 16384 else 16384)


def effect_walk(dst_w, dst_h):
    """(tiles_x, items, walkers) of effect_remap_kernel for one destination plane of dst_w x dst_h elements; a walker is a workgroup."""
    tiles_x = (dst_w + 255) // 256
    tiles = tiles_x * dst_h
    return tiles_x, tiles, (tiles if tiles < 16384 else 16384)


def grid_for(total):
    """convert.hip: grid_for (one 256-thread workgroup per 256 quads / pixels, at most 4096)."""
    g = _ceil_div(total, 256)                        # size_t g = (total + kBlock - 1) / kBlock;
    if g > 4096:                                     # if (g > 4096) g = 4096;
        g = 4096
    return 1 if g < 1 else g                         # return (int)(g < 1 ? 1 : g);


def convert420_walk(w, h):
    """(tiles_x, items, walkers) of transform_yuv420_kernel and rgb_to_ycbcr420_kernel on a w x h image; a walker is a workgroup.  The grid
    counts quads, the loop counts tiles of one quad row: a ragged row makes more tiles than workgroups well below the cap."""
    qw, qh = w // 2, h // 2
    tiles_x = _ceil_div(qw, 256)                     # const uint32_t tiles_x = (qw + kBlock - 1) / kBlock, tiles = tiles_x * qh;
    return tiles_x, tiles_x * qh, grid_for(qw * qh)  # grid_for((size_t)(p.img.w / 2) * (p.img.h / 2))


def convert444_walk(w, h):
    """(tiles_x, items, walkers) of transform_yuv444_kernel and rgb_to_ycbcr444_kernel on a w x h image; a walker is a workgroup."""
    tiles_x = _ceil_div(w, 256)                      # const uint32_t tiles_x = (w + kBlock - 1) / kBlock, tiles = tiles_x * h;
    return tiles_x, tiles_x * h, grid_for(w * h)     # grid_for((size_t)p.img.w * p.img.h)


def jpeg_colour_walk(cus, w, h):
    """(tiles_x, items, walkers) of jpeg_rgb_to_ycc_kernel<BPP, false> and jpeg_ycc_to_rgb_kernel<BPP, false>; a walker is a workgroup."""
    tiles_x = _ceil_div(w, 256)                      # per_row = p.w; tiles_x = (per_row + kBlock - 1) / kBlock
    tiles = tiles_x * h
    r = cus * 8                                      # resident_grid(..., 8): const uint32_t r = (uint32_t)(device_cu_count() * per_cu);
    return tiles_x, tiles, (tiles if tiles < r else r) or 1


def tone_grid(cus, tiles, per_cu):
    """tonemap.hip: tone_grid."""
    resident = cus * per_cu                          # const int resident = cus * per_cu;
    g = tiles if tiles < resident else resident      # const uint32_t g = tiles < (uint32_t)resident ? tiles : (uint32_t)resident;
    return 1 if g < 1 else g                         # return (int)(g < 1 ? 1 : g);


def tone_pixel_walk(cus, w, h):
    """(tiles_x, items, walkers) of tonemap_pixel_kernel; a walker is a workgroup."""
    tiles_x = _ceil_div(w, 256)
    tiles = tiles_x * h
    return tiles_x, tiles, tone_grid(cus, tiles, 4)  # tone_grid(((p.hdr.w + kBlock - 1) / kBlock) * p.hdr.h, 4)


def tone_p010_walk(cus, w, h):
    """(tiles_x, items, walkers) of tonemap_p010_kernel; a walker is a wave (kQuadBlock = 512: eight per workgroup)."""
    qw, qh = w // 2, h // 2
    tiles_x = (qw + 63) // 64                        # const uint32_t tiles_x = (qw + 63) / 64, tiles = tiles_x * qh;
    wave_tiles = tiles_x * qh
    grid = tone_grid(cus, _ceil_div(wave_tiles, 8), 4)  # tone_grid((wave_tiles + kQuadBlock / 64 - 1) / (kQuadBlock / 64), 4)
    return tiles_x, wave_tiles, grid * 8             # nwaves = gridDim.x * (kQuadBlock / 64)


# ---- the search -----------------------------------------------------------------------------------------------------------------------
def _is_pow2(n):
    return n & (n - 1) == 0


def _geometry(kernel, cus):
    """(walk(w, h), width of tiles_x tiles with a ragged last one, height of `rows` item rows, the row counts allowed)."""
    if kernel in ("p010_two_pass", "p010_one_pass"):  # 64 quads per tile, one item row per quad row
        two_pass = kernel == "p010_two_pass"
        return (lambda w, h: p010_walk(cus, w, h, two_pass)), (lambda tx: 2 * ((tx - 1) * 64 + 1)), (lambda r: 2 * r), range(1, MAX_DIM // 2 + 1)
    if kernel == "rgba":  # eight 8 x 8 blocks per group, one item row per block row
        return (lambda w, h: rgba_walk(cus, w, h)), (lambda tx: 8 * ((tx - 1) * 8 + 1)), (lambda r: 8 * r), range(1, MAX_DIM // 8 + 1)
    if kernel == "resize":  # 1024 pixels per tile; + 2: the last run of four pixels is ragged as well
        return resize_walk, (lambda tx: (tx - 1) * 1024 + 2), (lambda r: r), range(1, MAX_DIM + 1)
    if kernel == "effects":  # 256 elements per tile; even rows, so that a 4:2:0 image has whole chroma planes
        return effect_walk, (lambda tx: (tx - 1) * 256 + 8), (lambda r: r), range(2, MAX_DIM + 1, 2)
    # the narrow routes: a ragged last tile of whole vector tiles (8 pixels; 4 for the colour kernels)
    if kernel in ("yuv420", "rgb420"):  # 256 quads per tile, one item row per quad row
        return convert420_walk, (lambda tx: 2 * ((tx - 1) * 256 + 4)), (lambda r: 2 * r), range(1, MAX_DIM // 2 + 1)
    if kernel in ("yuv444", "rgb444"):  # 256 pixels per tile
        return convert444_walk, (lambda tx: (tx - 1) * 256 + 8), (lambda r: r), range(1, MAX_DIM + 1)
    if kernel == "jpeg_colour":
        return (lambda w, h: jpeg_colour_walk(cus, w, h)), (lambda tx: (tx - 1) * 256 + 4), (lambda r: r), range(1, MAX_DIM + 1)
    if kernel == "tone_pixel":
        return (lambda w, h: tone_pixel_walk(cus, w, h)), (lambda tx: (tx - 1) * 256 + 4), (lambda r: r), range(1, MAX_DIM + 1)
    if kernel == "tone_p010":  # 64 quads per tile, one item row per quad row
        return (lambda w, h: tone_p010_walk(cus, w, h)), (lambda tx: 2 * ((tx - 1) * 64 + 1)), (lambda r: 2 * r), range(1, MAX_DIM // 2 + 1)
    raise ValueError(f"unknown kernel {kernel!r}")


def satisfies(loop):
    """The constraints of the module docstring on a TileLoop (the width's raggedness is the caller's: it depends on the tile)."""
    return (loop.w <= MAX_DIM and loop.h <= MAX_DIM and LOW * loop.walkers < loop.items < HIGH * loop.walkers and
            loop.tiles_x >= 3 and not _is_pow2(loop.tiles_x))


def tile_loop(kernel, cus):
    """The smallest-tiles_x shape for `kernel` on a device with `cus` compute units, as a TileLoop; raises NoSuchShape."""
    if cus < 1:
        raise NoSuchShape(f"{cus} compute units")
    walk, width_of, height_of, rows_allowed = _geometry(kernel, cus)
    for tx in range(3, MAX_DIM):
        w = width_of(tx)
        if w > MAX_DIM:
            break
        if _is_pow2(tx):
            continue
        # walkers never exceed what the tallest image gets; aim at TARGET x that, then take the nearest row count that fits
        cap = walk(w, height_of(rows_allowed[-1]))[2]
        want = _ceil_div(int(TARGET * cap * 1000), 1000 * tx)
        fits = [r for r in rows_allowed if satisfies(TileLoop(kernel, w, height_of(r), *walk(w, height_of(r))))]
        if kernel in AT_CAP:  # (grid_for counts samples, the loop tiles: a ragged row alone makes a second trip -- take the grid at its cap)
            fits = [r for r in fits if walk(w, height_of(r))[2] == cap]
        if fits:
            r = min(fits, key=lambda r: (abs(r - want), r))
            return TileLoop(kernel, w, height_of(r), *walk(w, height_of(r)))
    raise NoSuchShape(f"{kernel}: no shape within {MAX_DIM} x {MAX_DIM} puts the item count between {LOW} and {HIGH} times the walkers of {cus} compute units")


def describe(loop):
    second = loop.items - loop.walkers
    return (f"{loop.kernel}: {loop.w}x{loop.h}, tiles_x {loop.tiles_x}, {loop.items} items over {loop.walkers} walkers "
            f"({second} walkers take a second trip)")
