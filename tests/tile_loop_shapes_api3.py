"""The shape at which generate_coef_kernel's tile loop takes a second trip: the API-3 sibling of tests/tile_loop_shapes.py, whose search
rules (LOW, HIGH, TARGET, MAX_DIM, satisfies, NoSuchShape) it keeps.  launch_generate_gainmap_coef caps its grid at two 512-thread
workgroups per compute unit for the two-pass preset (one for the one-pass preset) and at 2048 workgroups, and every WAVE walks
`for (t = wave; t < ntiles; t += nwaves)` over 128 x 16 pixel tiles; the launcher's grid arithmetic is restated here and MIRRORED lists
the source lines, which tests/test_tile_loop_shapes_api3.py checks still read the same.  No imports beyond the standard library and
that module."""
import tile_loop_shapes as T

KERNEL = "generate_coef"
COEF_BLOCK = 512  # constexpr int kCoefBlock = 512;
MAX_GRID = 2048   # constexpr int kCoefMaxGrid = 2048;

# (file under libultrahdr_amd/csrc, text): what coef_walk restates
MIRRORED = [
    ("generate_coef.hip", "constexpr int kCoefBlock = 512;"),
    ("generate_coef.hip", "constexpr int kCoefWaves = kCoefBlock / 64;"),
    ("generate_coef.hip", "constexpr int kCoefMaxGrid = 2048;"),
    ("generate_coef.hip", "const uint32_t tiles = ((p.sdr.w + 127) / 128) * ((p.sdr.h + 15) / 16);"),
    ("generate_coef.hip", "const uint32_t resident = (uint32_t)cus * (two_pass ? 2u : 1u);"),
    ("generate_coef.hip", "uint32_t g = (tiles + kCoefWaves - 1) / kCoefWaves;"),
    ("generate_coef.hip", "if (g > resident) g = resident;"),
    ("generate_coef.hip", "if (g > (uint32_t)kCoefMaxGrid) g = kCoefMaxGrid;"),
    ("generate_coef.hip", "const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 15) >> 4, ntiles = tiles_x * tiles_y;"),
    ("generate_coef.hip", "const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kCoefWaves + (tid >> 6));"),
    ("generate_coef.hip", "const uint32_t nwaves = gridDim.x * kCoefWaves;"),
    ("generate_coef.hip", "for (uint32_t t = wave; t < ntiles; t += nwaves) {"),
]


def coef_walk(cus, w, h, two_pass=True):
    """(tiles_x, items, walkers) of generate_coef_kernel on the coefficients of a w x h image; a walker is a wave."""
    tiles_x = (w + 127) >> 7                  # const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 15) >> 4, ntiles = tiles_x * tiles_y;
    tiles = tiles_x * ((h + 15) >> 4)         # ... and coef_grid: const uint32_t tiles = ((p.sdr.w + 127) / 128) * ((p.sdr.h + 15) / 16);
    waves = COEF_BLOCK // 64                  # constexpr int kCoefWaves = kCoefBlock / 64;
    resident = cus * (2 if two_pass else 1)   # const uint32_t resident = (uint32_t)cus * (two_pass ? 2u : 1u);
    g = (tiles + waves - 1) // waves          # uint32_t g = (tiles + kCoefWaves - 1) / kCoefWaves;
    if g > resident:                          # if (g > resident) g = resident;
        g = resident
    if g > MAX_GRID:                          # if (g > (uint32_t)kCoefMaxGrid) g = kCoefMaxGrid;
        g = MAX_GRID
    if g < 1:                                 # if (g < 1) g = 1;
        g = 1
    return tiles_x, tiles, g * waves          # const uint32_t nwaves = gridDim.x * kCoefWaves;


def coef_loop(cus, two_pass=True):
    """The smallest-tiles_x shape (even dimensions; a last tile column with two live pixels, a last tile row with eight live rows)
    whose tile count lies strictly between LOW x and HIGH x the waves launched on `cus` compute units, as a
    tile_loop_shapes.TileLoop; raises NoSuchShape."""
    if cus < 1:
        raise T.NoSuchShape(f"{cus} compute units")
    rows_allowed = range(2, T.MAX_DIM // 16 + 1)  # tile rows
    for tx in range(3, T.MAX_DIM):
        w = (tx - 1) * 128 + 2
        if w > T.MAX_DIM:
            break
        if tx & (tx - 1) == 0:
            continue
        mk = lambda r: T.TileLoop(KERNEL, w, 16 * r - 8, *coef_walk(cus, w, 16 * r - 8, two_pass))
        cap = mk(rows_allowed[-1]).walkers
        want = -(-int(T.TARGET * cap * 1000) // (1000 * tx))
        fits = [r for r in rows_allowed if T.satisfies(mk(r))]
        if fits:
            return mk(min(fits, key=lambda r: (abs(r - want), r)))
    raise T.NoSuchShape(f"{KERNEL}: no shape within {T.MAX_DIM} x {T.MAX_DIM} puts the tile count between {T.LOW} and {T.HIGH} times the waves of {cus} compute units")
