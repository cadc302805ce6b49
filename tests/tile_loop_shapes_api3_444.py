"""The shape at which generate_coef_kernel's tile loop takes a second trip on a 4:4:4 SDR intent: the sibling of
tests/tile_loop_shapes_api3.py for the eight-row tile, with the search rules of tests/tile_loop_shapes.py (LOW, HIGH, TARGET, MAX_DIM,
satisfies, NoSuchShape).  A 4:4:4 MCU row is eight pixel rows high, so a wave's tile is 128 x 8 pixels; the grid caps (two 512-thread
workgroups per compute unit two pass, one one pass, 2048 workgroups) and the walk `for (t = wave; t < ntiles; t += nwaves)` are those
of the other samplings.  The arithmetic is restated here and MIRRORED lists the source lines, which
tests/test_tile_loop_shapes_api3_444.py checks still read the same.  No imports beyond the standard library and those two modules."""
import tile_loop_shapes as T
import tile_loop_shapes_api3 as G

KERNEL = "generate_coef444"
TILE_ROWS = 8  # constexpr int tile_rows(int sampling) { return sampling == 444 ? 8 : 16; }

# (file under libultrahdr_amd/csrc, text): what coef_walk restates beyond tile_loop_shapes_api3.MIRRORED
MIRRORED = G.MIRRORED + [
    ("coef_tile.h", "constexpr int tile_rows(int sampling) { return sampling == 444 ? 8 : 16; }"),
    ("coef_tile.h", "const uint32_t rows = (uint32_t)tile_rows(sampling);"),
    ("coef_tile.h", "return ((w + 127) / 128) * ((h + rows - 1) / rows);"),
    ("generate_coef.hip", "if (sampling == 444) return coef_tile::tiles_of(p.sdr.w, p.sdr.h, 444);"),
    ("generate_coef.hip", "const uint32_t tiles = coef_tiles(p, sampling);"),
    ("generate_coef.hip", "const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 7) >> 3, ntiles = tiles_x * tiles_y;"),
    ("generate_coef.hip", "const uint2 tc = tile_counts<G::TROWS>(w, h);"),
    ("generate_coef.hip", "const uint32_t tiles_x = tc.x, ntiles = tc.y;"),
]


def coef_walk(cus, w, h, two_pass=True):
    """(tiles_x, items, walkers) of generate_coef_kernel on the coefficients of a w x h 4:4:4 image; a walker is a wave."""
    tiles_x = (w + 127) >> 7                          # const uint32_t tiles_x = (w + 127) >> 7, tiles_y = (h + 7) >> 3, ntiles = tiles_x * tiles_y;
    tiles = tiles_x * ((h + 7) >> 3)
    rows = TILE_ROWS                                  # const uint32_t rows = (uint32_t)tile_rows(sampling);
    assert tiles == ((w + 127) // 128) * ((h + rows - 1) // rows)  # return ((w + 127) / 128) * ((h + rows - 1) / rows);
    waves = G.COEF_BLOCK // 64                        # constexpr int kCoefWaves = kCoefBlock / 64;
    resident = cus * (2 if two_pass else 1)           # const uint32_t resident = (uint32_t)cus * (two_pass ? 2u : 1u);
    g = (tiles + waves - 1) // waves                  # uint32_t g = (tiles + kCoefWaves - 1) / kCoefWaves;
    if g > resident:                                  # if (g > resident) g = resident;
        g = resident
    if g > G.MAX_GRID:                                # if (g > (uint32_t)kCoefMaxGrid) g = kCoefMaxGrid;
        g = G.MAX_GRID
    if g < 1:                                         # if (g < 1) g = 1;
        g = 1
    return tiles_x, tiles, g * waves                  # const uint32_t nwaves = gridDim.x * kCoefWaves;


def coef_loop(cus, two_pass=True):
    """The smallest-tiles_x shape (even dimensions; a last tile column with two live pixels, a last tile row with four live rows) whose
    tile count lies strictly between LOW x and HIGH x the waves launched on `cus` compute units, as a tile_loop_shapes.TileLoop;
    raises NoSuchShape."""
    if cus < 1:
        raise T.NoSuchShape(f"{cus} compute units")
    rows_allowed = range(2, T.MAX_DIM // TILE_ROWS + 1)  # tile rows
    for tx in range(3, T.MAX_DIM):
        w = (tx - 1) * 128 + 2
        if w > T.MAX_DIM:
            break
        if tx & (tx - 1) == 0:
            continue
        mk = lambda r: T.TileLoop(KERNEL, w, TILE_ROWS * r - 4, *coef_walk(cus, w, TILE_ROWS * r - 4, two_pass))
        cap = mk(rows_allowed[-1]).walkers
        want = -(-int(T.TARGET * cap * 1000) // (1000 * tx))
        fits = [r for r in rows_allowed if T.satisfies(mk(r))]
        if fits:
            return mk(min(fits, key=lambda r: (abs(r - want), r)))
    raise T.NoSuchShape(f"{KERNEL}: no shape within {T.MAX_DIM} x {T.MAX_DIM} puts the tile count between {T.LOW} and {T.HIGH} times the waves of {cus} compute units")
