"""The shape at which map_blocks_onepass_kernel's strip loop takes a second trip: the one-pass sibling of tests/tile_loop_shapes.py,
whose search rules (LOW, HIGH, TARGET, MAX_DIM, satisfies, NoSuchShape) it keeps.  launch_map_blocks_onepass caps its grid at two
512-thread workgroups per compute unit and every WAVE walks `for (t = gwave; t < total; t += nwaves)` over strips of eight 8 x 8 map
blocks; the launcher's grid arithmetic is restated here and MIRRORED lists the source lines, which tests/test_tile_loop_shapes_onepass.py
checks still read the same.  No imports beyond the standard library and that module."""
import tile_loop_shapes as T

KERNEL = "map_onepass"
MAP_BLOCK = 512  # constexpr int kMapBlock = 512;
PER_CU = 2       # const int cap = resident_grid(1 << 30, 2);

# (file under libultrahdr_amd/csrc, text): what onepass_walk restates
MIRRORED = [
    ("encode_api1_fused.hip", "constexpr int kMapBlock = 512;"),
    ("encode_api1_fused.hip", "p.bw = (int)(g.map_w / 8); p.bh = (int)(g.map_h / 8);"),
    ("encode_api1_fused.hip", "int grid = (((p.bw + 7) / 8) * p.bh + kMapBlock / 64 - 1) / (kMapBlock / 64);"),
    ("encode_api1_fused.hip", "const int cap = resident_grid(1 << 30, 2);"),
    ("encode_api1_fused.hip", "if (grid > cap) grid = cap;"),
    ("encode_api1_fused.hip", "if (grid > cus * per_cu) grid = cus * per_cu;"),
    ("encode_api1_fused.hip", "constexpr int kBlock = kMapBlock;"),
    ("encode_api1_fused.hip", "const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;"),
    ("encode_api1_fused.hip", "const int gwave = blockIdx.x * (kBlock / 64) + wv, nwaves = gridDim.x * (kBlock / 64);"),
]


def onepass_walk(cus, w, h, scale=1):
    """(groups_x, items, walkers) of map_blocks_onepass_kernel on a w x h pair of intents at this scale factor; a walker is a wave."""
    bw, bh = (w // scale) // 8, (h // scale) // 8        # p.bw = (int)(g.map_w / 8); p.bh = (int)(g.map_h / 8);
    groups_x = (bw + 7) >> 3                             # const int groups_x = (p.bw + 7) >> 3, total = groups_x * p.bh;
    total = groups_x * bh
    waves = MAP_BLOCK // 64
    grid = (((bw + 7) // 8) * bh + waves - 1) // waves   # int grid = (((p.bw + 7) / 8) * p.bh + kMapBlock / 64 - 1) / (kMapBlock / 64);
    cap = T.resident_grid(cus, 1 << 30, PER_CU)          # const int cap = resident_grid(1 << 30, 2);
    if grid > cap:                                       # if (grid > cap) grid = cap;
        grid = cap
    return groups_x, total, grid * waves                 # nwaves = gridDim.x * (kBlock / 64), kBlock = kMapBlock inside the kernel


def onepass_loop(cus, scale=1):
    """The smallest-groups_x 4:2:0 shape (dimensions multiples of 16 x scale, a ragged last strip of two blocks) whose strip count lies
    strictly between LOW x and HIGH x the waves launched on `cus` compute units, as a tile_loop_shapes.TileLoop; raises NoSuchShape."""
    if cus < 1:
        raise T.NoSuchShape(f"{cus} compute units")
    rows_allowed = range(2, T.MAX_DIM // (8 * scale) + 1, 2)  # block rows: heights that are multiples of 16 x scale
    for tx in range(3, T.MAX_DIM):
        w = scale * 8 * ((tx - 1) * 8 + 2)
        if w > T.MAX_DIM:
            break
        if tx & (tx - 1) == 0:
            continue
        mk = lambda r: T.TileLoop(KERNEL, w, scale * 8 * r, *onepass_walk(cus, w, scale * 8 * r, scale))
        cap = mk(rows_allowed[-1]).walkers
        want = -(-int(T.TARGET * cap * 1000) // (1000 * tx))
        fits = [r for r in rows_allowed if T.satisfies(mk(r))]
        if fits:
            return mk(min(fits, key=lambda r: (abs(r - want), r)))
    raise T.NoSuchShape(f"{KERNEL}: no shape within {T.MAX_DIM} x {T.MAX_DIM} puts the strip count between {T.LOW} and {T.HIGH} times the waves of {cus} compute units")
