"""CPU: tests/tile_loop_shapes_api3_444.py -- the lines of generate_coef.hip and coef_tile.h it restates for the eight-row tile of a
4:4:4 SDR intent still read the same in the source, its shapes obey the rules of tests/tile_loop_shapes.py on the devices the project
meets, and it raises where there is no shape."""
import os

import pytest

import tile_loop_shapes as T
import tile_loop_shapes_api3 as G
import tile_loop_shapes_api3_444 as G8

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libultrahdr_amd", "csrc")


def test_the_restated_lines_still_read_the_same_in_the_source():
    assert len(G8.MIRRORED) > len(G.MIRRORED)
    for name, text in G8.MIRRORED:
        assert text in open(os.path.join(CSRC, name)).read(), f"{name} no longer contains: {text}"


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("two_pass", [True, False])
def test_shapes_reach_the_second_trip_with_ragged_last_tiles(cus, two_pass):
    loop = G8.coef_loop(cus, two_pass)
    assert T.satisfies(loop)
    assert loop.w % 2 == 0 and loop.h % 2 == 0 and loop.w % 128 == 2 and loop.h % 8 == 4
    assert (loop.tiles_x, loop.items, loop.walkers) == G8.coef_walk(cus, loop.w, loop.h, two_pass)
    assert loop.walkers == min(cus * (2 if two_pass else 1), G.MAX_GRID) * (G.COEF_BLOCK // 64)


def test_the_walk_on_256_compute_units():
    # 3840 x 2176: 30 x 272 eight-row tiles, twice the sixteen-row tiles of the other samplings: two trips two pass, four one pass
    assert G8.coef_walk(256, 3840, 2176, True) == (30, 8160, 4096)
    assert G8.coef_walk(256, 3840, 2176, False) == (30, 8160, 2048)
    assert G8.coef_walk(256, 3840, 2176, True)[1] == 2 * G.coef_walk(256, 3840, 2176, True)[1]
    # a small image launches only the workgroups it has tiles for
    assert G8.coef_walk(256, 392, 100) == (4, 52, 56)
    assert G8.coef_walk(256, 16, 8) == (1, 1, 8)
    assert G8.coef_walk(256, 130, 10) == (2, 4, 8)


def test_it_raises_without_compute_units_and_the_grid_cap_bounds_the_walkers():
    with pytest.raises(T.NoSuchShape):
        G8.coef_loop(0)
    loop = G8.coef_loop(100000)  # whatever the device, 2048 workgroups is the most that is launched: a shape exists
    assert T.satisfies(loop) and loop.walkers == G.MAX_GRID * (G.COEF_BLOCK // 64)
