"""CPU: tests/tile_loop_shapes_api3.py -- the lines of launch_generate_gainmap_coef / generate_coef_kernel it restates still read the
same in the source, its shapes obey the rules of tests/tile_loop_shapes.py on the devices the project meets, and it raises where there
is no shape."""
import os

import pytest

import tile_loop_shapes as T
import tile_loop_shapes_api3 as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libultrahdr_amd", "csrc")


def test_the_restated_lines_still_read_the_same_in_the_source():
    for name, text in G.MIRRORED:
        assert text in open(os.path.join(CSRC, name)).read(), f"{name} no longer contains: {text}"


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("two_pass", [True, False])
def test_shapes_reach_the_second_trip_with_ragged_last_tiles(cus, two_pass):
    loop = G.coef_loop(cus, two_pass)
    assert T.satisfies(loop)
    assert loop.w % 2 == 0 and loop.h % 2 == 0 and loop.w % 128 == 2 and loop.h % 16 == 8
    assert (loop.tiles_x, loop.items, loop.walkers) == G.coef_walk(cus, loop.w, loop.h, two_pass)
    assert loop.walkers == min(cus * (2 if two_pass else 1), G.MAX_GRID) * (G.COEF_BLOCK // 64)


def test_the_walk_on_256_compute_units():
    # 3840 x 2176: 30 x 136 tiles; two workgroups of eight waves per CU take them in one trip, one workgroup per CU in two
    assert G.coef_walk(256, 3840, 2176, True) == (30, 4080, 4080)
    assert G.coef_walk(256, 3840, 2176, False) == (30, 4080, 2048)
    # a small image launches only the workgroups it has tiles for
    assert G.coef_walk(256, 392, 200) == (4, 52, 56)
    assert G.coef_walk(256, 16, 16) == (1, 1, 8)


def test_it_raises_without_compute_units_and_the_grid_cap_bounds_the_walkers():
    with pytest.raises(T.NoSuchShape):
        G.coef_loop(0)
    loop = G.coef_loop(100000)  # whatever the device, 2048 workgroups is the most that is launched: a shape exists
    assert T.satisfies(loop) and loop.walkers == G.MAX_GRID * (G.COEF_BLOCK // 64)
