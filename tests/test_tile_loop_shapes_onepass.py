"""CPU: tests/tile_loop_shapes_onepass.py -- the lines of launch_map_blocks_onepass / map_blocks_onepass_kernel it restates still read
the same in the source, its shapes obey the rules of tests/tile_loop_shapes.py on the devices the project meets, and it raises where
there is no shape."""
import os

import pytest

import tile_loop_shapes as T
import tile_loop_shapes_onepass as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libultrahdr_amd", "csrc")


def test_the_restated_lines_still_read_the_same_in_the_source():
    for name, text in O.MIRRORED:
        assert text in open(os.path.join(CSRC, name)).read(), f"{name} no longer contains: {text}"


@pytest.mark.parametrize("cus", [64, 104, 228, 256, 304])
@pytest.mark.parametrize("scale", [1, 2])
def test_shapes_reach_the_second_trip_and_fit_a_420_pair(cus, scale):
    loop = O.onepass_loop(cus, scale)
    assert T.satisfies(loop)
    assert loop.w % (16 * scale) == 0 and loop.h % (16 * scale) == 0 and ((loop.w // scale) // 8) % 8 == 2
    assert (loop.tiles_x, loop.items, loop.walkers) == O.onepass_walk(cus, loop.w, loop.h, scale)
    assert loop.walkers == cus * O.PER_CU * (O.MAP_BLOCK // 64)


def test_the_walk_on_256_compute_units():
    # 528 x 8192 at scale 1: 66 blocks across (eight full strips and one of two blocks), 1024 block rows; two workgroups of eight waves per CU
    assert O.onepass_walk(256, 528, 8192) == (9, 9216, 4096)
    # a small image launches only the workgroups it has strips for
    assert O.onepass_walk(256, 144, 48) == (3, 18, 24)


def test_it_raises_where_no_shape_exists():
    with pytest.raises(T.NoSuchShape):
        O.onepass_loop(0)
    with pytest.raises(T.NoSuchShape):
        O.onepass_loop(100000)  # more waves than the largest image has strips
