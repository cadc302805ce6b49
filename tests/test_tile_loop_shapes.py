"""CPU: tests/tile_loop_shapes.py -- the shapes test_gpu_tile_loops.py runs really leave every persistent tile loop on its second
trip, for the compute-unit counts of the gfx9 parts (64, 256, 304), and the helper says so loudly where no shape can.  The same for the
per-pixel routes of the oldest launchers (T.NARROW_KERNELS), whose shapes also have to suit the vector route of the same operator."""
import os

import pytest

import tile_loop_shapes as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libultrahdr_amd", "csrc")
# elements (quads, blocks, pixels, elements) per tile along a row, and image columns per element
TILE = {"p010_two_pass": (64, 2), "p010_one_pass": (64, 2), "rgba": (8, 8), "resize": (1024, 1), "effects": (256, 1),
        "yuv420": (256, 2), "rgb420": (256, 2), "yuv444": (256, 1), "rgb444": (256, 1), "jpeg_colour": (256, 1), "tone_pixel": (256, 1), "tone_p010": (64, 2)}
# pixels per vector tile of the same operator's vector route: the narrow shapes are whole ones, so the same samples run on both
VECTOR_TILE = {"yuv420": 8, "rgb420": 8, "yuv444": 8, "rgb444": 8, "jpeg_colour": 4, "tone_pixel": 1, "tone_p010": 2}


def _walk(loop, cus):
    return {"p010_two_pass": lambda: T.p010_walk(cus, loop.w, loop.h, True), "p010_one_pass": lambda: T.p010_walk(cus, loop.w, loop.h, False),
            "rgba": lambda: T.rgba_walk(cus, loop.w, loop.h), "resize": lambda: T.resize_walk(loop.w, loop.h),
            "effects": lambda: T.effect_walk(loop.w, loop.h),
            "yuv420": lambda: T.convert420_walk(loop.w, loop.h), "rgb420": lambda: T.convert420_walk(loop.w, loop.h),
            "yuv444": lambda: T.convert444_walk(loop.w, loop.h), "rgb444": lambda: T.convert444_walk(loop.w, loop.h),
            "jpeg_colour": lambda: T.jpeg_colour_walk(cus, loop.w, loop.h), "tone_pixel": lambda: T.tone_pixel_walk(cus, loop.w, loop.h),
            "tone_p010": lambda: T.tone_p010_walk(cus, loop.w, loop.h)}[loop.kernel]()


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("kernel", T.KERNELS + T.NARROW_KERNELS)
def test_shape_leaves_the_loop_on_its_second_trip(kernel, cus):
    loop = T.tile_loop(kernel, cus)
    print(T.describe(loop))
    assert loop.kernel == kernel and (loop.tiles_x, loop.items, loop.walkers) == _walk(loop, cus)
    assert 0 < loop.w <= 8192 and 0 < loop.h <= 8192
    assert 1.25 * loop.walkers < loop.items < 2.5 * loop.walkers  # some walkers take two trips, some one, none three
    assert loop.tiles_x >= 3 and loop.tiles_x & (loop.tiles_x - 1) != 0
    per_tile, px = TILE[kernel]
    assert loop.w % px == 0 and (loop.w // px) % per_tile != 0, "the last tile of a row is ragged"
    assert -(-(loop.w // px) // per_tile) == loop.tiles_x
    if kernel.startswith("p010") or kernel == "effects":
        assert loop.w % 2 == 0 and loop.h % 2 == 0  # whole chroma planes
    if kernel == "rgba":
        assert loop.w % 8 == 0 and loop.h % 8 == 0  # whole blocks, for the map too
    if kernel == "resize":
        assert loop.w % 4 != 0  # the last run of four pixels is ragged too
    if kernel in T.NARROW_KERNELS:
        assert loop.w % VECTOR_TILE[kernel] == 0  # the vector route of the same operator takes the width as well
        if kernel.endswith("420") or kernel == "tone_p010":
            assert loop.h % 2 == 0
    if kernel in T.AT_CAP:
        assert loop.walkers == 4096  # grid_for's cap, not just a ragged row


def test_the_grid_arithmetic_on_known_shapes():
    """256 compute units, figures worked out by hand from the launchers."""
    assert T.p010_walk(256, 258, 8190, True) == (3, 12285, 6144)   # 3 x 256 workgroups of 8 waves
    assert T.p010_walk(256, 258, 8190, False) == (3, 12285, 6144)  # 2 x 256 workgroups of 12 waves
    assert T.p010_walk(256, 144, 34, True) == (2, 34, 40)          # five workgroups: more waves than tiles
    assert T.p010_walk(1024, 8192, 8192, True) == (64, 262144, 2048 * 8)  # 3072 resident: the 2048 cap of the partials buffer
    assert T.rgba_walk(256, 520, 8000) == (9, 9000, 7168)          # 7 x 256 workgroups of 4 waves
    assert T.rgba_walk(256, 96, 32) == (2, 8, 8)
    assert T.resize_walk(2050, 7000) == (3, 21000, 16384)
    assert T.resize_walk(1027, 3) == (2, 6, 6)
    assert T.effect_walk(520, 7000) == (3, 21000, 16384)
    assert T.effect_walk(208, 144) == (1, 144, 144)
    assert T.convert420_walk(1032, 4066) == (3, 6099, 4096)        # 516 quads per row: three tiles, 2.02 workgroups' worth; the cap
    assert T.convert420_walk(1032, 3550) == (3, 5325, 3578)        # below the cap the ragged row alone makes second trips
    assert T.convert420_walk(130, 66) == (1, 33, 9)
    assert T.convert444_walk(520, 2017) == (3, 6051, 4096)
    assert T.convert444_walk(131, 17) == (1, 17, 9)
    assert T.jpeg_colour_walk(256, 516, 888) == (3, 2664, 2048)    # 8 x 256 workgroups
    assert T.jpeg_colour_walk(256, 131, 17) == (1, 17, 17)
    assert T.tone_pixel_walk(256, 516, 444) == (3, 1332, 1024)     # 4 x 256 workgroups
    assert T.tone_p010_walk(256, 258, 7100) == (3, 10650, 8192)    # 4 x 256 workgroups of 8 waves
    assert T.tone_p010_walk(256, 256, 96) == (2, 96, 96)           # twelve workgroups


def test_no_shape_is_an_error():
    # 100000 compute units keep 2.8 million waves of base_blocks_rgba_kernel resident; an 8192 x 8192 image has 131072 groups
    with pytest.raises(T.NoSuchShape):
        T.tile_loop("rgba", 100000)
    with pytest.raises(T.NoSuchShape):  # 8192 x 8192 has 12288 row tiles for 400000 resident waves of tonemap_p010_kernel
        T.tile_loop("tone_p010", 100000)
    for kernel in T.KERNELS + T.NARROW_KERNELS:
        with pytest.raises(T.NoSuchShape):
            T.tile_loop(kernel, 0)
    with pytest.raises(ValueError):
        T.tile_loop("no such kernel", 256)


def test_the_restated_source_lines_still_read_the_same():
    text = {}
    for name, line in T.MIRRORED:
        if name not in text:
            with open(os.path.join(CSRC, name)) as f:
                text[name] = f.read()
        assert line in text[name], f"{name} no longer contains `{line}`: tests/tile_loop_shapes.py restates it"
