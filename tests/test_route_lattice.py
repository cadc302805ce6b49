"""CPU: tests/route_lattice.py -- the case table of tests/test_gpu_route_lattice.py really reaches every kernel route of the
pixel-format launchers, flips every conjunct of every vector-route predicate on its own, and builds every view inside its frame;
and the launcher lines the table restates still read the same."""
import os

import numpy as np
import pytest

import framed as F
import route_lattice as RL
from libultrahdr_amd.images import Image

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libultrahdr_amd", "csrc")


def _text(name, cache={}):
    if name not in cache:
        with open(os.path.join(CSRC, name)) as f:
            cache[name] = f.read()
    return cache[name]


def test_the_restated_source_lines_still_read_the_same():
    for name, line in RL.MIRRORED:
        assert line in _text(name), f"{name} no longer contains `{line}`: tests/route_lattice.py restates it"


def test_the_refusals_are_where_the_table_says():
    for launcher, what, name, line in RL.REFUSED:
        assert line in _text(name), f"{name} no longer contains `{line}`, the check that keeps callers off {what}"
        assert any(RL.route(c) == ("refused",) for c in RL.cases_of(launcher)), f"no case of {launcher} pins the refusal"


@pytest.mark.parametrize("launcher", list(RL.ROUTES))
def test_every_route_is_selected_by_a_case(launcher):
    taken = {r for c in RL.cases_of(launcher) for r in RL.route(c)}
    assert taken == set(RL.ROUTES[launcher]), (sorted(set(RL.ROUTES[launcher]) - taken), sorted(taken - set(RL.ROUTES[launcher])))


def test_every_case_belongs_to_a_launcher_and_has_a_name_of_its_own():
    names = [(c.launcher, c.name) for c in RL.CASES]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    assert {c.launcher for c in RL.CASES} == set(RL.ROUTES)
    print(RL.describe())


@pytest.mark.parametrize("pid", list(RL.PREDICATES))
def test_every_conjunct_has_a_pair_that_flips_it_alone(pid):
    applies, conj = RL.PREDICATES[pid]
    assert any(applies(c) and all(v for _, v in conj(c)) for c in RL.CASES), f"{pid}: no case takes the vector route"
    pairs = RL.flipping_pairs(pid)
    assert pairs, pid
    for name, pair in pairs.items():
        assert pair is not None, f"{pid}: no case in which `{name}` alone is false"
        on, off = pair
        assert RL.route(on) != RL.route(off), f"{pid}: {on.name} and {off.name} differ in `{name}` alone and take the same route {RL.route(on)}"
        print(f"{pid}: `{name}`: {on.name} {RL.route(on)} | {off.name} {RL.route(off)}")


def test_the_table_stays_small():
    for c in RL.CASES:
        if c.launcher in ("tone_map", "generate"):
            assert (c.w, c.h) in ((256, 96), (255, 96), (256, 95), (252, 96), (254, 96), (250, 96)), c.name  # tests/test_gpu_formats.py's size and its crops
        else:
            assert c.w < 100 and c.h < 100, c.name


def test_fdct_quant_has_an_odd_stride_and_an_odd_base():
    cs = RL.cases_of("fdct_quant")
    assert any(c.a.strides[0] % 2 == 1 and c.a.offsets[0] % 4 == 0 for c in cs)
    assert any(c.a.offsets[0] % 2 == 1 and c.a.strides[0] % 4 == 0 for c in cs)
    assert any(c.a.offsets[0] % 2 == 1 and c.a.strides[0] % 2 == 1 for c in cs)


def _random_image(fmt, w, h, seed):
    img = Image(fmt, w, h, align=1)
    img.buf[:] = np.random.default_rng(seed).integers(0, 256, img.buf.size, dtype=np.uint8)
    return img


@pytest.mark.parametrize("case", RL.CASES, ids=lambda c: f"{c.launcher}:{c.name}")
def test_every_view_lies_inside_its_frame(case):
    """Host frames of every image of every case: the view is where the case puts it, the valid samples read back as written, and
    the frame check passes on the fresh frame and trips on a byte behind a row, in front of the base and in a guard row."""
    for k, lay in enumerate((case.a, case.b, case.c)):
        if lay is None:
            continue
        w, h = case.w, case.h
        if case.launcher == "generate" and k == 2:
            w, h = w // case.opt["scale"], h // case.opt["scale"]
        src = _random_image(lay.fmt, w + w % 2, h + h % 2, 7 + k)  # (an odd-sized view is the crop of an even-sized image)
        fr = F.framed(lay.fmt, w, h, lay.strides, lay.offsets, src=src, device=None)
        assert F.view_inside_frame(fr)
        for i, pl in enumerate(fr.planes):
            assert fr.raw.planes[i] % 256 == lay.offsets[i] and fr.raw.stride[i] == lay.strides[i]
            assert pl.base >= F.GUARD_ROWS * pl.pitch and pl.nbytes - (pl.base + pl.rows * pl.pitch) >= (F.GUARD_ROWS - 1) * pl.pitch
        want = F.tight(lay.fmt, w, h, src).planes_valid()
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(fr.valid(), want))
        F.assert_frame_intact(fr, written=())
        pl = fr.planes[-1]
        spots = [pl.base - 1, pl.base - pl.pitch, pl.base + pl.rows * pl.pitch, pl.nbytes - 1]
        if pl.width < pl.pitch:
            spots.append(pl.base + pl.width)
        for spot in spots:
            fr.bufs[-1][spot] ^= 0xFF
            with pytest.raises(AssertionError):
                F.assert_frame_intact(fr)
            fr.bufs[-1][spot] ^= 0xFF
        fr.bufs[-1][pl.base] ^= 0xFF  # a valid sample: a destination may change it, an input may not
        F.assert_frame_intact(fr)
        with pytest.raises(AssertionError):
            F.assert_frame_intact(fr, written=())
