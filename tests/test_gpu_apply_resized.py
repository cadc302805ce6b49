"""GPU: uhdr_hip_apply_gainmap_any / _any_dev -- applyGainMap for a gain map whose aspect ratio differs from the base image's
(the reference's resize step, lib/src/jpegr.cpp:1651-1671) -- for each forced route (UHDR_HIP_APPLY_RESIZE=staged|fused) and for
the default:
  * against the old uhdr_hip_apply_gainmap_dev fed with the map tests/resize_port.py resized (no reference needed),
  * against the real reference where it is built (gamma 1: with gamma != 1 the existing tests allow the reference a tolerance),
  * stripes, the 1 % decision on both sides and at the boundary, and the old entry points' unchanged refusal."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import resize_cases as K
import resize_port as P
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image, stripe_view
from oracle import loader as L

pytestmark = pytest.mark.gpu

ROUTES = ["staged", "fused", "default"]
LINEAR, HLG, PQ = A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ
F420, F422, F444 = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCr444

# a thin matrix over (base image, map size, map format, output transfer, metadata): every base, every map geometry of
# resize_cases.GEOMETRIES, every map format, every output and every metadata kind appear, not their full product
MATRIX = [
    ("420-48x32", (10, 10), "y400", LINEAR, "plain"),
    ("420-48x32", (7, 13), "rgb888", HLG, "cg0"),
    ("420-48x32", (100, 20), "rgba8888", PQ, "perch"),
    ("420-48x32", (1, 5), "y400", PQ, "gamma"),
    ("420-48x32", (5, 1), "rgb888", LINEAR, "boost"),
    ("420-48x32", (1, 1), "rgba8888", HLG, "plain"),
    ("420-260x6", (64, 48), "y400", HLG, "boost"),
    ("420-260x6", (64, 48), "rgb888", PQ, "plain"),
    ("420-260x6", (64, 48), "rgba8888", LINEAR, "gamma"),
    ("420-260x6", (64, 48), "y400", LINEAR, "plain"),
    ("422", (64, 48), "y400", PQ, "cg0"),
    ("422", (10, 10), "rgb888", LINEAR, "perch"),
    ("444", (64, 48), "rgba8888", HLG, "gamma"),
    ("444", (7, 13), "y400", LINEAR, "plain"),
    ("rgba", (64, 48), "rgb888", HLG, "perch"),
    ("rgba", (100, 20), "y400", LINEAR, "cg0"),
    ("rgb", (64, 48), "rgba8888", PQ, "boost"),
    ("rgb", (10, 10), "y400", HLG, "plain"),
]


def _row_id(row):
    base, (mw, mh), fmt, ct, md = row
    return f"{base}/{mw}x{mh}-{fmt}/{ {LINEAR: 'linear', HLG: 'hlg', PQ: 'pq'}[ct]}/{md}"


@functools.lru_cache(maxsize=None)
def _base(kind):
    if kind.startswith("420-"):
        w, h = (int(v) for v in kind[4:].split("x"))
        return synth.make_sdr_yuv420(w, h, noise=0.05)
    w, h = 130, 66
    if kind == "422":
        return synth.make_sdr_planar(F422, w, h, noise=0.05)
    if kind == "444":
        return synth.make_sdr_planar(F444, w, h, noise=0.05)
    rgba = synth.make_sdr_rgba8888(w, h, noise=0.05)
    if kind == "rgba":
        return rgba
    img = Image(A.UHDR_IMG_FMT_24bppRGB888, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE)
    img.valid(0)[:] = np.ascontiguousarray(rgba.valid(0)).view(np.uint8).reshape(h, w, 4)[:, :, :3].reshape(h, w * 3)
    return img


def _metadata(kind):
    """-> (metadata, max_display_boost, the gain map's gamut)"""
    if kind == "plain":
        return synth.default_metadata(use_base_cg=1), A.FLT_MAX, A.UHDR_CG_UNSPECIFIED
    if kind == "cg0":  # the gain map carries the HDR gamut and the base image is converted to it
        return synth.default_metadata(use_base_cg=0), A.FLT_MAX, A.UHDR_CG_BT_2100
    if kind == "perch":
        return synth.default_metadata(use_base_cg=1, per_channel=True), A.FLT_MAX, A.UHDR_CG_DISPLAY_P3
    if kind == "gamma":
        return synth.default_metadata(gamma=1.7, use_base_cg=1), A.FLT_MAX, A.UHDR_CG_UNSPECIFIED
    return synth.default_metadata(use_base_cg=1), 2.5, A.UHDR_CG_UNSPECIFIED  # "boost": gain-map weight < 1


def _out_fmt(ct):
    return A.UHDR_IMG_FMT_64bppRGBAHalfFloat if ct == LINEAR else A.UHDR_IMG_FMT_32bppRGBA1010102


class _Route:
    """UHDR_HIP_APPLY_RESIZE for the duration of a call ("default": unset)."""

    def __init__(self, route):
        self.route = route

    def __enter__(self):
        self.old = os.environ.pop("UHDR_HIP_APPLY_RESIZE", None)
        if self.route != "default":
            os.environ["UHDR_HIP_APPLY_RESIZE"] = self.route

    def __exit__(self, *exc):
        os.environ.pop("UHDR_HIP_APPLY_RESIZE", None)
        if self.old is not None:
            os.environ["UHDR_HIP_APPLY_RESIZE"] = self.old


def _apply(ctx, fn_name, base_dev, gm_dev, md, ct, boost, route="default", check=True):
    dest = Image(_out_fmt(ct), base_dev.w, base_dev.h, align=4, device="cuda:0")
    with _Route(route):
        st = getattr(ctx.lib, fn_name)(ctx.handle, C.byref(base_dev.raw), C.byref(gm_dev.raw), C.byref(md), ct, _out_fmt(ct), boost,
                                       C.byref(dest.raw), 0, 0)
    if not check:
        return st
    A.check(st)
    ctx.synchronize()
    return dest.to_host().valid(0)


@functools.lru_cache(maxsize=None)
def _row_inputs(row):
    base_kind, (mw, mh), fmt_name, ct, md_kind = row
    base = _base(base_kind)
    md, boost, map_cg = _metadata(md_kind)
    gm = K.make_map(K.FORMATS[fmt_name], mw, mh, cg=map_cg)
    assert P.needs_resize(base.w, base.h, mw, mh)
    return base, gm, P.resize_image(gm, base.w, base.h), md, boost


@functools.lru_cache(maxsize=None)
def _row_expected(ctx, row):
    """The old entry point on the port-resized map: computed once per row, shared by the three routes."""
    base, gm, resized, md, boost = _row_inputs(row)
    want = _apply(ctx, "uhdr_hip_apply_gainmap_dev", base.to("cuda:0"), resized.to("cuda:0"), md, row[3], boost)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("row", MATRIX, ids=[_row_id(r) for r in MATRIX])
def test_any_equals_the_old_entry_point_on_the_port_resized_map(hip_ctx, row, route):
    base, gm, resized, md, boost = _row_inputs(row)
    want = _row_expected(hip_ctx, row)
    got = _apply(hip_ctx, "uhdr_hip_apply_gainmap_any_dev", base.to("cuda:0"), gm.to("cuda:0"), md, row[3], boost, route)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} output pixels differ"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("row", [r for r in MATRIX if r[4] != "gamma"], ids=[_row_id(r) for r in MATRIX if r[4] != "gamma"])
def test_any_equals_the_reference(hip_ctx, ref, row, route):
    base, gm, resized, md, boost = _row_inputs(row)
    want = L.apply_gainmap("ref", base, gm, md, row[3], boost).valid(0)
    got = _apply(hip_ctx, "uhdr_hip_apply_gainmap_any_dev", base.to("cuda:0"), gm.to("cuda:0"), md, row[3], boost, route)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} output pixels differ"


@pytest.mark.parametrize("route", ROUTES)
def test_host_form_and_python_wrapper(hip_ctx, route):
    from libultrahdr_amd.ultrahdr import UltraHdr

    row = MATRIX[1]
    base, gm, resized, md, boost = _row_inputs(row)
    dest = Image(_out_fmt(row[3]), base.w, base.h, align=4)
    with _Route(route):
        UltraHdr(ctx=hip_ctx).applyGainMapAny(base, gm, md, row[3], _out_fmt(row[3]), boost, dest)
    assert np.array_equal(dest.valid(0), _row_expected(hip_ctx, row))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("row", [MATRIX[0], MATRIX[8], MATRIX[12]], ids=[_row_id(MATRIX[i]) for i in (0, 8, 12)])
def test_two_stripes_stitch_to_the_whole_image(hip_ctx, row, route):
    base, gm, resized, md, boost = _row_inputs(row)
    ct = row[3]
    want = _row_expected(hip_ctx, row)
    bd, gd = base.to("cuda:0"), gm.to("cuda:0")
    dest = Image(_out_fmt(ct), base.w, base.h, align=4, device="cuda:0")
    cut = (base.h // 3) & ~1
    with _Route(route):
        for y0, rows in ((0, cut), (cut, base.h - cut)):
            s, d = stripe_view(bd, y0, rows), stripe_view(dest, y0, rows)
            A.check(hip_ctx.lib.uhdr_hip_apply_gainmap_any_dev(hip_ctx.handle, C.byref(s), C.byref(gd.raw), C.byref(md), ct, _out_fmt(ct), boost,
                                                               C.byref(d), y0, base.h))
    hip_ctx.synchronize()
    assert np.array_equal(dest.to_host().valid(0), want)


# Base 400x200 (aspect 2.0).  Which side of the reference's `fabs(pa - ga) / pa > 0.01f` a map falls on is computed here in numpy
# float32, exactly as written there, never assumed:
#   200x101  1.9802: 0.99 % off, within the tolerance -- exactly the old entry point's bytes
#   101x50   2.02:   the boundary, 1 % on paper; float32 decides
#   100x51   1.9608: 1.96 % off, so beyond the tolerance although it differs by one row only
DECISION_MAPS = [(200, 101), (101, 50), (100, 51)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("map_size", DECISION_MAPS, ids=["%dx%d" % m for m in DECISION_MAPS])
def test_the_decision_follows_the_float_expression(hip_ctx, map_size, route):
    base = synth.make_sdr_yuv420(400, 200)
    gm = synth.make_gainmap(map_size[0], map_size[1], 1)
    md = synth.default_metadata()
    bd = base.to("cuda:0")
    resize = P.needs_resize(400, 200, *map_size)
    if map_size == (200, 101):
        assert not resize
    if map_size == (100, 51):
        assert resize
    old = _apply(hip_ctx, "uhdr_hip_apply_gainmap_dev", bd, gm.to("cuda:0"), md, PQ, A.FLT_MAX, check=False)
    if resize:
        assert old.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
        want = _apply(hip_ctx, "uhdr_hip_apply_gainmap_dev", bd, P.resize_image(gm, 400, 200).to("cuda:0"), md, PQ, A.FLT_MAX)
    else:
        assert old.error_code == A.UHDR_CODEC_OK
        want = _apply(hip_ctx, "uhdr_hip_apply_gainmap_dev", bd, gm.to("cuda:0"), md, PQ, A.FLT_MAX)
    got = _apply(hip_ctx, "uhdr_hip_apply_gainmap_any_dev", bd, gm.to("cuda:0"), md, PQ, A.FLT_MAX, route)
    assert np.array_equal(got, want)


def test_the_old_entry_points_still_refuse(hip_ctx):
    base, gm, resized, md, boost = _row_inputs(MATRIX[0])
    st = _apply(hip_ctx, "uhdr_hip_apply_gainmap_dev", base.to("cuda:0"), gm.to("cuda:0"), md, LINEAR, boost, check=False)
    assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE and b"resize_image fallback" in st.detail
    dest = Image(_out_fmt(LINEAR), base.w, base.h, align=4)
    st = hip_ctx.lib.uhdr_hip_apply_gainmap(hip_ctx.handle, C.byref(base.raw), C.byref(gm.raw), C.byref(md), LINEAR, _out_fmt(LINEAR), boost,
                                            C.byref(dest.raw))
    assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    bd, gd = base.to("cuda:0"), gm.to("cuda:0")
    ddev = Image(_out_fmt(LINEAR), base.w, base.h, align=4, device="cuda:0")
    n = 2
    arr = lambda im: (A.RawImage * n)(*[im.raw] * n)
    st = hip_ctx.lib.uhdr_hip_apply_gainmap_batch_dev(hip_ctx.handle, n, arr(bd), arr(gd), C.byref(md), LINEAR, _out_fmt(LINEAR), boost, arr(ddev))
    assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
