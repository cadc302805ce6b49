"""GPU: uhdr_hip_resize_image_dev / uhdr_hip_resize_image -- the reference's resize_image (lib/src/editorhelper.cpp:88-146) for Y400,
RGB888 and RGBA8888 -- against tests/resize_port.py (pinned to the reference by test_resize_port.py), byte for byte."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_cases as K
import resize_port as P
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image, bytes_per_sample

pytestmark = pytest.mark.gpu

VALUES = ["random", "zeros", "ones", "checker"]
CASES = [(g, f) for g in K.GEOMETRIES for f in K.FORMATS]


@functools.lru_cache(maxsize=None)
def _source_and_expected(geom, fmt_name, values):
    (sw, sh), (dw, dh) = geom
    src = K.make_map(K.FORMATS[fmt_name], sw, sh, values, align=24)  # rows of a multiple of 24 pixels: every stride is larger than its width
    assert src.raw.stride[0] > src.w
    want = P.resize_channels(P.channels_of(src), src.fmt, dw, dh)
    want.setflags(write=False)
    return src, want


def _expect(img: Image, want, x0=0):
    """The destination's pixels x0 .. x0 + want.shape[1] hold `want` (and alpha 255)."""
    ch = P.channels_of(img)[:, x0: x0 + want.shape[1]]
    assert np.array_equal(ch, want), f"{(ch != want).sum()} of {want.size} bytes differ"
    if img.fmt == K.RGBA8888:
        assert np.all(img.valid(0)[:, x0: x0 + want.shape[1]] >> 24 == 255)


@pytest.mark.parametrize("geom,fmt_name", CASES, ids=[K.geom_id(g) + "/" + f for g, f in CASES])
def test_resize_equals_the_port(hip_ctx, geom, fmt_name):
    (sw, sh), (dw, dh) = geom
    lib = hip_ctx.lib
    for values in VALUES:
        src, want = _source_and_expected(geom, fmt_name, values)
        dsrc = src.to("cuda:0")
        # device form, rows aligned to 64 pixels
        dst = Image(src.fmt, dw, dh, align=64, device="cuda:0", fill=0x33)
        A.check(lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(dsrc.raw), C.byref(dst.raw), 0, 0))
        hip_ctx.synchronize()
        _expect(dst.to_host(), want)
        # device form, a destination that starts one pixel into a row of dw + 3 pixels: no row is 16-byte aligned
        # (Y400 and RGB888 rows are not even 4-byte aligned), and the pixels around it must stay as they were
        wide = Image(src.fmt, dw + 3, dh, align=1, device="cuda:0", fill=0x33)
        view = A.RawImage()
        C.memmove(C.byref(view), C.byref(wide.raw), C.sizeof(A.RawImage))
        view.w = dw
        view.planes[0] = wide.raw.planes[0] + bytes_per_sample(src.fmt)
        A.check(lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(dsrc.raw), C.byref(view), 0, 0))
        hip_ctx.synchronize()
        got = wide.to_host()
        _expect(got, want, x0=1)
        raw = got.plane(0).view(np.uint8).reshape(dh, -1)
        bpp = bytes_per_sample(src.fmt)
        assert np.all(raw[:, :bpp] == 0x33) and np.all(raw[:, (dw + 1) * bpp:] == 0x33), "bytes outside the destination were written"
        # host form
        hdst = Image(src.fmt, dw, dh, align=1, fill=0x33)
        A.check(lib.uhdr_hip_resize_image(hip_ctx.handle, C.byref(src.raw), C.byref(hdst.raw)))
        _expect(hdst, want)


@pytest.mark.parametrize("fmt_name", sorted(K.FORMATS))
def test_a_stripe_equals_those_rows_of_the_whole_call(hip_ctx, fmt_name):
    geom = K.GEOMETRIES[1]
    (sw, sh), (dw, dh) = geom
    src, want = _source_and_expected(geom, fmt_name, "random")
    dsrc = src.to("cuda:0")
    y0, rows = 5, 15  # rows 5..20 of 32
    dst = Image(src.fmt, dw, rows, align=64, device="cuda:0")
    A.check(hip_ctx.lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(dsrc.raw), C.byref(dst.raw), y0, dh))
    hip_ctx.synchronize()
    _expect(dst.to_host(), want[y0: y0 + rows])


def test_python_wrapper(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    src, want = _source_and_expected(K.GEOMETRIES[0], "rgb888", "random")
    u = UltraHdr(ctx=hip_ctx)
    _expect(u.resizeImage(src, 48, 32), want)
    out = u.resizeImage(src.to("cuda:0"), 48, 32)
    hip_ctx.synchronize()
    _expect(out.to_host(), want)


def test_refusals(hip_ctx):
    lib = hip_ctx.lib
    src = K.make_map(K.Y400, 10, 10)
    dst = Image(K.Y400, 48, 32)
    for fmt in (A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_24bppYCbCr444, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCrP010,
                A.UHDR_IMG_FMT_32bppRGBA1010102, A.UHDR_IMG_FMT_64bppRGBAHalfFloat):
        s, d = Image(fmt, 16, 16), Image(fmt, 48, 32)
        for fn, extra in ((lib.uhdr_hip_resize_image, ()), (lib.uhdr_hip_resize_image_dev, (0, 0))):
            st = fn(hip_ctx.handle, C.byref(s.raw), C.byref(d.raw), *extra)
            assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE, fmt
    inv = A.UHDR_CODEC_INVALID_PARAM
    assert lib.uhdr_hip_resize_image(None, C.byref(src.raw), C.byref(dst.raw)).error_code == inv
    assert lib.uhdr_hip_resize_image(hip_ctx.handle, None, C.byref(dst.raw)).error_code == inv
    assert lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(src.raw), None, 0, 0).error_code == inv
    for which in ("src", "dst"):  # null planes
        s, d = K.make_map(K.Y400, 10, 10), Image(K.Y400, 48, 32)
        (s if which == "src" else d).raw.planes[0] = None
        assert lib.uhdr_hip_resize_image(hip_ctx.handle, C.byref(s.raw), C.byref(d.raw)).error_code == inv
        assert lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(s.raw), C.byref(d.raw), 0, 0).error_code == inv
    other = Image(K.RGB888, 48, 32)  # the format is kept
    assert lib.uhdr_hip_resize_image(hip_ctx.handle, C.byref(src.raw), C.byref(other.raw)).error_code == inv
    # a stripe needs the whole height, and has to lie inside it
    assert lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(src.raw), C.byref(dst.raw), 4, 0).error_code == inv
    assert lib.uhdr_hip_resize_image_dev(hip_ctx.handle, C.byref(src.raw), C.byref(dst.raw), 4, 34).error_code == inv
