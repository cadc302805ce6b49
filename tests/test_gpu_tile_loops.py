"""GPU: the persistent tile loops of encode_api0_p010_fused_kernel, base_blocks_rgba_kernel, resize_image_kernel and
effect_remap_kernel past one item per walker.  The launchers cap their grids at what is resident (or at 16384 workgroups) and
every wave / workgroup walks `for (t = first; t < items; t += walkers)`; the shapes come from tests/tile_loop_shapes.py for
the compute-unit count of the device the test runs on, so that some walkers take a second trip and some do not, tiles_x is
neither 1 nor a power of two and each row ends in a ragged tile.  Every comparison is exact: against the staged operators
(P010, RGBA), tests/resize_port.py and row stripes below the cap (resize), the remap formulas of test_gpu_effects.py.  At the end of the
file the per-pixel routes of convertYuv, convert_raw_input_to_ycbcr, libjpeg's colour conversions and toneMap, against their vector routes."""
import ctypes as C
import functools

import numpy as np
import pytest

import framed as FR
import resize_cases as K
import resize_port as P
import route_lattice as RL
import test_gpu_api0_p010 as P0
import test_gpu_api1_rgba as R
import test_gpu_effects as E
import tile_loop_shapes as T
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FULL, LIMITED = A.UHDR_CR_FULL_RANGE, A.UHDR_CR_LIMITED_RANGE
P010, S420, Y400 = A.UHDR_IMG_FMT_24bppYCbCrP010, A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_8bppYCbCr400


@functools.lru_cache(maxsize=None)
def _loop(kernel):
    """The helper's shape for this device; NoSuchShape fails the test."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    loop = T.tile_loop(kernel, cus)
    print(f"{cus} compute units; {T.describe(loop)}")
    assert T.satisfies(loop)
    return loop


# ---- encode_api0_p010_fused_kernel ------------------------------------------------------------------------------------------------------
def _p010_calm_dark_head_bright_tail(w, h, ct, cg, rng_range, edge, seed):
    """A P010 image of mid codes (luma 400..519, chroma near neutral) whose first `edge` rows draw from darker codes and whose
    last `edge` rows from brighter ones: the gain grows with the luminance, so the smallest lives in the head and the largest in
    the tail.  No channel reaches zero, where the gain would sit at its clamp in many places at once.  Independent draws per
    sample, so a tile written to another tile's place shows.  Returns (image, the image without its head, the image without
    its tail)."""
    rng = np.random.default_rng(seed)
    y = rng.integers(400, 520, (h, w), dtype=np.uint16)
    c = rng.integers(490, 534, (h // 2, w), dtype=np.uint16)
    dark, bright = rng.integers(160, 400, (edge, w), dtype=np.uint16), rng.integers(520, 941, (edge, w), dtype=np.uint16)
    out = []
    for head, tail in ((True, True), (False, True), (True, False)):
        yy, cc = y.copy(), c.copy()
        if head:
            yy[:edge] = dark
        if tail:
            yy[-edge:] = bright
        img = Image(P010, w, h, cg, ct, rng_range, 64)
        img.valid(0)[:] = yy << 6
        img.valid(1)[:] = cc << 6
        out.append(img)
    return out


@pytest.mark.parametrize("kernel,ct,cg,rng_range,cfg_kw", [
    ("p010_two_pass", A.UHDR_CT_HLG, A.UHDR_CG_BT_2100, LIMITED, dict(preset=A.UHDR_USAGE_BEST_QUALITY)),
    ("p010_one_pass", A.UHDR_CT_PQ, A.UHDR_CG_BT_709, FULL, dict(preset=A.UHDR_USAGE_REALTIME, use_multi_channel_gainmap=0))])
def test_p010_fused_front_end_on_the_second_trip(hip_ctx, kernel, ct, cg, rng_range, cfg_kw):
    """encodeApi0FusedP010 == toneMap -> generateGainMap, bit for bit, where a wave walks two tiles and the row of a tile comes from
    the float estimate of t / 3 for t in the thousands.  Two pass: the smallest gain sits in tiles that are the first of two trips
    and the largest in tiles that only second trips reach, so a wave that carried its accumulators over wrongly in either
    direction would report another range -- the metadata would differ."""
    loop = _loop(kernel)
    w, h, edge = loop.w, loop.h, 32
    # quad rows: the head's tiles have indices below items - walkers (their waves come round again), the tail's at least walkers
    assert (edge // 2) * loop.tiles_x <= loop.items - loop.walkers and (h - edge) // 2 * loop.tiles_x >= loop.walkers
    hdr, no_head, no_tail = _p010_calm_dark_head_bright_tail(w, h, ct, cg, rng_range, edge, seed=loop.items)
    cfg = A.default_encode_cfg(use_luminance=0, **cfg_kw)
    u = P0._uhdr_for(hip_ctx, cfg)
    dh = hdr.to(DEV)
    base_f, md_f, gm_f = u.encodeApi0FusedP010(dh)
    hip_ctx.synchronize()
    base_s, md_s, gm_s = P0._staged(u, dh)
    hip_ctx.synchronize()
    assert P0.planes_equal(base_f, base_s), "base image planes"
    assert P0.planes_equal(gm_f, gm_s), "gain map"
    assert md_f.as_dict() == md_s.as_dict()
    assert P0._desc(base_f) == P0._desc(base_s) and P0._desc(gm_f) == P0._desc(gm_s)
    assert gm_f.raw.fmt == (A.UHDR_IMG_FMT_24bppRGB888 if cfg.use_multi_channel_gainmap else A.UHDR_IMG_FMT_8bppYCbCr400)
    if kernel == "p010_two_pass":  # the head and the tail are what set the range: the staged route reports another one without either
        md_no_head, md_no_tail = P0._staged(u, no_head.to(DEV))[1], P0._staged(u, no_tail.to(DEV))[1]
        hip_ctx.synchronize()
        print("min / max content boost:", list(md_s.min_content_boost), list(md_s.max_content_boost), "without the head:",
              list(md_no_head.min_content_boost), "without the tail:", list(md_no_tail.max_content_boost))
        assert all(a > b for a, b in zip(md_no_head.min_content_boost, md_s.min_content_boost)), "the head does not hold the smallest gain"
        assert all(a < b for a, b in zip(md_no_tail.max_content_boost, md_s.max_content_boost)), "the tail does not hold the largest gain"


# ---- base_blocks_rgba_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [True, False], ids=["pitch-16B", "pitch-odd"])
def test_rgba_base_launch_on_the_second_trip(hip_ctx, vec):
    """encodeApi1FusedAny on an RGBA8888 intent of random bytes == convert_raw_input_to_ycbcr + convertYuv + fdct_quant x 3 where a
    wave owns two strips, i.e. uses its LDS workspace six times: all coefficients, the map and the metadata.  Once with rows on
    16-byte boundaries (two 16-byte loads per lane) and once with a pitch that is no multiple of 4 pixels (dword loads)."""
    import torch

    loop = _loop("rgba")
    w, h = loop.w, loop.h
    align = 64 if vec else next(a for a in (3, 5, 7) if (-(-w // a) * a) % 4)
    rng = np.random.default_rng(loop.items + align)
    sdr = Image(R.RGBA, w, h, R.BT709, A.UHDR_CT_SRGB, FULL, align)
    sdr.buf[:] = rng.integers(0, 256, sdr.buf.size, dtype=np.uint8)
    assert ((sdr.raw.stride[0] * 4) % 16 == 0) == vec and (vec or sdr.raw.stride[0] % 4 != 0)
    hdr = Image(A.UHDR_IMG_FMT_32bppRGBA1010102, w, h, R.BT2100, A.UHDR_CT_PQ, FULL, 64)
    hdr.buf[:] = rng.integers(0, 256, hdr.buf.size, dtype=np.uint8)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    assert (ds.raw.planes[0] % 16 == 0) or not vec
    u = R._uhdr(hip_ctx)
    qb, qm = R._tables()
    base_f, map_f, md_f, gm_f = u.encodeApi1FusedAny(ds, dh, R.P3, qb, qm, want_map=True)
    hip_ctx.synchronize()
    assert [tuple(b.shape) for b in base_f] == [(h // 8, w // 8, 64)] * 3
    base_s, map_s, md_s, gm_s = R._staged(hip_ctx, u, ds, dh, R.P3, qb, qm)
    for i in range(3):
        assert torch.equal(base_f[i], base_s[i].reshape(base_f[i].shape)), f"base component {i}"
    R._assert_blocks_equal(map_f, map_s, "map")
    assert md_f.as_dict() == md_s.as_dict()
    assert R._planes_equal(gm_f, gm_s), "8-bit map"


# ---- resize_image_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ["y400", "rgba8888"])
def test_resize_image_past_the_grid_cap(hip_ctx, fmt_name):
    """resizeImage of a 64 x 48 map to a destination of more than 16384 tiles.  Against tests/resize_port.py on three bands of 32
    rows -- the first, the one in which tile 16384 (the first second trip) lies, the last -- and on the whole image for Y400, where
    the port is quick; and every row against the same destination made of row stripes that stay below 16384 tiles each."""
    from libultrahdr_amd.ultrahdr import UltraHdr

    loop = _loop("resize")
    dw, dh = loop.w, loop.h
    fmt = K.FORMATS[fmt_name]
    src = K.make_map(fmt, 64, 48, "random", align=24)
    sch = P.channels_of(src)
    u = UltraHdr(ctx=hip_ctx)
    dsrc = src.to(DEV)
    whole = u.resizeImage(dsrc, dw, dh)
    hip_ctx.synchronize()
    got = whole.to_host()
    gch = P.channels_of(got)
    turn = 16384 // loop.tiles_x
    assert 16 <= turn < dh - 48
    for y0 in (0, turn - 16, dh - 32):
        want = P.resize_channels(sch, fmt, dw, dh, y0, 32)
        assert np.array_equal(gch[y0: y0 + 32], want), f"rows {y0}..{y0 + 32}: {(gch[y0: y0 + 32] != want).sum()} bytes differ from the port"
    if fmt == K.Y400:
        want = P.resize_channels(sch, fmt, dw, dh)
        assert np.array_equal(gch, want), f"{(gch != want).sum()} bytes differ from the port"
    else:
        assert np.all(got.valid(0) >> 24 == 255)
    rows_per = 2048
    assert T.resize_walk(dw, rows_per)[1] < 16384
    for y0 in range(0, dh, rows_per):
        rows = min(rows_per, dh - y0)
        stripe = Image(fmt, dw, rows, align=64, device=DEV, fill=0x33)
        u.resizeImage(dsrc, dw, rows, stripe, y0, dh)
        hip_ctx.synchronize()
        assert np.array_equal(stripe.to_host().valid(0), got.valid(0)[y0: y0 + rows]), f"rows {y0}..{y0 + rows} differ from their stripe"


# ---- effect_remap_kernel ----------------------------------------------------------------------------------------------------------------
def _random_image(fmt, w, h, seed):
    img = Image(fmt, w, h, align=64)
    img.buf[:] = np.random.default_rng(seed).integers(0, 256, img.buf.size, dtype=np.uint8)
    return img


def _check_effects(hip_ctx, src, cases):
    """uhdr_hip_apply_effect_dev on `src` for every (effect, p0, p1, dw, dh) against _remap of test_gpu_effects.py, plane by plane."""
    fmt, dsrc = src.fmt, src.to(DEV)
    for (effect, p0, p1, dw, dh) in cases:
        dst = Image(fmt, dw, dh, align=64, device=DEV, fill=0x33)
        A.check(hip_ctx.lib.uhdr_hip_apply_effect_dev(hip_ctx.handle, effect, p0, p1, C.byref(dsrc.raw), C.byref(dst.raw)))
        hip_ctx.synchronize()
        got = dst.to_host()
        for c in range(len(src.layout)):
            if src.layout[c] is None:
                continue
            div = 2 if c > 0 and fmt in (P010, S420) else 1  # chroma planes: half size (crop origins are halved, editorhelper.cpp:375, 385)
            want = E._remap(E._elements(src, c), effect, p0 // div if effect == 2 else p0, p1 // div if effect == 2 else p1, dw // div, dh // div)
            assert np.array_equal(E._elements(got, c), want), (fmt, src.w, src.h, effect, p0, p1, dw, dh, c)


@pytest.mark.parametrize("fmt", E.FMTS)
def test_effects_with_three_tiles_per_row(hip_ctx, fmt):
    """A 520 x 36 source: destinations of 520 (516) elements are three tiles per row with a ragged last one, two for the chroma
    planes of the subsampled formats; all seven modes.  Then a 40 x 24 source: a crop whose origin has odd halves, and resizes to
    a larger destination, where src / dst is 0 and resize_buffer (editorhelper.cpp:78-86) repeats element (0, 0) along that axis."""
    w, h = 520, 36
    assert T.effect_walk(w, h)[0] == 3 and T.effect_walk(516, 32)[0] == 3 and T.effect_walk(w // 2, h // 2)[0] == 2
    _check_effects(hip_ctx, _random_image(fmt, w, h, 520 + fmt),
                   [(0, 90, 0, h, w), (0, 180, 0, w, h), (0, 270, 0, h, w), (1, 0, 0, w, h), (1, 1, 0, w, h), (2, 4, 2, 516, 32), (3, 0, 0, w, h), (3, 0, 0, 260, 18)])
    _check_effects(hip_ctx, _random_image(fmt, 40, 24, 40 + fmt), [(2, 6, 10, 24, 12), (3, 0, 0, 96, 64), (3, 0, 0, 96, 12), (3, 0, 0, 20, 64)])


@pytest.mark.parametrize("fmt", [Y400, S420])
def test_effects_past_the_grid_cap(hip_ctx, fmt):
    """Destinations of more than 16384 tiles with three tiles per row: rotate 180, both mirrors, a crop with a non-zero origin and a
    2:1 resize (horizontally: the source stays within 8192 rows); and a rotation by 90 degrees of a 4100 x 1030 source, whose
    destination has five tiles per row."""
    loop = _loop("effects")
    dw, dh = loop.w, loop.h
    _check_effects(hip_ctx, _random_image(fmt, dw, dh, 1 + fmt), [(0, 180, 0, dw, dh), (1, 0, 0, dw, dh), (1, 1, 0, dw, dh)])
    _check_effects(hip_ctx, _random_image(fmt, dw + 16, dh + 12, 2 + fmt), [(2, 10, 6, dw, dh)])
    _check_effects(hip_ctx, _random_image(fmt, 2 * dw, dh, 3 + fmt), [(3, 0, 0, dw, dh)])
    tiles_x, tiles, walkers = T.effect_walk(1030, 4100)
    assert tiles_x == 5 and tiles > walkers == 16384
    _check_effects(hip_ctx, _random_image(fmt, 4100, 1030, 4 + fmt), [(0, 90, 0, 1030, 4100)])


# ---- the per-pixel routes of the oldest launchers (tests/route_lattice.py) ------------------------------------------------------------------
# Each operator once on a view with odd strides and bases inside a 0xA5 frame (tests/framed.py), which forces its per-pixel kernel, at
# the shape where that kernel's workgroups (waves) come round again -- and once on an aligned copy of the same samples, which its
# vector route takes.  The two outputs are equal byte for byte; the integer operators equal the oracle as well.
def _odd(fmt, w, sample_bytes=1):
    """(strides, offsets) of a view no vector route takes: odd strides, bases off every alignment the sample size allows."""
    n = len(FR.plane_samples(fmt, w, 2))
    widths = [pw for _, pw in FR.plane_samples(fmt, w, 2)]
    return [pw + 3 - pw % 2 for pw in widths], [sample_bytes * (1 + 2 * (i % 2)) for i in range(n)]


def _aligned(fmt, w):
    widths = [pw for _, pw in FR.plane_samples(fmt, w, 2)]
    return [-(-pw // 64) * 64 for pw in widths], [0] * len(widths)


def _random_bytes(fmt, w, h, seed, cg=A.UHDR_CG_BT_709, ct=A.UHDR_CT_SRGB):
    img = Image(fmt, w, h, cg, ct, FULL, align=2)
    img.buf[:] = np.random.default_rng(seed).integers(0, 256, img.buf.size, dtype=np.uint8)
    return img


def _planes_same(got, want, what):
    for i, (g, w_) in enumerate(zip(got, want)):
        if not np.array_equal(g, w_):
            ys, xs = np.nonzero(np.asarray(g) != np.asarray(w_))
            raise AssertionError(f"{what}: plane {i}: {ys.size} samples differ, the first at row {ys[0]}, column {xs[0]}")


@pytest.mark.parametrize("kernel,fmt", [("yuv420", S420), ("yuv444", A.UHDR_IMG_FMT_24bppYCbCr444)])
def test_convert_yuv_narrow_route_on_the_second_trip(hip_ctx, kernel, fmt):
    loop = _loop(kernel)
    w, h = loop.w, loop.h
    src = _random_bytes(fmt, w, h, loop.items)
    enc = (A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100)
    outs = []
    for strides, offsets in (_odd(fmt, w), _aligned(fmt, w)):
        case = RL.Case("transform_yuv", kernel, w, h, RL.Layout(fmt, tuple(strides), tuple(offsets)), None, None, {})
        outs.append(RL.route(case))
        fr = FR.framed(fmt, w, h, strides, offsets, src=src, device=DEV)
        A.check(hip_ctx.lib.uhdr_hip_convert_yuv_dev(hip_ctx.handle, C.byref(fr.raw), *enc))
        hip_ctx.synchronize()
        FR.assert_frame_intact(fr, what=f"{kernel} {outs[-1]}")
        outs.append(fr.valid())
    assert outs[0] == (f"transform_{kernel}_kernel",) and outs[2] == (f"transform_{kernel}_wide_kernel",)
    _planes_same(outs[1], outs[3], f"{kernel}: the per-pixel route against the vector route")
    _planes_same(outs[1], L.convert_yuv(P0.oracle_kind(), src, *enc).planes_valid(), f"{kernel}: against the oracle")


@pytest.mark.parametrize("kernel,src_fmt,dst_fmt", [("rgb420", R.RGBA, S420), ("rgb444", A.UHDR_IMG_FMT_32bppRGBA1010102, A.UHDR_IMG_FMT_30bppYCbCr444)])
def test_convert_raw_input_narrow_route_on_the_second_trip(hip_ctx, kernel, src_fmt, dst_fmt):
    loop = _loop(kernel)
    w, h = loop.w, loop.h
    ten = dst_fmt == A.UHDR_IMG_FMT_30bppYCbCr444
    src = _random_bytes(src_fmt, w, h, loop.items, cg=A.UHDR_CG_DISPLAY_P3)
    outs = []
    for lay in (_odd, _aligned):
        (ss, so), (ds, do) = (lay(src_fmt, w, 4), lay(dst_fmt, w, 2 if ten else 1)) if lay is _odd else (lay(src_fmt, w), lay(dst_fmt, w))
        case = RL.Case("rgb_to_ycbcr", kernel, w, h, RL.Layout(src_fmt, tuple(ss), tuple(so)), RL.Layout(dst_fmt, tuple(ds), tuple(do)), None, {})
        outs.append(RL.route(case))
        sfr, dfr = FR.framed(src_fmt, w, h, ss, so, src=src, device=DEV), FR.framed(dst_fmt, w, h, ds, do, device=DEV)
        A.check(hip_ctx.lib.uhdr_hip_convert_raw_input_to_ycbcr_dev(hip_ctx.handle, C.byref(sfr.raw), int(not ten), C.byref(dfr.raw)))
        hip_ctx.synchronize()
        FR.assert_frame_intact(dfr, what=f"{kernel} {outs[-1]}")
        FR.assert_frame_intact(sfr, written=(), what=f"{kernel} source")
        outs.append(dfr.valid())
    t = "true" if ten else "false"
    assert outs[0] == (f"rgb_to_ycbcr{kernel[3:]}_kernel<{t}>",) and outs[2] == (f"rgb_to_ycbcr{kernel[3:]}_wide_kernel<{t}>",)
    _planes_same(outs[1], outs[3], f"{kernel}: the per-pixel route against the vector route")
    _planes_same(outs[1], L.convert_raw_input_to_ycbcr(P0.oracle_kind(), src, not ten).planes_valid(), f"{kernel}: against the oracle")


@pytest.mark.parametrize("direction,rgb_fmt", [("rgb_to_ycc", A.UHDR_IMG_FMT_24bppRGB888), ("ycc_to_rgb", R.RGBA)])
def test_jpeg_colour_narrow_route_on_the_second_trip(hip_ctx, direction, rgb_fmt):
    loop = _loop("jpeg_colour")
    w, h = loop.w, loop.h
    ycc_fmt = A.UHDR_IMG_FMT_24bppYCbCr444
    src_fmt, dst_fmt = (rgb_fmt, ycc_fmt) if direction == "rgb_to_ycc" else (ycc_fmt, rgb_fmt)
    src = _random_bytes(src_fmt, w, h, loop.items)
    outs = []
    for lay in (_odd, _aligned):
        (ss, so), (ds, do) = lay(src_fmt, w), lay(dst_fmt, w)
        if lay is _odd and rgb_fmt == R.RGBA:  # pixels stay on 4-byte boundaries
            do = [4]
        case = RL.Case("jpeg_" + direction, direction, w, h, RL.Layout(src_fmt, tuple(ss), tuple(so)), RL.Layout(dst_fmt, tuple(ds), tuple(do)), None, {})
        outs.append(RL.route(case))
        sfr, dfr = FR.framed(src_fmt, w, h, ss, so, src=src, device=DEV), FR.framed(dst_fmt, w, h, ds, do, device=DEV)
        if direction == "rgb_to_ycc":
            A.check(hip_ctx.lib.uhdr_hip_jpeg_rgb_to_ycc_dev(hip_ctx.handle, C.byref(sfr.raw), C.byref(dfr.raw)))
        else:
            A.check(hip_ctx.lib.uhdr_hip_jpeg_ycc_to_rgb_dev(hip_ctx.handle, C.byref(sfr.raw), 0, C.byref(dfr.raw)))
        hip_ctx.synchronize()
        FR.assert_frame_intact(dfr, what=f"{direction} {outs[-1]}")
        FR.assert_frame_intact(sfr, written=(), what=f"{direction} source")
        outs.append([p.view(np.uint8) for p in dfr.valid()])
    bpp = 4 if rgb_fmt == R.RGBA else 3
    assert outs[0] == (f"jpeg_{direction}_kernel<{bpp}, false>",) and outs[2] == (f"jpeg_{direction}_kernel<{bpp}, true>",)
    _planes_same(outs[1], outs[3], f"{direction}: the per-pixel route against the vector route")
    if direction == "rgb_to_ycc":
        want = L.jpeg_rgb_to_ycc_port(np.ascontiguousarray(src.valid(0)), w, w, h)
    else:
        want = [L.jpeg_ycc_to_rgb_port(src.valid(0), src.valid(1), src.valid(2), out_bpp=4, variant=0)]
    _planes_same(outs[1], want, f"{direction}: against the oracle")


def _legal_p010(w, h, ct, cg, seed):
    """Independent random codes of the limited range in every sample of a P010 image."""
    rng = np.random.default_rng(seed)
    img = Image(P010, w, h, cg, ct, LIMITED, 2)
    img.valid(0)[:] = rng.integers(64, 941, (h, w), dtype=np.uint16) << 6
    img.valid(1)[:] = rng.integers(64, 961, (h // 2, w), dtype=np.uint16) << 6
    return img


@pytest.mark.parametrize("kernel", ["tone_p010", "tone_pixel"])
def test_tone_map_narrow_routes_on_the_second_trip(hip_ctx, kernel):
    """tonemap_p010_kernel with per-pixel loads and byte luma stores against its quad loads and 16-bit stores; tonemap_pixel_kernel, which
    has one route, on the odd view against the aligned one -- and, being the only check of its loop, against the oracle at the bar of
    tests/test_gpu_formats.py (+-1 code on <= 1e-4 of the samples)."""
    loop = _loop(kernel)
    w, h = loop.w, loop.h
    if kernel == "tone_p010":
        src_fmt, dst_fmt, sb = P010, S420, 2
        hdr = _legal_p010(w, h, A.UHDR_CT_HLG, A.UHDR_CG_BT_2100, loop.items)
    else:
        src_fmt, dst_fmt, sb = A.UHDR_IMG_FMT_32bppRGBA1010102, R.RGBA, 4
        hdr = _random_bytes(src_fmt, w, h, loop.items, cg=A.UHDR_CG_BT_2100, ct=A.UHDR_CT_PQ)
    outs = []
    for lay in (_odd, _aligned):
        (ss, so), (ds, do) = (lay(src_fmt, w, sb), lay(dst_fmt, w, 4 if dst_fmt == R.RGBA else 1)) if lay is _odd else (lay(src_fmt, w), lay(dst_fmt, w))
        case = RL.Case("tone_map", kernel, w, h, RL.Layout(src_fmt, tuple(ss), tuple(so)), RL.Layout(dst_fmt, tuple(ds), tuple(do)), None,
                       dict(ct=hdr.raw.ct, cg=hdr.raw.cg))
        outs.append(RL.route(case))
        hfr, sfr = FR.framed(src_fmt, w, h, ss, so, src=hdr, device=DEV), FR.framed(dst_fmt, w, h, ds, do, device=DEV)
        A.check(hip_ctx.lib.uhdr_hip_tone_map_dev(hip_ctx.handle, C.byref(hfr.raw), C.byref(sfr.raw)))
        hip_ctx.synchronize()
        FR.assert_frame_intact(sfr, what=f"{kernel} {outs[-1]}")
        FR.assert_frame_intact(hfr, written=(), what=f"{kernel} hdr intent")
        outs.append([p.view(np.uint8) for p in sfr.valid()])
    if kernel == "tone_p010":
        assert outs[0][1:] == ("p010: pixel loads", "p010: byte luma stores") and outs[2][1:] == ("p010: quad loads", "p010: 16-bit luma store")
    _planes_same(outs[1], outs[3], f"{kernel}: the odd view against the aligned one")
    if kernel == "tone_pixel":
        import test_gpu_formats as TF

        want = L.tone_map(P0.oracle_kind(), hdr)
        TF.assert_close_codes(outs[1][0], want.valid(0).view(np.uint8), 1e-4, "tone_pixel against the oracle")
