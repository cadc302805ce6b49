"""GPU: the persistent tile loops of encode_api0_p010_fused_kernel, base_blocks_rgba_kernel, resize_image_kernel and
effect_remap_kernel past one item per walker.  The launchers cap their grids at what is resident (or at 16384 workgroups) and
every wave / workgroup walks `for (t = first; t < items; t += walkers)`; the shapes come from tests/tile_loop_shapes.py for
the compute-unit count of the device the test runs on, so that some walkers take a second trip and some do not, tiles_x is
neither 1 nor a power of two and each row ends in a ragged tile.  Every comparison is exact: against the staged operators
(P010, RGBA), tests/resize_port.py and row stripes below the cap (resize), the remap formulas of test_gpu_effects.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_cases as K
import resize_port as P
import test_gpu_api0_p010 as P0
import test_gpu_api1_rgba as R
import test_gpu_effects as E
import tile_loop_shapes as T
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image

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
