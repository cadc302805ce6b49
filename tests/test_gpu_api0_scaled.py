"""GPU: the fused API-0 front ends at gain-map scale factors 2 and 4 (uhdr_hip_encode_api0_fused_scaled_dev for RGBA1010102 intents,
uhdr_hip_encode_api0_p010_fused_scaled_dev for P010) and the one-call form (uhdr_hip_encode_api0_scans_scaled).  The yardstick is the
staged route through the device operators with the same configuration -- toneMap, generateGainMap(sdr, hdr, False, False) and, for RGB
intents, convert_raw_input_to_ycbcr; per-plane FDCT and the two-scan Huffman coder behind them --, which are held to the reference
elsewhere (tests/test_gpu_parity.py holds the generic generate kernel to the oracle at scales 2, 3 and 4).  Equality is exact.

Tile widths.  RGBA1010102: a lane owns 4 pixels x S rows, a wave tile is 64 cells = 256 pixels of one strip of S rows.  P010: a lane owns
an S x S box, a wave tile is 64 boxes = 64 * S pixels (128 at S = 2, 256 at S = 4) of one box row.  So
  4 x 4      a single cell: one map pixel at S = 4, four at S = 2 (P010 at S = 2: four lanes);
  264 x 12   RGBA: a full tile + 2 ragged cells, three (S = 4) and six (S = 2) strips; P010: two tiles + 4 boxes (S = 2), one + 2 (S = 4);
  260 x 8    RGBA and P010 at S = 4: one cell / box past a full tile; P010 at S = 2: two boxes past two tiles."""
import ctypes as C

import numpy as np
import pytest

import code_lattice as CL
import tile_loop_shapes as T
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L
from test_gpu_api0_p010 import PAIRS, _uhdr_for  # the four transfer / gamut pairs: the three gamut modes and a linear intent with no table

pytestmark = pytest.mark.gpu

RGBA, P010 = A.UHDR_IMG_FMT_32bppRGBA1010102, A.UHDR_IMG_FMT_24bppYCbCrP010
FMTS = [RGBA, P010]
SCALES = [2, 4]
# one channel, three channels, a gamma (no gain step table: encode_gain per map pixel), a target display peak (metadata only)
CONFIGS = [dict(use_multi_channel_gainmap=0), dict(use_multi_channel_gainmap=1), dict(use_multi_channel_gainmap=1, gamma=1.3),
           dict(use_multi_channel_gainmap=0, target_disp_peak_nits=1000.0)]
SHAPES = [(4, 4), (264, 12), (260, 8)]


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def _cfg(scale, **kw):
    return A.default_encode_cfg(use_luminance=0, preset=A.UHDR_USAGE_REALTIME, map_dimension_scale_factor=scale, **kw)


def _make(fmt, w, h, ct, cg, rng, seed=None, align=64):
    seed = w * 7 + h if seed is None else seed
    if fmt == P010:
        return synth.make_hdr_p010(w, h, seed=seed, ct=ct, cg=cg, noise=0.05, rng_range=rng, align=align)
    return synth.make_hdr_rgba1010102(w, h, seed=seed, ct=ct, cg=cg, noise=0.05, align=align)


def _staged(u, dh):
    """(RGBA8888 rendition or None, base image, metadata, map) from the staged device operators, as JpegR::encodeJPEGR API-0 calls them."""
    if dh.fmt == P010:
        sdr = Image(A.UHDR_IMG_FMT_12bppYCbCr420, dh.w, dh.h, align=64, device="cuda:0")
        u.toneMap(dh, sdr)
        md, gm = u.generateGainMap(sdr, dh, False, False)
        return None, sdr, md, gm
    sdr = Image(A.UHDR_IMG_FMT_32bppRGBA8888, dh.w, dh.h, align=64, device="cuda:0")
    u.toneMap(dh, sdr)
    md, gm = u.generateGainMap(sdr, dh, False, False)
    ycc = u.convert_raw_input_to_ycbcr(sdr, False)
    return sdr, ycc, md, gm


def _fused(u, dh, **kw):
    if dh.fmt == P010:
        base, md, gm = u.encodeApi0FusedP010Scaled(dh, **kw)
        return None, base, md, gm
    return u.encodeApi0FusedScaled(dh, **kw)


def _desc(img):
    return (img.raw.fmt, img.raw.cg, img.raw.ct, img.raw.range, img.raw.w, img.raw.h)


def planes_equal(a: Image, b: Image):
    pa, pb = a.to_host().planes_valid(), b.to_host().planes_valid()
    return len(pa) == len(pb) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(pa, pb))


def assert_same(fused, staged, what=""):
    """The base planes, the optional RGBA8888 rendition, the map, the metadata and the descriptors: exact."""
    (sdr_f, base_f, md_f, gm_f), (sdr_s, base_s, md_s, gm_s) = fused, staged
    assert planes_equal(base_f, base_s), f"base image planes {what}"
    assert planes_equal(gm_f, gm_s), f"gain map {what}"
    assert md_f.as_dict() == md_s.as_dict(), what
    assert _desc(base_f) == _desc(base_s) and _desc(gm_f) == _desc(gm_s), what
    if sdr_f is not None:
        assert planes_equal(sdr_f, sdr_s), f"RGBA8888 rendition {what}"
        assert _desc(sdr_f) == _desc(sdr_s), what


def assert_close_codes(got, want, max_code_diff, max_frac, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    frac = (d != 0).mean()
    print(f"{what}: max code diff {d.max()}, {frac:.4%} of samples differ (allowed {max_frac:.2%})")
    assert d.max() <= max_code_diff, f"{what}: max code diff {d.max()}"
    assert frac <= max_frac, f"{what}: {frac:.4%} of samples differ (allowed {max_frac:.2%})"


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("ct,cg,rng", PAIRS)
@pytest.mark.parametrize("cfg_kw", CONFIGS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_front_end_equals_the_staged_operators(hip_ctx, fmt, scale, cfg_kw, ct, cg, rng, w, h):
    u = _uhdr_for(hip_ctx, _cfg(scale, **cfg_kw))
    dh = _make(fmt, w, h, ct, cg, rng).to("cuda:0")
    fused = _fused(u, dh)
    hip_ctx.synchronize()
    staged = _staged(u, dh)
    hip_ctx.synchronize()
    assert_same(fused, staged)
    assert (fused[3].w, fused[3].h) == (w // scale, h // scale)
    if fmt == RGBA:  # without the optional rendition
        lean = u.encodeApi0FusedScaled(dh, want_sdr_rgba=False)
        hip_ctx.synchronize()
        assert lean[0] is None
        assert_same(lean, staged, "without the rendition")


# ---- the second trip of the tile loop ------------------------------------------------------------------------------------------------
def scaled_walk(cus, fmt, scale, w, h):
    """(tiles_x, items, walkers) of the scaled kernels; a walker is a wave.  Restates launch_encode_api0_fused_scaled /
    launch_encode_api0_p010_fused_scaled and scaled_grid of encode_fused.hip."""
    cells = w // 4 if fmt == RGBA else w // scale  # const uint32_t w4 = p.tm.hdr.w / 4 | bw = p.tm.hdr.w / S
    tiles_x = (cells + 63) // 64                   # const uint32_t tiles_x = (w4 + 63) / 64, tiles = tiles_x * strips;
    wave_tiles = tiles_x * (h // scale)            # scaled_grid(((w / 4 + 63) / 64) * (h / S)) | (((w / S + 63) / 64) * (h / S))
    wg_waves = 512 // 64                           # constexpr int kScaledBlock = 512;
    grid = T.fused_grid(cus, -(-wave_tiles // wg_waves), 2)  # fused_grid((wave_tiles + wg_waves - 1) / wg_waves, 2)
    return tiles_x, wave_tiles, grid * wg_waves    # nwaves = gridDim.x * (kScaledBlock / 64)


def second_trip_shape(cus, fmt, scale):
    """The rule of tests/tile_loop_shapes.py: within 8192 x 8192, an item count strictly between 1.25 x and 2.5 x the walkers, tiles_x >= 3
    and not a power of two, a ragged last tile; the smallest such tiles_x, then the smallest height."""
    cell_w = 4 if fmt == RGBA else scale
    for tx in range(3, T.MAX_DIM):
        w = cell_w * ((tx - 1) * 64 + (2 if cell_w == 2 else 1))  # (a width that is a multiple of 4)
        if w > T.MAX_DIM:
            break
        if tx & (tx - 1) == 0:
            continue
        for rows in range(1, T.MAX_DIM // scale + 1):
            loop = T.TileLoop(f"scaled-{fmt}-{scale}", w, rows * scale, *scaled_walk(cus, fmt, scale, w, rows * scale))
            if T.satisfies(loop):
                return loop
    raise T.NoSuchShape(f"scale {scale}, format {fmt}: no shape within {T.MAX_DIM} x {T.MAX_DIM} for {cus} compute units")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_front_end_on_the_second_trip_of_its_tile_loop(hip_ctx, fmt, scale):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    loop = second_trip_shape(cus, fmt, scale)  # NoSuchShape fails the test
    print(f"{cus} compute units; {T.describe(loop)}")
    assert loop.w % 4 == 0 and loop.h % scale == 0 and loop.items > loop.walkers
    ct, cg, rng = PAIRS[0]
    u = _uhdr_for(hip_ctx, _cfg(scale, use_multi_channel_gainmap=1))
    dh = _make(fmt, loop.w, loop.h, ct, cg, rng, seed=11).to("cuda:0")
    fused = _fused(u, dh)
    hip_ctx.synchronize()
    staged = _staged(u, dh)
    hip_ctx.synchronize()
    assert_same(fused, staged)


# ---- the code lattice ----------------------------------------------------------------------------------------------------------------
FULL, LIMITED = A.UHDR_CR_FULL_RANGE, A.UHDR_CR_LIMITED_RANGE
LATTICE_IMAGES = ([(CL.H1010102, FULL, ct, cg) for ct in (CL.HLG, CL.PQ, CL.LINEAR) for cg in (CL.BT2100, CL.P3, CL.BT709)] +
                  [(CL.HP010, rng, ct, cg) for rng in (LIMITED, FULL) for ct in (CL.HLG, CL.PQ, CL.LINEAR) for cg in (CL.BT2100, CL.P3, CL.BT709)])


@pytest.mark.parametrize("fmt,rng,ct,cg", LATTICE_IMAGES)
def test_scaled_front_end_on_the_code_lattice(hip_ctx, fmt, rng, ct, cg):
    """The RGBA1010102 and the P010 lattice image of tests/code_lattice.py (every code of every channel, the ends of the code range, the
    limited-range bounds and their outsides) at SIZE_MAIN through every configuration and both scale factors: equal to the staged route."""
    w, h = CL.SIZE_MAIN
    dh = CL.hdr(fmt, w, h, ct=ct, cg=cg, rng_range=rng).to("cuda:0")
    for scale in SCALES:
        for cfg_kw in CONFIGS:
            u = _uhdr_for(hip_ctx, _cfg(scale, **cfg_kw))
            fused = _fused(u, dh)
            hip_ctx.synchronize()
            staged = _staged(u, dh)
            hip_ctx.synchronize()
            assert_same(fused, staged, f"scale {scale}, {cfg_kw}")


# ---- caller-provided images ----------------------------------------------------------------------------------------------------------
def _untouched_outside(img: Image, fill=0xA5):
    """Every byte of the image's allocation that no row's width covers still holds `fill`."""
    got = img.to_host()
    mask = Image(img.fmt, img.w, img.h, align=img.align)
    for i, pl in enumerate(mask.layout):
        if pl is not None:
            v = mask.valid(i)
            v[...] = np.iinfo(v.dtype).max
    outside = got.buf[mask.buf == 0]
    return bool((outside == fill).all())


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_front_end_into_caller_images(hip_ctx, fmt, scale, pad):
    """0xA5-filled images for the base, the map and the rendition whose rows are not padded to 64 samples.  pad == False: the smallest
    alignment the entry point accepts (strides that are multiples of 4 for the RGB planes and the rendition, of 2 for 4:2:0 luma, any for
    the map: the rows touch); pad == True: rows padded to 8 samples, whose padding must survive."""
    w, h = 260, 8
    ct, cg, rng = PAIRS[0]
    u = _uhdr_for(hip_ctx, _cfg(scale, use_multi_channel_gainmap=1))
    dh = _make(fmt, w, h, ct, cg, rng, seed=5, align=2 if fmt == P010 else 4).to("cuda:0")
    a_base, a_map = (8, 8) if pad else ((2 if fmt == P010 else 4), 1)
    gm = Image(A.UHDR_IMG_FMT_24bppRGB888, w // scale, h // scale, align=a_map, device="cuda:0", fill=0xA5)
    if fmt == P010:
        base = Image(A.UHDR_IMG_FMT_12bppYCbCr420, w, h, align=a_base, device="cuda:0", fill=0xA5)
        fused = _fused(u, dh, base=base, gm=gm)
        images = [base, gm]
    else:
        base = Image(A.UHDR_IMG_FMT_24bppYCbCr444, w, h, align=a_base, device="cuda:0", fill=0xA5)
        sdr = Image(A.UHDR_IMG_FMT_32bppRGBA8888, w, h, align=a_base, device="cuda:0", fill=0xA5)
        fused = _fused(u, dh, sdr=sdr, ycc=base, gm=gm)
        images = [base, gm, sdr]
    hip_ctx.synchronize()
    staged = _staged(u, dh)
    hip_ctx.synchronize()
    assert_same(fused, staged)
    if pad:
        assert base.raw.stride[0] > w and gm.raw.stride[0] > w // scale
    for img in images:
        assert _untouched_outside(img), f"format {img.fmt}: a byte behind a row's width was written"


# ---- against the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,cg,rng", PAIRS)
@pytest.mark.parametrize("cfg_kw", CONFIGS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_scaled_front_end_against_the_oracle(hip_ctx, fmt, scale, cfg_kw, ct, cg, rng):
    """The project's own bars (test_fused_api0_front_end_equals_the_three_operators, test_gpu_api0_p010.py): the SDR bytes within one code
    of the oracle's tone_map on at most 1e-4 of the samples; the map within one code on at most 1e-4 of the samples (5e-3 where gamma != 1)
    of the oracle's generate_gainmap run on the FUSED SDR image itself, downloaded, and the HDR intent -- every map pixel is compared,
    whatever the SDR bytes did."""
    w, h = 264, 12
    hdr = _make(fmt, w, h, ct, cg, rng)
    cfg = _cfg(scale, **cfg_kw)
    u = _uhdr_for(hip_ctx, cfg)
    sdr_f, base_f, md_f, gm_f = _fused(u, hdr.to("cuda:0"))
    hip_ctx.synchronize()
    sdr_o = L.tone_map(oracle_kind(), hdr)
    got = (base_f if fmt == P010 else sdr_f).to_host()
    if fmt == P010:
        for i in range(3):
            assert_close_codes(got.valid(i), sdr_o.valid(i), 1, 1e-4, f"fused sdr plane {i}")
    else:
        assert_close_codes(got.valid(0).view(np.uint8), sdr_o.valid(0).view(np.uint8), 1, 1e-4, "fused sdr")
    md_o, gm_o = L.generate_gainmap(oracle_kind(), got, hdr, cfg)
    tol = 1e-4 if cfg.gamma == 1.0 else 5e-3
    gm_h = gm_f.to_host()
    assert gm_h.valid(0).shape == gm_o.valid(0).shape
    assert_close_codes(gm_h.valid(0), gm_o.valid(0), 1, tol, "fused gain map")
    assert np.allclose(list(md_f.max_content_boost), list(md_o.max_content_boost), rtol=1e-6)


# ---- the one-call form ---------------------------------------------------------------------------------------------------------------
def _quant():
    return ((L.quant_table_port(95, False), L.quant_table_port(95, True)), (L.quant_table_port(85, False), L.quant_table_port(85, True)))


def _staged_scans(hip_ctx, u, hdr, qb, qm):
    """The staged route to the two scans: the operators, per-plane fdct_quant / fdct_quant_rgb on the (w / S) x (h / S) map, huffman_encode2."""
    w, h = hdr.w, hdr.h
    _, base, md, gm = _staged(u, hdr.to("cuda:0"))
    mw, mh = gm.w, gm.h
    nch = 3 if gm.raw.fmt == A.UHDR_IMG_FMT_24bppRGB888 else 1
    sub = 2 if hdr.fmt == P010 else 1  # chroma planes of the base image
    base_c = [u.fdct_quant(base.plane_tensor(i), base.raw.stride[i], (w if i == 0 else w // sub) // 8, (h if i == 0 else h // sub) // 8,
                           qb[0 if i == 0 else 1]) for i in range(3)]
    map_c = u.fdct_quant_rgb(gm, qm[0], qm[1]) if nch == 3 else [u.fdct_quant(gm.plane_tensor(0), gm.raw.stride[0], mw // 8, mh // 8, qm[0])]
    hip_ctx.synchronize()
    ob, om = u.huffman_encode2(base_c, w, h, [(sub, sub), (1, 1), (1, 1)], list(map_c), mw, mh, [(1, 1)] * nch)
    hip_ctx.synchronize()
    return ob.cpu().numpy().tobytes(), om.cpu().numpy().tobytes(), md, base.raw.cg


@pytest.mark.parametrize("w,h", [(64, 32), (288, 64)])
@pytest.mark.parametrize("multi", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
def test_api0_scans_scaled_equals_the_staged_route(hip_ctx, fmt, scale, multi, w, h):
    """Both scans byte for byte, the metadata, sdr_cg and gainmap_desc's dimensions and format; the caller's BEST_QUALITY is overridden."""
    u = _uhdr_for(hip_ctx, _cfg(scale, use_multi_channel_gainmap=multi))
    hdr = _make(fmt, w, h, A.UHDR_CT_HLG, A.UHDR_CG_BT_2100, FULL, seed=w + h)
    qb, qm = _quant()
    cap = w * h * 3 + 4096
    base, mp, md, desc, cg = u.encodeApi0ScansScaled(hdr, qb, qm, cap, cap)
    base_s, mp_s, md_s, cg_s = _staged_scans(hip_ctx, u, hdr, qb, qm)
    assert base == base_s, "base scan"
    assert mp == mp_s, "map scan"
    assert md.as_dict() == md_s.as_dict() and cg == cg_s == A.UHDR_CG_DISPLAY_P3
    assert (desc.w, desc.h, desc.fmt) == (w // scale, h // scale, A.UHDR_IMG_FMT_24bppRGB888 if multi else A.UHDR_IMG_FMT_8bppYCbCr400)
    cfg_b = _cfg(scale, use_multi_channel_gainmap=multi)
    cfg_b.preset = A.UHDR_USAGE_BEST_QUALITY
    base2, mp2, md2, _, _ = _uhdr_for(hip_ctx, cfg_b).encodeApi0ScansScaled(hdr, qb, qm, cap, cap)
    assert (base2, mp2) == (base, mp) and md2.as_dict() == md.as_dict()


@pytest.mark.parametrize("fmt", FMTS + [A.UHDR_IMG_FMT_64bppRGBAHalfFloat])
def test_api0_scans_scaled_at_scale_1_is_scans_any(hip_ctx, fmt):
    w, h = 64, 32
    u = _uhdr_for(hip_ctx, _cfg(1))
    hdr = synth.make_hdr_rgba_f16(w, h) if fmt == A.UHDR_IMG_FMT_64bppRGBAHalfFloat else _make(fmt, w, h, A.UHDR_CT_PQ, A.UHDR_CG_BT_2100, FULL)
    qb, qm = _quant()
    a = u.encodeApi0ScansScaled(hdr, qb, qm, 1 << 16, 1 << 16)
    b = u.encodeApi0ScansAny(hdr, qb, qm, 1 << 16, 1 << 16)
    assert a[0] == b[0] and a[1] == b[1] and a[2].as_dict() == b[2].as_dict() and a[4] == b[4]
    assert (a[3].w, a[3].h, a[3].fmt) == (b[3].w, b[3].h, b[3].fmt) == (w, h, A.UHDR_IMG_FMT_24bppRGB888)
    assert len(a[0]) > 0 and len(a[1]) > 0


@pytest.mark.parametrize("fmt", FMTS)
def test_api0_scans_scaled_reports_both_sizes(hip_ctx, fmt):
    u = _uhdr_for(hip_ctx, _cfg(2))
    hdr = _make(fmt, 288, 64, A.UHDR_CT_HLG, A.UHDR_CG_BT_2100, FULL)
    qb, qm = _quant()
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi0ScansScaled(hdr, qb, qm, 64, 64)
    assert e.value.code == A.UHDR_CODEC_MEM_ERROR
    nb, nm = e.value.needed
    assert nb > 64 and nm > 64
    base, mp, _, _, _ = u.encodeApi0ScansScaled(hdr, qb, qm, nb, nm)
    roomy = u.encodeApi0ScansScaled(hdr, qb, qm, 1 << 20, 1 << 20)
    assert 64 < len(base) <= nb and 64 < len(mp) <= nm and (base, mp) == (roomy[0], roomy[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(fn, *a, **kw):
    with pytest.raises(A.UhdrError) as e:
        fn(*a, **kw)
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE, e.value


def _view(img, plane, byte_offset):
    v = A.RawImage()
    C.memmove(C.byref(v), C.byref(img.raw), C.sizeof(A.RawImage))
    v.planes[plane] = img.raw.planes[plane] + byte_offset
    return v


def test_scaled_entry_points_refuse_what_they_cannot_take(hip_ctx):
    lib = hip_ctx.lib
    qb, qm = _quant()
    pq, c2100 = A.UHDR_CT_PQ, A.UHDR_CG_BT_2100
    rgb, p010 = _make(RGBA, 64, 32, pq, c2100, FULL), _make(P010, 64, 32, pq, c2100, FULL)
    f16 = synth.make_hdr_rgba_f16(64, 32)
    d_rgb, d_p010, d_f16 = rgb.to("cuda:0"), p010.to("cuda:0"), f16.to("cuda:0")
    # any scale factor other than 1, 2 or 4
    for s in (3, 8):
        u = _uhdr_for(hip_ctx, _cfg(s))
        _refused(u.encodeApi0FusedScaled, d_rgb)
        _refused(u.encodeApi0FusedP010Scaled, d_p010)
        _refused(u.encodeApi0ScansScaled, rgb, qb, qm, 1 << 16, 1 << 16)
        _refused(u.encodeApi0ScansScaled, p010, qb, qm, 1 << 16, 1 << 16)
    for s in SCALES:
        u = _uhdr_for(hip_ctx, _cfg(s))
        # a half-float intent
        _refused(u.encodeApi0FusedScaled, d_f16)
        _refused(u.encodeApi0ScansScaled, f16, qb, qm, 1 << 16, 1 << 16)
        # the wrong front end for the format
        _refused(u.encodeApi0FusedScaled, d_p010)
        _refused(u.encodeApi0FusedP010Scaled, d_rgb)
        # the two-pass preset on the two _dev forms
        cfg_b = _cfg(s)
        cfg_b.preset = A.UHDR_USAGE_BEST_QUALITY
        ub = _uhdr_for(hip_ctx, cfg_b)
        _refused(ub.encodeApi0FusedScaled, d_rgb)
        _refused(ub.encodeApi0FusedP010Scaled, d_p010)
        # a width that is not a multiple of 4, a height that is not a multiple of S
        _refused(u.encodeApi0FusedScaled, _make(RGBA, 62, 32, pq, c2100, FULL).to("cuda:0"))
        _refused(u.encodeApi0FusedP010Scaled, _make(P010, 62, 32, pq, c2100, FULL).to("cuda:0"))
        h_bad = 9 if s == 2 else 18
        _refused(u.encodeApi0FusedScaled, _make(RGBA, 64, h_bad, pq, c2100, FULL).to("cuda:0"))
        _refused(u.encodeApi0FusedP010Scaled, _make(P010, 64, h_bad, pq, c2100, FULL).to("cuda:0"))
        # layouts the vector accesses cannot read.  60 pixels in rows of 64: a view one pixel / two bytes in stays inside the allocation
        cfg = u.encode_cfg(False, False)
        md = A.GainmapMetadata()
        wide = _make(RGBA, 60, 32, pq, c2100, FULL).to("cuda:0")
        ycc = Image(A.UHDR_IMG_FMT_24bppYCbCr444, 60, 32, align=64, device="cuda:0")
        gm60 = Image(A.UHDR_IMG_FMT_24bppRGB888, 60 // s, 32 // s, align=64, device="cuda:0")
        v = _view(wide, 0, 4)  # an intent base that is not 16-byte aligned
        st = lib.uhdr_hip_encode_api0_fused_scaled_dev(hip_ctx.handle, C.byref(v), C.byref(cfg), None, C.byref(ycc.raw), C.byref(md), C.byref(gm60.raw))
        assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
        vb = _view(ycc, 1, 2)  # a Cb plane base that is not 4-byte aligned
        st = lib.uhdr_hip_encode_api0_fused_scaled_dev(hip_ctx.handle, C.byref(wide.raw), C.byref(cfg), None, C.byref(vb), C.byref(md), C.byref(gm60.raw))
        assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
        st = lib.uhdr_hip_encode_api0_fused_scaled_dev(hip_ctx.handle, C.byref(wide.raw), C.byref(cfg), None, C.byref(ycc.raw), C.byref(md), C.byref(gm60.raw))
        assert st.error_code == A.UHDR_CODEC_OK  # (the same call on the images themselves is taken)
        wide_p = _make(P010, 60, 32, pq, c2100, FULL).to("cuda:0")
        b420 = Image(A.UHDR_IMG_FMT_12bppYCbCr420, 60, 32, align=64, device="cuda:0")
        vp = _view(wide_p, 1, 2)  # a P010 chroma base that is not 4-byte aligned
        st = lib.uhdr_hip_encode_api0_p010_fused_scaled_dev(hip_ctx.handle, C.byref(vp), C.byref(cfg), C.byref(b420.raw), C.byref(md), C.byref(gm60.raw))
        assert st.error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
        st = lib.uhdr_hip_encode_api0_p010_fused_scaled_dev(hip_ctx.handle, C.byref(wide_p.raw), C.byref(cfg), C.byref(b420.raw), C.byref(md), C.byref(gm60.raw))
        assert st.error_code == A.UHDR_CODEC_OK
        hip_ctx.synchronize()
        # the scans form: dimensions that are not whole MCUs (8; 16 for P010)
        _refused(u.encodeApi0ScansScaled, _make(RGBA, 64, 36, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
        _refused(u.encodeApi0ScansScaled, _make(P010, 64, 40, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
    # the scans form: a map that is not whole blocks.  72 / 2 = 36, 72 / 4 = 18, 40 / 2 = 20; P010: 80 / 4 = 20 (at S = 2 whole MCUs give whole blocks)
    u2, u4 = _uhdr_for(hip_ctx, _cfg(2)), _uhdr_for(hip_ctx, _cfg(4))
    _refused(u2.encodeApi0ScansScaled, _make(RGBA, 72, 32, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
    _refused(u4.encodeApi0ScansScaled, _make(RGBA, 72, 32, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
    _refused(u2.encodeApi0ScansScaled, _make(RGBA, 64, 40, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
    _refused(u4.encodeApi0ScansScaled, _make(P010, 80, 32, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)
    _refused(u4.encodeApi0ScansScaled, _make(P010, 64, 48, pq, c2100, FULL), qb, qm, 1 << 16, 1 << 16)


def test_api0_scans_scaled_refuses_a_context_with_a_communicator():
    from libultrahdr_amd.stripes import init_comm_relay
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    try:
        init_comm_relay(ctx)
        qb, qm = _quant()
        for fmt in FMTS:
            _refused(_uhdr_for(ctx, _cfg(2)).encodeApi0ScansScaled, _make(fmt, 64, 32, A.UHDR_CT_PQ, A.UHDR_CG_BT_2100, FULL), qb, qm, 1 << 16, 1 << 16)
    finally:
        ctx.lib.uhdr_hip_comm_destroy(ctx.handle)
        ctx.close()


def test_the_old_entry_points_still_refuse_scale_2(hip_ctx):
    u = _uhdr_for(hip_ctx, _cfg(2))
    qb, qm = _quant()
    rgb, p010 = _make(RGBA, 64, 32, A.UHDR_CT_PQ, A.UHDR_CG_BT_2100, FULL), _make(P010, 64, 32, A.UHDR_CT_PQ, A.UHDR_CG_BT_2100, FULL)
    _refused(u.encodeApi0Fused, rgb.to("cuda:0"))
    _refused(u.encodeApi0FusedP010, p010.to("cuda:0"))
    _refused(u.encodeApi0ScansAny, rgb, qb, qm, 1 << 16, 1 << 16, any_format=False)
    _refused(u.encodeApi0ScansAny, rgb, qb, qm, 1 << 16, 1 << 16)
    _refused(u.encodeApi0ScansAny, p010, qb, qm, 1 << 16, 1 << 16)
