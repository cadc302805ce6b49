"""GPU: generateGainMap on a 4:4:4 SDR intent in coefficient form (uhdr_hip_generate_gainmap_coef444_dev: the dequantize + IDCT stage
inside pass 1 / the one-pass generation, 128 x 8 pixel tiles per wave), section by section what tests/test_gpu_generate_coef.py checks
for the sixteen-row tile.  Bit for bit against the library's staged operators (uhdr_hip_idct_dequant_dev x 3 into a w x h
UHDR_IMG_FMT_24bppYCbCr444 image, then uhdr_hip_generate_gainmap_dev) over every template instance of the kernel, against the oracle
within the allowance test_gpu_parity.py::test_generate_gainmap already grants the staged route, and on the things that can only go
wrong here: wild coefficients, pixels of the block grid beyond the image, extrema in tiles of every loop trip, requests the kernel
does not cover.  What the cases share is built once per geometry and kept for this module only: it is released with the module, so that the
tests that follow find the device allocator as the tests before left it."""
import ctypes as C
import gc

import numpy as np
import pytest

import test_gpu_generate_coef as M
import tile_loop_shapes as T
import tile_loop_shapes_api3_444 as G8
from libultrahdr_amd import capi as A
from libultrahdr_amd import stripes
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMT444 = A.UHDR_IMG_FMT_24bppYCbCr444
P010 = A.UHDR_IMG_FMT_24bppYCbCrP010
BT709, P3, BT2100 = A.UHDR_CG_BT_709, A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_2100
BEST, REALTIME = A.UHDR_USAGE_BEST_QUALITY, A.UHDR_USAGE_REALTIME
ENTRY = {"420": "uhdr_hip_generate_gainmap_coef_dev", "422": "uhdr_hip_generate_gainmap_coef422_dev", "444": "uhdr_hip_generate_gainmap_coef444_dev"}
# 16 x 8: less than one tile.  128 x 8: exactly one.  130 x 10: a second tile column and row with two live pixels / rows (scale
# factors 1 and 2 only).  392 x 100: partial last tiles in both directions and a last block row with four live rows.
SHAPES = ((16, 8), (128, 8), (130, 10), (392, 100))


def grid(w, h):
    """(blocks_w, blocks_h) of every component of a 4:4:4 frame: libjpeg's width_in_blocks / height_in_blocks."""
    return (w + 7) // 8, (h + 7) // 8


_shared = {}  # what the cases share; emptied when the module is done


@pytest.fixture(scope="module", autouse=True)
def _release_shared_data():
    yield
    _shared.clear()
    gc.collect()


def _once(key, make):
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def coef_case(w, h, quality=88, wild=False):
    """Coefficients of a 4:4:4 image on libjpeg's grid (a smooth field + noise through the oracle's FDCT, three different tables;
    wild: the full int16 range with all-255 tables) and, on the device, the same.  Built once per geometry and left unchanged."""
    return _once(("coef", w, h, quality, wild), lambda: _coef_case(w, h, quality, wild))


def hdr_case(kind, w, h, cg, misaligned=False):
    """tests/test_gpu_generate_coef.py::hdr_case, kept here instead of in that module's cache."""
    return _once(("hdr", kind, w, h, cg, misaligned), lambda: M.hdr_case.__wrapped__(kind, w, h, cg, misaligned))


def _coef_case(w, h, quality, wild):
    import torch

    rng = np.random.default_rng(1000 * w + h + 444)
    bw, bh = grid(w, h)
    if wild:
        qts = [np.full(64, 255, dtype=np.uint16)] * 3
        coefs = [rng.integers(-32768, 32768, (bh, bw, 64), dtype=np.int16) for _ in range(3)]
    else:
        qts = [L.quant_table_port(quality, False), L.quant_table_port(quality, True), L.quant_table_port(max(quality - 10, 1), True)]
        coefs = []
        for c in range(3):
            yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
            pl = 128 + 90 * np.sin(xx / (13.0 + 5 * c)) * np.cos(yy / (9.0 + 3 * c)) + rng.normal(0, 12, (bh * 8, bw * 8))
            coefs.append(L.fdct_quant_port(np.ascontiguousarray(np.clip(pl, 0, 255).astype(np.uint8)), bw * 8, bw, bh, qts[c]))
    return coefs, qts, [torch.from_numpy(c).to(DEV) for c in coefs]


def _decode(coefs, qts, w, h, cg):
    """The oracle's decode of the coefficients as a w x h host 4:4:4 image."""
    dec = Image(FMT444, w, h, cg, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    for c in range(3):
        dec.valid(c)[:] = L.idct_dequant_port(coefs[c], qts[c])[:h, :w]
    return dec


def staged_image(u, dcoefs, qts, w, h, cg):
    """uhdr_hip_idct_dequant_dev x 3 into a device 4:4:4 image of w x h whose planes hold the whole block grid."""
    bw, bh = grid(w, h)
    img = Image(FMT444, bw * 8, bh * 8, cg, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=16, device=DEV)
    for c in range(3):
        pl = img.plane_tensor(c)
        assert pl.shape[0] >= bh * 8 and pl.shape[1] >= bw * 8
        u.idct_dequant(dcoefs[c], qts[c], plane=pl, stride=pl.shape[1])
    img.raw.w, img.raw.h = w, h
    img.w, img.h = w, h
    return img


def both_routes(ctx, cfg, dcoefs, qts, w, h, sdr_cg, dhdr):
    """((metadata, map bytes, description) of the coefficient operator, the same of the staged operators)."""
    u = M.uhdr_for(ctx, cfg)
    md_f, gm_f = u.generateGainMapFromCoefficients(dcoefs, qts, w, h, sdr_cg, dhdr, "444", bool(cfg.sdr_is_601), bool(cfg.use_luminance))
    ctx.synchronize()
    md_s, gm_s = u.generateGainMap(staged_image(u, dcoefs, qts, w, h, sdr_cg), dhdr, bool(cfg.sdr_is_601), bool(cfg.use_luminance))
    ctx.synchronize()
    desc = lambda g: (g.raw.fmt, g.raw.w, g.raw.h, g.raw.cg, g.raw.ct, g.raw.range)
    return (md_f.as_dict(), gm_f.to_host().valid(0), desc(gm_f)), (md_s.as_dict(), gm_s.to_host().valid(0), desc(gm_s))


def assert_routes_equal(ctx, cfg, w, h, sdr_cg, hdr_kind, hdr_cg, misaligned=False, wild=False, what=""):
    coefs, qts, dcoefs = coef_case(w, h, wild=wild)
    fused, staged = both_routes(ctx, cfg, dcoefs, qts, w, h, sdr_cg, hdr_case(hdr_kind, w, h, hdr_cg, misaligned)[1])
    assert fused[2] == staged[2], what
    diff = int((fused[1] != staged[1]).sum())
    assert diff == 0, f"{what}: {diff} map bytes differ from the staged operators"
    assert fused[0] == staged[0], f"{what}: metadata {fused[0]} != {staged[0]}"


# ---- 1. against the staged operators, every template instance -------------------------------------------------------------------------------
# An instance is (HDR format, preset, quad fetch).  Each gets three cases, built so that within the instance every value of every
# other axis appears: channels {1, 3}, scale factor {1, 2, 4} (the quad fetch exists at 1 only), the HDR kinds of its format, gamut
# pairs giving use_base_cg 1 / 0 and an equal pair, sdr_is_601 {0, 1}, use_luminance {0, 1}.
INSTANCES = [(f, p, q) for f in ("p010", "1010102", "f16") for p in (BEST, REALTIME) for q in ((True, False) if f == "p010" else (False,))]


@pytest.mark.parametrize("hdr_fmt,preset,quad", INSTANCES, ids=[f"{f}-{'two' if p == BEST else 'one'}-pass-{'quad' if q else 'px'}" for f, p, q in INSTANCES])
def test_operator_equals_the_staged_operators(hip_ctx, hdr_fmt, preset, quad):
    ran = 0
    for k in range(3):
        scale = 1 if quad else (1, 2, 4)[k]
        sdr_cg, hdr_cg = M.GAMUTS[k]
        kind = M.HDR_KINDS[hdr_fmt][k % len(M.HDR_KINDS[hdr_fmt])]
        cfg = A.default_encode_cfg(map_dimension_scale_factor=scale, use_multi_channel_gainmap=k % 2, preset=preset, sdr_is_601=(k + 1) % 2, use_luminance=int(k == 0))
        # P010 at scale factor 1 without the quad fetch: a luma plane that is not 4-byte aligned
        misaligned = hdr_fmt == "p010" and not quad and scale == 1
        for (w, h) in SHAPES:
            if (w % scale or h % scale) and (w, h) == (130, 10):
                continue
            assert_routes_equal(hip_ctx, cfg, w, h, sdr_cg, kind, hdr_cg, misaligned, what=f"{w}x{h} 444 {kind} S={scale} ch={1 + 2 * (k % 2)}")
            ran += 1
    assert ran >= 11


@pytest.mark.parametrize("preset,nch", [(BEST, 1), (REALTIME, 0)])
def test_gamma_and_the_content_boost_hints(hip_ctx, preset, nch):
    """gamma 1.7 (no step tables: the per-sample evaluation of either preset), and both content-boost hints on the two-pass range."""
    for (w, h) in ((130, 10), (392, 100)):
        cfg = A.default_encode_cfg(use_multi_channel_gainmap=nch, preset=preset, gamma=1.7)
        assert_routes_equal(hip_ctx, cfg, w, h, BT709, "p010-hlg-limited", BT2100, what=f"gamma 1.7 {w}x{h}")
        cfg = A.default_encode_cfg(use_multi_channel_gainmap=nch, preset=preset, min_content_boost=1.5, max_content_boost=3.0)
        assert_routes_equal(hip_ctx, cfg, w, h, BT709, "1010102-pq", BT2100, what=f"hints {w}x{h}")


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_kw", [dict(), dict(preset=REALTIME, use_multi_channel_gainmap=0, map_dimension_scale_factor=4), dict(gamma=1.7, map_dimension_scale_factor=2)],
                         ids=["two-pass-3ch-S1", "one-pass-1ch-S4", "gamma-S2"])
def test_operator_against_the_oracle(hip_ctx, cfg_kw):
    """The allowance of test_gpu_parity.py::test_generate_gainmap: +-1 map code on <= 1e-4 of the samples (5e-3 with gamma != 1, which keeps
    a device pow per sample), metadata within 1e-6 relative.  The differing-sample count of either route is printed."""
    w, h = 392, 100
    cfg = A.default_encode_cfg(sdr_is_601=1, **cfg_kw)
    coefs, qts, dcoefs = coef_case(w, h)
    hdr, dhdr = hdr_case("p010-hlg-limited", w, h, BT2100)
    md_w, gm_w = L.generate_gainmap(M.oracle_kind(), _decode(coefs, qts, w, h, BT709), hdr, cfg)
    fused, staged = both_routes(hip_ctx, cfg, dcoefs, qts, w, h, BT709, dhdr)
    want = gm_w.valid(0)
    for name, (md, got, desc) in (("coefficient operator", fused), ("staged operators", staged)):
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print(f"{name} 444 {cfg_kw}: {int((d != 0).sum())} of {d.size} samples differ from the oracle, max {int(d.max())}")
        assert desc[:3] == (gm_w.raw.fmt, gm_w.raw.w, gm_w.raw.h)
        assert d.max() <= 1, name
        assert (d != 0).mean() <= (5e-3 if cfg.gamma != 1.0 else 1e-4), name
        dw = md_w.as_dict()
        for k in dw:
            assert np.allclose(md[k], dw[k], rtol=1e-6, atol=0), (name, k, md[k], dw[k])


# ---- 3. wild coefficients ---------------------------------------------------------------------------------------------------------------
def test_wild_coefficients(hip_ctx):
    """The full int16 range with all-255 tables: the 32-bit multiply path of the IDCT and the modulo-1024 range limit."""
    for (w, h, preset, scale) in ((256, 24, BEST, 1), (130, 10, REALTIME, 2)):
        cfg = A.default_encode_cfg(preset=preset, map_dimension_scale_factor=scale)
        assert_routes_equal(hip_ctx, cfg, w, h, BT709, "p010-pq-full", BT2100, wild=True, what=f"wild {w}x{h}")


# ---- 4. pixels of the block grid beyond the image --------------------------------------------------------------------------------------------
def test_cropped_pixels_stay_out(hip_ctx):
    """130 x 10, two pass, quality-100 tables: the live area is mid-grey and smooth, the padded columns and rows of the 136 x 16 block
    grid decode to 0, and the HDR intent -- brighter than the live area everywhere -- lies in an allocation whose pitch and rows cover the
    whole padded grid, so that no kernel, right or wrong, reads outside an allocation.  A ratio taken from the padding (HDR over black:
    the dark-pixel cap) would move max_content_boost: the metadata and the map equal the staged operators'."""
    import torch

    w, h = 130, 10
    bw, bh = grid(w, h)
    assert (bw * 8, bh * 8) == (136, 16)
    qts = [np.ones(64, dtype=np.uint16)] * 3
    coefs = []
    for c in range(3):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
        pl = np.zeros((bh * 8, bw * 8), dtype=np.uint8)
        pl[:h, :w] = (128 + (10 if c == 0 else 0) * np.sin(xx / 17.0) * np.cos(yy / 11.0))[:h, :w].astype(np.uint8)
        coefs.append(L.fdct_quant_port(np.ascontiguousarray(pl), bw * 8, bw, bh, qts[c]))
        dec = L.idct_dequant_port(coefs[c], qts[c])
        assert dec[:h, :w].min() > 100 and dec[h + 2:, :].max(initial=0) < 16 and dec[:, w + 2:].max(initial=0) < 16
    dcoefs = [torch.from_numpy(c).to(DEV) for c in coefs]
    wp, hp = 144, 32
    # PQ codes 480..520 are about 70..100 nits over a live area of about 36..52 nits: ratios below 3.  Over black the ratio would sit at
    # computeGain's dark-pixel cap, 2^2.3 = 4.92
    hdr = Image(P010, wp, hp, BT2100, A.UHDR_CT_PQ, A.UHDR_CR_FULL_RANGE, 64)
    hdr.valid(0)[:] = np.random.default_rng(3).integers(480, 521, hdr.valid(0).shape).astype(np.uint16) << 6
    hdr.valid(1)[:] = np.uint16(512 << 6)
    dhdr = hdr.to(DEV)
    assert dhdr.raw.stride[0] >= wp and dhdr.layout[0][0] >= hp
    dhdr.raw.w, dhdr.raw.h = w, h
    dhdr.w, dhdr.h = w, h
    for nch in (0, 1):
        cfg = A.default_encode_cfg(use_multi_channel_gainmap=nch)
        fused, staged = both_routes(hip_ctx, cfg, dcoefs, qts, w, h, BT709, dhdr)
        print("max_content_boost", fused[0]["max_content_boost"], staged[0]["max_content_boost"])
        assert fused[0] == staged[0]
        assert np.array_equal(fused[1], staged[1]) and fused[2] == staged[2]
        assert max(fused[0]["max_content_boost"]) < 4.0  # (4.92 with a single sample of the padding)


# ---- 5. extrema in every kind of tile -------------------------------------------------------------------------------------------------
def test_extrema_in_tiles_of_both_trips(hip_ctx):
    """Two pass, one channel, on the shape tests/tile_loop_shapes_api3_444.py gives for this device: some waves walk two tiles.  The
    smallest ratio of the staged ratio plane lies in a tile whose wave comes round again, the largest in a tile only a second trip
    reaches -- a wave that dropped or mixed up its running extrema on the way would report another range."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    loop = G8.coef_loop(cus, True)
    print(f"{cus} compute units; {T.describe(loop)}")
    assert T.satisfies(loop)
    w, h, edge = loop.w, loop.h, 32
    bw, bh = grid(w, h)
    gen = torch.Generator(device=DEV).manual_seed(loop.items)
    qts = [np.ones(64, dtype=np.uint16)] * 3
    dcoefs = []
    for c in range(3):  # mid-grey blocks with a little texture, independent per block: a tile in another's place shows
        t = torch.randint(-5, 6, (bh, bw, 64), generator=gen, device=DEV, dtype=torch.int16)
        t[:, :, 0] = torch.randint(-160, 161, (bh, bw), generator=gen, device=DEV, dtype=torch.int16) if c == 0 else 0
        dcoefs.append(t.contiguous())
    dhdr = Image(P010, w, h, BT2100, A.UHDR_CT_HLG, A.UHDR_CR_LIMITED_RANGE, 64, device=DEV)
    luma = dhdr.plane_tensor(0).view(torch.int16)
    luma[:, :] = torch.randint(400, 520, luma.shape, generator=gen, device=DEV, dtype=torch.int16) << 6
    luma[:edge] = torch.randint(160, 400, luma[:edge].shape, generator=gen, device=DEV, dtype=torch.int16) << 6     # a dark head
    luma[h - edge: h] = torch.randint(520, 941, luma[:edge].shape, generator=gen, device=DEV, dtype=torch.int16) << 6  # a bright tail
    chroma = dhdr.plane_tensor(1).view(torch.int16)
    chroma[:, :] = torch.randint(490, 534, chroma.shape, generator=gen, device=DEV, dtype=torch.int16) << 6
    torch.cuda.synchronize()
    cfg = A.default_encode_cfg(use_multi_channel_gainmap=0, sdr_is_601=1)
    u = M.uhdr_for(hip_ctx, cfg)
    md_f, gm_f = u.generateGainMapFromCoefficients(dcoefs, qts, w, h, BT709, dhdr, "444", True, True)
    hip_ctx.synchronize()
    sdr = staged_image(u, dcoefs, qts, w, h, BT709)
    md_s, gm_s = u.generateGainMap(sdr, dhdr, True, True)
    hip_ctx.synchronize()
    assert md_f.as_dict() == md_s.as_dict()
    assert torch.equal(gm_f.plane_tensor(0)[:, :w], gm_s.plane_tensor(0)[:, :w])
    # where the extrema are: the staged route's ratio plane (pass 1 of the striped interface on the whole image)
    ratio = torch.empty((h, w), dtype=torch.float32, device=DEV)
    mm = torch.empty(6, dtype=torch.float32, device=DEV)
    ubc = C.c_int(0)
    torch.cuda.synchronize()
    A.check(hip_ctx.lib.uhdr_hip_generate_gainmap_pass1_dev(hip_ctx.handle, C.byref(sdr.raw), C.byref(dhdr.raw), C.byref(cfg), C.c_void_p(ratio.data_ptr()),
                                                         C.c_void_p(mm.data_ptr()), C.byref(ubc)))
    hip_ctx.synchronize()
    tile_of = lambda i: (int(i) // w // G8.TILE_ROWS) * loop.tiles_x + (int(i) % w) // 128
    t_min, t_max = tile_of(ratio.argmin()), tile_of(ratio.argmax())
    print(f"smallest ratio in tile {t_min}, largest in tile {t_max}; {loop.items} tiles over {loop.walkers} waves")
    assert t_min < loop.items - loop.walkers, "the smallest ratio is not in a first-trip tile whose wave walks a second one"
    assert t_max >= loop.walkers, "the largest ratio is not in a tile of the second trip"


# ---- 6. what the operator declines -------------------------------------------------------------------------------------------------------
def _refused(ctx, cfg, dcoefs, qts, w, h, entry, dhdr, code, names_alternative=True):
    """The call at the entry point of sampling `entry` is refused with `code`, the message names the staged operators, and neither the
    metadata nor the map was touched."""
    gm = Image(A.UHDR_IMG_FMT_24bppRGB888, max(w, 8), max(h, 8), align=64, device=DEV, fill=0x5A)
    jc = A.JpegCoefficients()
    for i in range(3):
        jc.coef[i] = dcoefs[i].data_ptr()
        jc.blocks_h[i], jc.blocks_w[i] = int(dcoefs[i].shape[0]), int(dcoefs[i].shape[1])
        for k in range(64):
            jc.qtable[i][k] = int(qts[i][k])
    md = A.GainmapMetadata()
    C.memset(C.byref(md), 0x5A, C.sizeof(md))
    before = bytes(md)
    st = getattr(ctx.lib, ENTRY[entry])(ctx.handle, C.byref(jc), w, h, BT709, C.byref(dhdr.raw), C.byref(cfg), C.byref(md), C.byref(gm.raw))
    ctx.synchronize()
    assert st.error_code == code, (st.error_code, st.detail)
    if names_alternative:
        assert b"uhdr_hip_idct_dequant_dev" in st.detail and b"uhdr_hip_generate_gainmap_dev" in st.detail, st.detail
    assert bytes(md) == before
    assert bool((gm.buf == 0x5A).all())
    return st


def _zeros(w, h):
    import torch

    bw, bh = grid(w, h)
    return [torch.zeros((bh, bw, 64), dtype=torch.int16, device=DEV) for _ in range(3)]


def test_declines_leave_everything_untouched(hip_ctx):
    import torch

    w, h = 392, 100
    coefs, qts, dcoefs = coef_case(w, h)
    dhdr = hdr_case("p010-hlg-limited", w, h, BT2100)[1]
    UNSUP, INVAL = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM
    _refused(hip_ctx, A.default_encode_cfg(map_dimension_scale_factor=3), dcoefs, qts, w, h, "444", dhdr, UNSUP)
    # the small-image fallback of jpegr.cpp:696-706 changes the factor to min(w, h) / 8 = 3: 24 x 24 at a configured 32
    _refused(hip_ctx, A.default_encode_cfg(map_dimension_scale_factor=32), _zeros(24, 24), qts, 24, 24, "444", hdr_case("p010-hlg-limited", 24, 24, BT2100)[1], UNSUP)
    _refused(hip_ctx, A.default_encode_cfg(), _zeros(131, 10), qts, 131, 10, "444", hdr_case("1010102-pq", 131, 10, BT2100)[1], UNSUP)
    # the block grids of a 4:2:0 and of a 4:2:2 frame at the 4:4:4 entry point, and a 4:4:4 grid at each of the other two
    for other in ("420", "422"):
        theirs = [torch.zeros((gh, gw, 64), dtype=torch.int16, device=DEV) for gw, gh in M.grids(w, h, M.SAMPLINGS[other])]
        assert [tuple(t.shape[:2]) for t in theirs] != [tuple(t.shape[:2]) for t in dcoefs]
        _refused(hip_ctx, A.default_encode_cfg(), theirs, qts, w, h, "444", dhdr, INVAL, names_alternative=False)
        _refused(hip_ctx, A.default_encode_cfg(), dcoefs, qts, w, h, other, dhdr, INVAL, names_alternative=False)
    # one good call follows
    assert_routes_equal(hip_ctx, A.default_encode_cfg(), w, h, BT709, "p010-hlg-limited", BT2100, what="after the refusals")


def test_a_context_with_a_communicator_is_declined():
    from libultrahdr_amd.ultrahdr import Context

    w, h = 128, 8
    coefs, qts, dcoefs = coef_case(w, h)
    ctx = Context(0)
    try:
        assert stripes.init_comm_relay(ctx) == 1
        _refused(ctx, A.default_encode_cfg(), dcoefs, qts, w, h, "444", hdr_case("p010-hlg-limited", w, h, BT2100)[1], A.UHDR_CODEC_UNSUPPORTED_FEATURE)
    finally:
        ctx.close()
