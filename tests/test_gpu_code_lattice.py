"""Device parity on the code-lattice images of tests/code_lattice.py: every input code, the limited-range codes outside
the nominal range, YCbCr triples outside the RGB cube, and SDR black against HDR peak (and the other way round), so that
the content boost hits both clamps of jpegr.cpp:969-986, the map saturates at 0 and 255 and the applied output sits at
its ceiling.  That is where the kernels' tables end: the one-pass gain step table, the two-pass ratio -> byte tables with
their guard buckets, the dark-pixel cap in the ratio domain, the code -> linear tables, the unclipped LUT indices behind
yuv -> rgb, clip_neg behind the gamut matrices, the sRGB byte table and the HLG / PQ output tables at 10000/203.

The oracle is the real reference where oracle/_ref is loadable, the C restatement otherwise; tests/test_code_lattice.py
pins the two to each other on exactly these cases.  Bars are the project's existing ones: generateGainMap +-1 code on
<= 1e-4 of the samples (5e-3 with gamma != 1, as tests/fuzz_parity.py), metadata 1e-6 relative and exactly equal where the
reference's value is one of the two clamp constants; toneMap +-1 on <= 1e-4, a single differing sample passes
(fuzz_tonemap's rule); fused chains == the staged operators and applyGainMap == the oracle, bit for bit.  Every case
prints how many samples differ (pytest -s / -rP shows it)."""
import ctypes as C

import numpy as np
import pytest

import code_lattice as CL
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def _uhdr_for(hip_ctx, cfg):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx, mapDimensionScaleFactor=cfg.map_dimension_scale_factor,
                    useMultiChannelGainMap=bool(cfg.use_multi_channel_gainmap), gamma=cfg.gamma, preset=cfg.preset,
                    minContentBoost=cfg.min_content_boost, maxContentBoost=cfg.max_content_boost,
                    targetDispPeakBrightness=cfg.target_disp_peak_nits)


def _routes(hip_ctx):
    st = A.Stats()
    hip_ctx.lib.uhdr_hip_get_stats(hip_ctx.handle, C.byref(st))
    return np.array([st.generate_channels_tabled, st.generate_channels_per_sample], dtype=np.int64)


def _planes_equal(a: Image, b: Image):
    return all(np.array_equal(x, y) for x, y in zip(a.to_host().planes_valid(), b.to_host().planes_valid()))


def _diff(got: Image, want: Image):
    """(differing samples, samples, largest code difference) over all planes; packed 8-bit pixels count per byte."""
    n = tot = mx = 0
    for pg, pw in zip(got.planes_valid(), want.planes_valid()):
        if pg.dtype == np.uint32:
            pg, pw = pg.view(np.uint8), pw.view(np.uint8)
        d = np.abs(pg.astype(np.int64) - pw.astype(np.int64))
        n, tot, mx = n + int((d != 0).sum()), tot + d.size, max(mx, int(d.max()))
    return n, tot, mx


@pytest.fixture(scope="module")
def pairs():
    """name -> (sdr, hdr, sdr on the device, hdr on the device) at the main size; built once, never written."""
    out = {}
    for name in CL.PAIRS:
        s, h = CL.pair(name)
        out[name] = (s, h, s.to(DEV), h.to(DEV))
    return out


def _check_metadata(md_g, md_w, what):
    dg, dw = md_g.as_dict(), md_w.as_dict()
    for k in dw:
        assert np.allclose(dg[k], dw[k], rtol=1e-6, atol=0), (what, k, dg[k], dw[k])
    for k in ("min_content_boost", "max_content_boost"):
        for i in range(3):
            if dw[k][i] in (CL.CLAMP_MIN_BOOST, CL.CLAMP_MAX_BOOST):
                assert dg[k][i] == dw[k][i], (what, k, i, dg[k][i], dw[k][i])


@pytest.mark.parametrize("name,cfg_name", CL.GENERATE_CASES)
def test_generate_gainmap_on_the_lattice(hip_ctx, pairs, name, cfg_name):
    """generateGainMap, host and device buffers.  The default two-pass case must go through the ratio -> byte step
    tables: its range is the whole clamp, 29.9 log2 units."""
    sdr, hdr, dsdr, dhdr = pairs[name]
    cfg = CL.cfg(cfg_name)
    md_w, gm_w = L.generate_gainmap(oracle_kind(), sdr, hdr, cfg)
    u = _uhdr_for(hip_ctx, cfg)
    tol = 1e-4 if cfg.gamma == 1.0 else 5e-3
    for where, (a, b) in (("device", (dsdr, dhdr)), ("host", (sdr, hdr))):
        before = _routes(hip_ctx)
        md_g, gm_g = u.generateGainMap(a, b, bool(cfg.sdr_is_601), bool(cfg.use_luminance))
        hip_ctx.synchronize()
        tabled, per_sample = _routes(hip_ctx) - before
        gm_g = gm_g.to_host()
        assert (gm_g.raw.fmt, gm_g.raw.w, gm_g.raw.h) == (gm_w.raw.fmt, gm_w.raw.w, gm_w.raw.h)
        assert (gm_g.raw.cg, gm_g.raw.ct, gm_g.raw.range) == (gm_w.raw.cg, gm_w.raw.ct, gm_w.raw.range)
        n, tot, mx = _diff(gm_g, gm_w)
        route = "one pass" if cfg.preset == A.UHDR_USAGE_REALTIME else f"two pass, {tabled} channels tabled, {per_sample} per sample"
        print(f"generate {name} {cfg_name} {where}: {n}/{tot} samples differ, max {mx}; {route}")
        assert mx <= 1, f"{where}: max code diff {mx} ({n} samples differ)"
        assert n / tot <= tol, f"{where}: {n}/{tot} samples differ (allowed {tol:.0e})"
        _check_metadata(md_g, md_w, where)
        if cfg.preset == A.UHDR_USAGE_REALTIME:
            assert (tabled, per_sample) == (0, 0)
        else:
            assert tabled + per_sample == (3 if cfg.use_multi_channel_gainmap else 1)
        if cfg_name == "default":
            assert (tabled, per_sample) == (3, 0), "the default case left the step tables"


@pytest.mark.parametrize("key,ct,size", CL.TONEMAP_CASES)
def test_tone_map_on_the_lattice(hip_ctx, key, ct, size):
    """toneMap P010 -> 4:2:0, RGBA1010102 -> RGBA8888, 30bppYCbCr444 -> 4:4:4; host and device buffers.
    Measured on an MI355X against the real reference: identical in 34 of the 36 frames; the limited-range BT.2100 PQ 4:4:4
    image has one sample one code lower at both sizes (Cr 127 / 128 of the grey pixel Y 276, a value of 127.5 + 0.5 before
    truncation): srgbOetf's powf, tests/test_code_lattice.py::test_the_grey_sample_one_code_off_on_the_device_is_powf_rounding."""
    from libultrahdr_amd.ultrahdr import UltraHdr

    u = UltraHdr(ctx=hip_ctx)
    hdr = CL.tonemap_image(key, ct, size)
    want = L.tone_map(oracle_kind(), hdr)
    got_h = Image(want.fmt, *size, align=64)
    u.toneMap(hdr, got_h)
    got_d = Image(want.fmt, *size, align=64, device=DEV)
    u.toneMap(hdr.to(DEV), got_d)
    hip_ctx.synchronize()
    for where, got in (("host", got_h), ("device", got_d.to_host())):
        assert (got.raw.cg, got.raw.ct, got.raw.range) == (want.raw.cg, want.raw.ct, want.raw.range)
        n, tot, mx = _diff(got, want)
        print(f"tone map {key} ct{ct} {size[0]}x{size[1]} {where}: {n}/{tot} samples differ, max {mx}")
        assert mx <= 1, f"{where}: max code diff {mx} ({n} samples differ)"
        assert n <= 1 or n / tot <= 1e-4, f"{where}: {n}/{tot} samples differ"


@pytest.mark.parametrize("cfg_kw", [dict(preset=A.UHDR_USAGE_REALTIME), dict(preset=A.UHDR_USAGE_BEST_QUALITY),
                                    dict(preset=A.UHDR_USAGE_REALTIME, use_multi_channel_gainmap=0),
                                    dict(preset=A.UHDR_USAGE_BEST_QUALITY, use_multi_channel_gainmap=0)])
@pytest.mark.parametrize("key,ct", [("1010102-2100", CL.PQ), ("1010102-709", CL.HLG)])
def test_fused_api0_front_end_equals_the_three_operators_on_the_lattice(hip_ctx, key, ct, cfg_kw):
    """uhdr_hip_encode_api0_fused_dev == toneMap -> generateGainMap -> convert_raw_input_to_ycbcr(4:4:4), bit for bit."""
    w, h = CL.SIZE_PIXEL
    dh = CL.tonemap_image(key, ct, CL.SIZE_PIXEL).to(DEV)
    cfg = A.default_encode_cfg(use_luminance=0, **cfg_kw)
    u = _uhdr_for(hip_ctx, cfg)
    sdr_f, ycc_f, md_f, gm_f = u.encodeApi0Fused(dh, want_sdr_rgba=True, use_luminance=False)
    hip_ctx.synchronize()
    sdr_s = Image(A.UHDR_IMG_FMT_32bppRGBA8888, w, h, align=64, device=DEV)
    u.toneMap(dh, sdr_s)
    md_s, gm_s = u.generateGainMap(sdr_s, dh, False, False)
    ycc_s = u.convert_raw_input_to_ycbcr(sdr_s, False)
    hip_ctx.synchronize()
    assert _planes_equal(sdr_f, sdr_s), "sdr"
    assert _planes_equal(ycc_f, ycc_s), "base ycc"
    assert _planes_equal(gm_f, gm_s), f"map: {_diff(gm_f.to_host(), gm_s.to_host())}"
    assert md_f.as_dict() == md_s.as_dict()
    assert (ycc_f.raw.fmt, ycc_f.raw.cg, ycc_f.raw.range) == (ycc_s.raw.fmt, ycc_s.raw.cg, ycc_s.raw.range)


@pytest.mark.parametrize("name,scale,multi,convert", [("420+p010-hlg-limited", 1, True, True), ("420+p010-hlg-limited", 1, True, False),
                                                      ("420+p010-hlg-limited", 2, False, True), ("420+p010-hlg-limited", 2, False, False),
                                                      ("420p3+p010-pq-full", 1, True, False), ("420p3+p010-pq-full", 2, False, False)])
def test_api1_fused_chain_equals_the_operators_on_the_lattice(hip_ctx, pairs, name, scale, multi, convert):
    """uhdr_hip_encode_api1_fused_dev == generateGainMap -> fdct_quant_rgb / fdct_quant, convertYuv -> 3 x fdct_quant:
    coefficient blocks, the 8-bit map and the metadata, bit for bit."""
    import torch

    w, h = CL.SIZE_MAIN
    _, _, ds, dh = pairs[name]
    cfg = A.default_encode_cfg(map_dimension_scale_factor=scale, use_multi_channel_gainmap=int(multi))
    u = _uhdr_for(hip_ctx, cfg)
    ql, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
    qml, qmc = L.quant_table_port(90, False), L.quant_table_port(90, True)
    enc = A.UHDR_CG_DISPLAY_P3 if convert else A.UHDR_CG_UNSPECIFIED
    base_f, map_f, md_f, gm_f = u.encodeApi1Fused(ds, dh, enc, (ql, qc), (qml, qmc), want_map=True)
    hip_ctx.synchronize()
    md_s, gm_s = u.generateGainMap(ds, dh)
    base = ds.clone()
    if convert:
        u.convertYuv(base, ds.raw.cg, A.UHDR_CG_DISPLAY_P3)
    base_s = [u.fdct_quant(base.plane_tensor(i), base.raw.stride[i], (w if i == 0 else w // 2) // 8, (h if i == 0 else h // 2) // 8,
                           ql if i == 0 else qc) for i in range(3)]
    if multi:
        map_s = u.fdct_quant_rgb(gm_s, qml, qmc)
    else:
        map_s = [u.fdct_quant(gm_s.plane_tensor(0), gm_s.raw.stride[0], gm_s.w // 8, gm_s.h // 8, qml)]
    hip_ctx.synchronize()
    assert md_f.as_dict() == md_s.as_dict()
    assert _planes_equal(gm_f, gm_s), f"map: {_diff(gm_f.to_host(), gm_s.to_host())}"
    for i in range(3):
        assert torch.equal(base_f[i], base_s[i].reshape(base_f[i].shape)), f"base component {i}"
    for i in range(len(map_s)):
        assert torch.equal(map_f[i], map_s[i].reshape(map_f[i].shape)), f"map component {i}"


@pytest.fixture(scope="module")
def lattice_maps(pairs):
    """The oracle's own (metadata, map) of the generate cases applyGainMap is fed with."""
    return [L.generate_gainmap(oracle_kind(), pairs[name][0], pairs[name][1], CL.cfg(cfg_name)) for name, cfg_name in CL.APPLY_MAPS]


@pytest.mark.parametrize("m,ct,boost", CL.APPLY_CASES)
def test_apply_gainmap_of_the_lattice_map(hip_ctx, pairs, lattice_maps, m, ct, boost):
    """applyGainMap of the lattice SDR image with the map and metadata the oracle made of the lattice pair: a gain table
    over 30 binades, map bytes 0 and 255, the weight < 1 path (boost 4), the output tables at their ceiling.  Bit exact."""
    from libultrahdr_amd.ultrahdr import UltraHdr

    u = UltraHdr(ctx=hip_ctx)
    sdr, _, dsdr, _ = pairs[CL.APPLY_MAPS[m][0]]
    md, gm = lattice_maps[m]
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, ct, boost)
    fmt = A.UHDR_IMG_FMT_64bppRGBAHalfFloat if ct == A.UHDR_CT_LINEAR else A.UHDR_IMG_FMT_32bppRGBA1010102
    got_h = Image(fmt, sdr.w, sdr.h, align=1)
    u.applyGainMap(sdr, gm, md, ct, fmt, boost, got_h)
    got_d = Image(fmt, sdr.w, sdr.h, align=2, device=DEV)
    u.applyGainMap(dsdr, gm.to(DEV), md, ct, fmt, boost, got_d)
    hip_ctx.synchronize()
    for where, got in (("host", got_h), ("device", got_d.to_host())):
        n = int((got.valid(0) != want.valid(0)).sum())
        print(f"apply map {m} ct{ct} boost {boost:g} {where}: {n}/{want.valid(0).size} pixels differ")
        assert n == 0, f"{where}: {n} pixels differ"
        assert got.raw.cg == want.raw.cg
