"""GPU: a gain-map gamma other than 1 on the coefficient-input applyGainMap kernels (uhdr_hip_apply_gainmap_coef_ex_dev with
UHDR_HIP_APPLY_GAMMA_TABLE) and through the one-call decode (uhdr_hip_decode_api1_scans_ex_dev).  Bit for bit against the library's own
planes route -- three IDCT launches + uhdr_hip_apply_gainmap_ex_dev, which tests/test_gpu_apply_gamma.py holds to the oracle -- while
the three older coefficient entry points keep refusing the case with their message."""
import functools

import numpy as np
import pytest

from coef_cases import S420, S422, S444, grids, quality_tables, smooth_coefs
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, P1010102 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_32bppRGBA1010102
LINEAR, HLG, PQ = A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ
GT = A.UHDR_HIP_APPLY_GAMMA_TABLE
SAMPLINGS = {"420": (S420, A.UHDR_IMG_FMT_12bppYCbCr420), "422": (S422, A.UHDR_IMG_FMT_16bppYCbCr422), "444": (S444, A.UHDR_IMG_FMT_24bppYCbCr444)}
QUAD, PLAIN = "apply_gainmap_gamma_quad", "apply_gainmap"


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def out_fmt(ct):
    return F16 if ct == LINEAR else P1010102


def to_dev(coefs):
    import torch

    return [torch.from_numpy(c).to(DEV) for c in coefs]


@functools.lru_cache(maxsize=None)
def coef_case(sampling, w, h):
    """Coefficients of a w x h image on libjpeg's grids with three different quantization tables; built once and left unchanged."""
    rng = np.random.default_rng(1000 * w + h + int(sampling))
    qts = quality_tables(85)
    return smooth_coefs(grids(w, h, SAMPLINGS[sampling][0]), qts, rng), qts


def staged(uhdr, sampling, dcoefs, qts, w, h, gm_dev, md, out_ct, flags):
    """idct_dequant x 3 into a device image of that sampling, then applyGainMapEx (every plane is whole blocks at these sizes)."""
    img = Image(SAMPLINGS[sampling][1], w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=16, device=DEV)
    for c in range(3):
        pl = img.plane_tensor(c)
        assert pl.shape[0] == dcoefs[c].shape[0] * 8 and pl.shape[1] >= dcoefs[c].shape[1] * 8
        uhdr.idct_dequant(dcoefs[c], qts[c], plane=pl, stride=pl.shape[1])
    dest = Image(out_fmt(out_ct), w, h, align=4, device=DEV)
    uhdr.applyGainMapEx(img, gm_dev, md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest, flags)
    uhdr.ctx.synchronize()
    return dest.to_host()


MAPS = [("y400", 4), ("rgb888", 2)]


@pytest.mark.parametrize("out_ct", [LINEAR, HLG, PQ], ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("w,h", [(256, 48), (384, 176)])
@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_coefficient_kernel_equals_the_planes_route(uhdr, sampling, w, h, out_ct):
    coefs, qts = coef_case(sampling, w, h)
    dco = to_dev(coefs)
    ctx = uhdr.ctx
    for kind, scale in MAPS:
        gm = synth.make_gainmap(w // scale, h // scale, 1 if kind == "y400" else 3, cg=A.UHDR_CG_BT_2100).to(DEV)
        md = synth.default_metadata(gamma=1.571, per_channel=(kind != "y400"), use_base_cg=0 if kind == "y400" else 1)
        want = staged(uhdr, sampling, dco, qts, w, h, gm, md, out_ct, GT)
        ctx.synchronize()
        ctx.profile(True)
        ctx.profile_read(None)
        try:
            dest = Image(out_fmt(out_ct), w, h, align=4, device=DEV)
            uhdr.applyGainMapFromCoefficientsEx(dco, qts, w, h, A.UHDR_CG_BT_709, gm, md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest, sampling, GT)
            ctx.synchronize()
            assert ctx.profile_read(QUAD)[0] == 1 and ctx.profile_read(PLAIN)[0] == 0 and ctx.profile_read("idct_dequant")[0] == 0
        finally:
            ctx.profile_read(None)
            ctx.profile(False)
        got = dest.to_host()
        diff = int((got.valid(0) != want.valid(0)).sum())
        print(f"{sampling} {w}x{h} {kind} scale={scale} ct={out_ct}: {diff} differing samples")
        assert want.valid(0).any() and diff == 0


def test_the_planes_route_of_this_file_equals_the_oracle(uhdr):
    """The yardstick above, tied to the oracle once: its IDCT, then its applyGainMap."""
    w, h = 256, 48
    coefs, qts = coef_case("420", w, h)
    dec = Image(A.UHDR_IMG_FMT_12bppYCbCr420, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    for c in range(3):
        full = L.idct_dequant_port(coefs[c], qts[c])
        dec.valid(c)[:] = full[: dec.valid(c).shape[0], : dec.valid(c).shape[1]]
    gm = synth.make_gainmap(w // 4, h // 4, 1, cg=A.UHDR_CG_BT_2100)
    md = synth.default_metadata(gamma=1.571)
    kind = "ref" if L.ref() is not None else "port"
    dest = Image(F16, w, h, align=4, device=DEV)
    uhdr.applyGainMapFromCoefficientsEx(to_dev(coefs), qts, w, h, A.UHDR_CG_BT_709, gm.to(DEV), md, LINEAR, F16, A.FLT_MAX, dest, "420", GT)
    uhdr.ctx.synchronize()
    assert np.array_equal(dest.to_host().valid(0), L.apply_gainmap(kind, dec, gm, md, LINEAR).valid(0))


@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_the_old_entry_points_keep_refusing(uhdr, sampling):
    w, h = 256, 48
    coefs, qts = coef_case(sampling, w, h)
    dco = to_dev(coefs)
    gm = synth.make_gainmap(w // 4, h // 4, 1).to(DEV)
    md = synth.default_metadata(gamma=1.571)
    dest = Image(F16, w, h, align=4, device=DEV)
    old = (lambda: uhdr.applyGainMapFromCoefficients444(dco, qts, w, h, A.UHDR_CG_BT_709, gm, md, LINEAR, F16, A.FLT_MAX, dest)) if sampling == "444" else \
          (lambda: uhdr.applyGainMapFromCoefficients(dco, qts, w, h, A.UHDR_CG_BT_709, gm, md, LINEAR, F16, A.FLT_MAX, dest, sampling))
    flags0 = lambda: uhdr.applyGainMapFromCoefficientsEx(dco, qts, w, h, A.UHDR_CG_BT_709, gm, md, LINEAR, F16, A.FLT_MAX, dest, sampling, 0)
    for call in (old, flags0):
        with pytest.raises(A.UhdrError) as e:
            call()
        assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
        assert "an even scale <= 8 with gamma 1" in e.value.detail and "decode with idct_dequant and call apply_gainmap" in e.value.detail


def test_flags_the_coefficient_form_does_not_take(uhdr):
    w, h = 256, 48
    coefs, qts = coef_case("420", w, h)
    dco = to_dev(coefs)
    gm = synth.make_gainmap(w // 4, h // 4, 1).to(DEV)
    md = synth.default_metadata(gamma=1.571)
    dest = Image(F16, w, h, align=4, device=DEV)
    for flags in (A.UHDR_HIP_APPLY_RESIZED_MAP, A.UHDR_HIP_APPLY_RESIZED_MAP | GT, 0x4, GT | 0x100):
        with pytest.raises(A.UhdrError) as e:
            uhdr.applyGainMapFromCoefficientsEx(dco, qts, w, h, A.UHDR_CG_BT_709, gm, md, LINEAR, F16, A.FLT_MAX, dest, "420", flags)
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM
    jc = A.JpegCoefficients()
    import ctypes as C

    with pytest.raises(A.UhdrError) as e:  # a sampling that is none of the three
        A.check(uhdr.lib.uhdr_hip_apply_gainmap_coef_ex_dev(uhdr.ctx.handle, C.byref(jc), 411, w, h, A.UHDR_CG_BT_709, C.byref(gm.raw), C.byref(md), LINEAR, F16,
                                                            A.FLT_MAX, C.byref(dest.raw), GT))
    assert e.value.code == A.UHDR_CODEC_INVALID_PARAM


# ---- the one-call decode ---------------------------------------------------------------------------------------------------------------
def _map_scan(uhdr, mw, mh, seed):
    rng = np.random.default_rng(seed)
    ql = L.quant_table_port(92, False)
    dco = to_dev(smooth_coefs(grids(mw, mh, [(1, 1)]), [ql], rng))
    return uhdr.jpeg_header(mw, mh, [(1, 1)], [ql]), uhdr.huffman_encode(dco, mw, mh, [(1, 1)], 0), dco, ql


@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_one_call_decode_stays_on_the_coefficient_kernel(uhdr, sampling):
    w, h = 384, 176
    samp = SAMPLINGS[sampling][0]
    coefs, qts = coef_case(sampling, w, h)
    dco = to_dev(coefs)
    scan_b = uhdr.huffman_encode(dco, w, h, samp, 0)
    hb = uhdr.jpeg_header(w, h, samp, qts)
    mw, mh = w // 4, h // 4
    hm, scan_m, dmap, ql = _map_scan(uhdr, mw, mh, seed=w + int(sampling))
    md = synth.default_metadata(gamma=1.571, use_base_cg=0)
    base_cg, map_cg = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
    ctx = uhdr.ctx
    for out_ct in (LINEAR, PQ):
        # entropy decode + IDCTs + applyGainMapEx, step by step
        back = uhdr.huffman_decode(scan_b, [(bh, bw) for bw, bh in grids(w, h, samp)], w, h, samp, 0)
        assert all(np.array_equal(b.cpu().numpy(), c) for b, c in zip(back, coefs))
        plane = uhdr.idct_dequant(dmap[0], ql)
        uhdr.ctx.synchronize()
        gm = Image(A.UHDR_IMG_FMT_8bppYCbCr400, mw, mh, map_cg)
        gm.valid(0)[:] = plane.cpu().numpy()[:mh, :mw]
        want = staged(uhdr, sampling, back, qts, w, h, gm.to(DEV), md, out_ct, GT)
        for flags, fused in ((GT, True), (0, False)):
            ctx.synchronize()
            ctx.profile(True)
            ctx.profile_read(None)
            try:
                dest = Image(out_fmt(out_ct), w, h, align=64, device=DEV)
                uhdr.decodeApi1ScansEx(hb, scan_b, base_cg, hm, scan_m, map_cg, md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest, flags)
                ctx.synchronize()
                n_idct, n_quad, n_plain = ctx.profile_read("idct_dequant")[0], ctx.profile_read(QUAD)[0], ctx.profile_read(PLAIN)[0]
            finally:
                ctx.profile_read(None)
                ctx.profile(False)
            if fused:  # the map's IDCT only: no launch for the base image
                assert (n_idct, n_quad, n_plain) == (1, 1, 0)
                assert np.array_equal(dest.to_host().valid(0), want.valid(0))
            else:  # flags 0 is decodeApi1ScansAny: three more IDCT launches and the pow route, as before
                assert (n_idct, n_quad, n_plain) == (4, 0, 1)
                old = Image(out_fmt(out_ct), w, h, align=64, device=DEV)
                uhdr.decodeApi1ScansAny(hb, scan_b, base_cg, hm, scan_m, map_cg, md, out_ct, out_fmt(out_ct), A.FLT_MAX, old)
                ctx.synchronize()
                assert np.array_equal(dest.to_host().valid(0), old.to_host().valid(0))


def test_one_call_decode_refuses_the_flags_it_cannot_serve(uhdr):
    w, h = 256, 48
    coefs, qts = coef_case("420", w, h)
    scan_b = uhdr.huffman_encode(to_dev(coefs), w, h, S420, 0)
    hb = uhdr.jpeg_header(w, h, S420, qts)
    hm, scan_m, _, _ = _map_scan(uhdr, w // 4, h // 4, seed=5)
    md = synth.default_metadata(gamma=1.571)
    dest = Image(F16, w, h, align=64, device=DEV)
    for flags in (A.UHDR_HIP_APPLY_RESIZED_MAP, 0x8):
        with pytest.raises(A.UhdrError) as e:
            uhdr.decodeApi1ScansEx(hb, scan_b, A.UHDR_CG_BT_709, hm, scan_m, A.UHDR_CG_BT_709, md, LINEAR, F16, A.FLT_MAX, dest, flags)
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM
