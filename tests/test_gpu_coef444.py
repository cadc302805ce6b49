"""GPU: applyGainMap on a 4:4:4 base image in coefficient form (uhdr_hip_apply_gainmap_coef444_dev: the dequantize + IDCT stage
inside the 2x2-quad kernel, 128 x 8 pixel tiles of 16 + 16 + 16 blocks) and the one-call decode for any base sampling
(uhdr_hip_decode_api1_scans_any_dev) taking a 1x1 / 1x1 / 1x1 base scan through it.  Everything is bit for bit: against the
oracle's IDCT followed by the oracle's applyGainMap (whose 4:4:4 parity is held in test_oracle_vs_ref.py), and against the
library's own staged route."""
import functools
import io

import numpy as np
import pytest

from coef_cases import S420, S422, S444, grids, quality_tables, smooth_coefs as _smooth_coefs, wild_coefs
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, P1010102 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_32bppRGBA1010102
Y444 = A.UHDR_IMG_FMT_24bppYCbCr444


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def out_fmt(out_ct):
    return F16 if out_ct == A.UHDR_CT_LINEAR else P1010102


def _decode444(coefs, qts, w, h):
    dec = Image(Y444, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    for c in range(3):
        full = L.idct_dequant_port(coefs[c], qts[c])
        dec.valid(c)[:] = full[: dec.valid(c).shape[0], : dec.valid(c).shape[1]]
    return dec


@functools.lru_cache(maxsize=None)
def coef_case(w, h, quality, wild=False):
    """Coefficients of a 4:4:4 image on libjpeg's grids (as the Huffman decoder would hand them over), three different
    quantization tables, and the oracle's decode of them as a 4:4:4 Image.  Built once per geometry and left unchanged."""
    rng = np.random.default_rng(1000 * w + h)
    dims = grids(w, h, S444)
    if wild:  # the full int16 range with all-255 tables: the 32-bit multiply path and the modulo-1024 range limit
        qts = [np.full(64, 255, dtype=np.uint16)] * 3
        coefs = wild_coefs(dims, rng)
    else:
        qts = quality_tables(quality)
        coefs = _smooth_coefs(dims, qts, rng)
    return coefs, qts, _decode444(coefs, qts, w, h)


def to_dev(coefs):
    import torch

    return [torch.from_numpy(c).to(DEV) for c in coefs]


def run_coef444(uhdr, coefs, qts, w, h, gm, md, out_ct, align=4):
    dest = Image(out_fmt(out_ct), w, h, align=align, device=DEV)
    uhdr.applyGainMapFromCoefficients444(to_dev(coefs), qts, w, h, A.UHDR_CG_BT_709, gm.to(DEV), md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest)
    uhdr.ctx.synchronize()
    return dest.to_host()


# ---- 1. the operator against the oracle ---------------------------------------------------------------------------------------------
# 128 x 8: exactly one 128 x 8 tile (and half of a 128 x 16 one).  130 x 18: a second tile column with two live pixels, a last tile
# row with two live rows, seventeen blocks per row.  392 x 204: a partial last tile in both directions and a last block row half
# used.  256 x 48: whole tiles.  A size is skipped where the scale does not divide it or leaves the map fewer than two rows; 392 x 200
# (a partial last tile column, twenty-five tile rows) is there so that scale 8, which divides only 256 x 48 of the other four with
# two map rows left, still runs two sizes.
SIZES = ((128, 8, 95, 1), (130, 18, 85, 0), (392, 204, 70, 0), (256, 48, 80, 1), (392, 200, 75, 0))


@pytest.mark.parametrize("ch,alpha,scale", [(1, False, 1), (1, False, 2), (1, False, 4), (1, False, 8), (3, False, 1), (3, False, 2), (3, True, 1), (3, True, 2),
                                            (3, True, 4), (3, False, 8)])
@pytest.mark.parametrize("out_ct", [A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ])
def test_operator_equals_the_oracle(uhdr, ch, alpha, scale, out_ct):
    ran = 0
    for (w, h, quality, ubc) in SIZES:
        if w % scale or h % scale or h // scale < 2:
            continue
        coefs, qts, dec = coef_case(w, h, quality)
        gm = synth.make_gainmap(w // scale, h // scale, ch, alpha, cg=A.UHDR_CG_BT_2100)
        md = synth.default_metadata(use_base_cg=ubc, per_channel=(ch == 3))  # the gamut conversion on the HDR side (1) / the SDR side (0)
        want = L.apply_gainmap(oracle_kind(), dec, gm, md, out_ct)
        got = run_coef444(uhdr, coefs, qts, w, h, gm, md, out_ct)
        diff = int((got.valid(0) != want.valid(0)).sum())
        print(f"{w}x{h} ch={ch} alpha={alpha} scale={scale} ct={out_ct}: {diff} differing samples")
        assert diff == 0, (w, h)
        ran += 1
    assert ran >= 2  # the skip rule hides no parameter row


def test_operator_equals_the_oracle_at_a_camera_size(uhdr):
    """1920 x 1080: the height is not a multiple of 16 (an odd number of 128 x 8 tile rows), fifteen tile columns."""
    w, h = 1920, 1080
    coefs, qts, dec = coef_case(w, h, 90)
    gm = synth.make_gainmap(w // 4, h // 4, 1, cg=A.UHDR_CG_BT_2100)
    md = synth.default_metadata(use_base_cg=0)
    want = L.apply_gainmap(oracle_kind(), dec, gm, md, A.UHDR_CT_LINEAR)
    got = run_coef444(uhdr, coefs, qts, w, h, gm, md, A.UHDR_CT_LINEAR)
    assert np.array_equal(got.valid(0), want.valid(0))


# ---- 2. the operator against the library's staged route --------------------------------------------------------------------------------
def staged(uhdr, dcoefs, qts, w, h, gm_dev, md, out_ct):
    """idct_dequant x 3 into a 4:4:4 device image, then applyGainMap (w and h whole blocks, so the planes hold every row written)."""
    assert w % 8 == 0 and h % 8 == 0
    img = Image(Y444, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=16, device=DEV)
    for c in range(3):
        pl = img.plane_tensor(c)
        uhdr.idct_dequant(dcoefs[c], qts[c], plane=pl, stride=pl.shape[1])
    dest = Image(out_fmt(out_ct), w, h, align=4, device=DEV)
    uhdr.applyGainMap(img, gm_dev, md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest)
    uhdr.ctx.synchronize()
    return dest.to_host()


def test_operator_equals_the_staged_route_on_wild_coefficients(uhdr):
    w, h = 256, 48
    coefs, qts, dec = coef_case(w, h, 50, wild=True)
    gm = synth.make_gainmap(w // 4, h // 4, 1)
    md = synth.default_metadata()
    got = run_coef444(uhdr, coefs, qts, w, h, gm, md, A.UHDR_CT_LINEAR)
    want = staged(uhdr, to_dev(coefs), qts, w, h, gm.to(DEV), md, A.UHDR_CT_LINEAR)
    assert np.array_equal(got.valid(0), want.valid(0))
    assert np.array_equal(got.valid(0), L.apply_gainmap(oracle_kind(), dec, gm, md, A.UHDR_CT_LINEAR).valid(0))


# ---- 3. the one-call decode -----------------------------------------------------------------------------------------------------------
def _map_scan(uhdr, mw, mh, nch, seed):
    """A gain map of mw x mh as an entropy-coded scan (one component, or three at 4:4:4): (header, scan bytes on the device,
    coefficients on the device, the two tables)."""
    rng = np.random.default_rng(seed)
    ql, qc = L.quant_table_port(92, False), L.quant_table_port(92, True)
    sampling = S444 if nch == 3 else [(1, 1)]
    dims = grids(mw, mh, sampling)
    dco = to_dev(_smooth_coefs(dims, [ql, qc, qc][:nch], rng))
    scan = uhdr.huffman_encode(dco, mw, mh, sampling, 0)
    return uhdr.jpeg_header(mw, mh, sampling, [ql, qc, qc][:nch]), scan, dco, (ql, qc)


def _decoded_map(uhdr, dco, tables, mw, mh, cg):
    """The image those coefficients decode to, on the host (the library's map IDCT; three channels: ycc -> rgb, alpha 255)."""
    if len(dco) == 3:
        img = uhdr.idct_dequant_rgb(dco, tables[0], tables[1], mw, mh, A.UHDR_IMG_FMT_32bppRGBA8888, 0)
        uhdr.ctx.synchronize()
        img.raw.cg = cg
        return img.to_host()
    plane = uhdr.idct_dequant(dco[0], tables[0])
    uhdr.ctx.synchronize()
    gm = Image(A.UHDR_IMG_FMT_8bppYCbCr400, mw, mh, cg)
    gm.valid(0)[:] = plane.cpu().numpy()[:mh, :mw]
    return gm


@pytest.mark.parametrize("w,h", [(256, 48), (392, 204)])
@pytest.mark.parametrize("nch,scale", [(3, 1), (1, 4)])
def test_one_call_decode_of_a_444_base(uhdr, w, h, nch, scale):
    coefs, qts, dec = coef_case(w, h, 88)
    dco = to_dev(coefs)
    scan_b = uhdr.huffman_encode(dco, w, h, S444, 0)
    hb = uhdr.jpeg_header(w, h, S444, qts)
    mw, mh = w // scale, h // scale
    hm, scan_m, dmap, tables = _map_scan(uhdr, mw, mh, nch, seed=w + nch)
    md = synth.default_metadata(use_base_cg=0, per_channel=(nch == 3))
    base_cg, map_cg = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
    for out_ct in (A.UHDR_CT_LINEAR, A.UHDR_CT_HLG):
        dest = Image(out_fmt(out_ct), w, h, align=64, device=DEV)
        uhdr.decodeApi1ScansAny(hb, scan_b, base_cg, hm, scan_m, map_cg, md, out_ct, out_fmt(out_ct), A.FLT_MAX, dest)
        uhdr.ctx.synchronize()
        got = dest.to_host().valid(0)
        back = uhdr.huffman_decode(scan_b, [(bh, bw) for bw, bh in grids(w, h, S444)], w, h, S444, 0)
        assert all(np.array_equal(b.cpu().numpy(), c) for b, c in zip(back, coefs))
        gm = _decoded_map(uhdr, dmap, tables, mw, mh, map_cg)
        via_op = Image(out_fmt(out_ct), w, h, align=64, device=DEV)
        uhdr.applyGainMapFromCoefficients444(back, qts, w, h, base_cg, gm.to(DEV), md, out_ct, out_fmt(out_ct), A.FLT_MAX, via_op)
        uhdr.ctx.synchronize()
        assert np.array_equal(got, via_op.to_host().valid(0))
        assert np.array_equal(got, L.apply_gainmap(oracle_kind(), dec, gm, md, out_ct).valid(0))


def test_one_call_decode_of_a_real_444_file(uhdr):
    """A file Pillow wrote at 4:4:4 (subsampling=0) as the base image: its own DQT / DHT, parsed by uhdr_hip_jpeg_parse."""
    pytest.importorskip("PIL")
    import torch
    from PIL import Image as PImage

    w, h = 256, 80
    a = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: h // 2] = (a[: h // 2].astype(np.int32) // 64 * 85).astype(np.uint8)  # flat saturated patches
    buf = io.BytesIO()
    PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=90, subsampling=0)
    jpeg = buf.getvalue()
    hb = uhdr.jpeg_parse(jpeg)
    sc = hb.scan
    assert (sc.w, sc.h) == (w, h) and [(sc.h_samp[c], sc.v_samp[c]) for c in range(3)] == S444
    scan_b = torch.from_numpy(np.frombuffer(jpeg, dtype=np.uint8)[hb.scan_offset: hb.scan_offset + hb.scan_bytes].copy()).to(DEV)
    mw, mh = w // 4, h // 4
    hm, scan_m, dmap, tables = _map_scan(uhdr, mw, mh, 1, seed=9)
    md = synth.default_metadata()
    dest = Image(F16, w, h, align=64, device=DEV)
    uhdr.decodeApi1ScansAny(hb, scan_b, A.UHDR_CG_BT_709, hm, scan_m, A.UHDR_CG_BT_709, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest)
    uhdr.ctx.synchronize()
    planes = uhdr.jpeg_decode(jpeg, 0)  # uhdr_hip_jpeg_decode_scan: planar, block padding included
    base = Image(Y444, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    for c in range(3):
        base.valid(c)[:] = planes[c][: base.valid(c).shape[0], : base.valid(c).shape[1]]
    gm = _decoded_map(uhdr, dmap, tables, mw, mh, A.UHDR_CG_BT_709)
    want = Image(F16, w, h, align=64, device=DEV)
    uhdr.applyGainMap(base.to(DEV), gm.to(DEV), md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, want)
    uhdr.ctx.synchronize()
    assert np.array_equal(dest.to_host().valid(0), want.to_host().valid(0))


def test_one_call_decode_falls_back_to_planes_outside_the_quad_contract(uhdr):
    """A scale-3 map is the generic kernel's business: the one-call decode still answers, through the planes route (three IDCT
    launches into a 4:4:4 image), with the oracle's pixels."""
    w, h = 264, 48
    coefs, qts, dec = coef_case(w, h, 80)
    scan_b = uhdr.huffman_encode(to_dev(coefs), w, h, S444, 0)
    hb = uhdr.jpeg_header(w, h, S444, qts)
    mw, mh = w // 3, h // 3
    hm, scan_m, dmap, tables = _map_scan(uhdr, mw, mh, 1, seed=3)
    md = synth.default_metadata()
    dest = Image(F16, w, h, align=64, device=DEV)
    uhdr.decodeApi1ScansAny(hb, scan_b, A.UHDR_CG_BT_709, hm, scan_m, A.UHDR_CG_BT_709, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest)
    uhdr.ctx.synchronize()
    gm = _decoded_map(uhdr, dmap, tables, mw, mh, A.UHDR_CG_BT_709)
    assert np.array_equal(dest.to_host().valid(0), L.apply_gainmap(oracle_kind(), dec, gm, md, A.UHDR_CT_LINEAR).valid(0))


@pytest.mark.parametrize("sampling", [S420, S422])
def test_any_writes_what_the_first_entry_point_writes_for_subsampled_bases(uhdr, sampling):
    w, h = 256, 48
    rng = np.random.default_rng(11)
    qts = [L.quant_table_port(88, False), L.quant_table_port(88, True), L.quant_table_port(78, True)]
    dco = to_dev(_smooth_coefs(grids(w, h, sampling), qts, rng))
    scan_b = uhdr.huffman_encode(dco, w, h, sampling, 0)
    hb = uhdr.jpeg_header(w, h, sampling, qts)
    hm, scan_m, _, _ = _map_scan(uhdr, w // 4, h // 4, 1, seed=21)
    md = synth.default_metadata()
    outs = []
    for fn in (uhdr.decodeApi1Scans, uhdr.decodeApi1ScansAny):
        dest = Image(F16, w, h, align=64, device=DEV)
        fn(hb, scan_b, A.UHDR_CG_BT_709, hm, scan_m, A.UHDR_CG_BT_709, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest)
        uhdr.ctx.synchronize()
        outs.append(dest.to_host().valid(0))
    assert outs[0].any() and np.array_equal(outs[0], outs[1])


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(uhdr):
    import torch

    w, h = 256, 48
    coefs, qts, dec = coef_case(w, h, 88)
    gm = synth.make_gainmap(w // 4, h // 4, 1)
    md = synth.default_metadata()
    d422 = [torch.zeros((bh, bw, 64), dtype=torch.int16, device=DEV) for bw, bh in grids(w, h, S422)]
    dest = Image(F16, w, h, align=2, device=DEV)

    def call(dco, q, ww, hh, g, dst):
        uhdr.applyGainMapFromCoefficients444(dco, q, ww, hh, A.UHDR_CG_BT_709, g.to(DEV), md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dst)

    with pytest.raises(A.UhdrError) as e:  # the block grids of a 4:2:2 frame at the 4:4:4 entry
        call(d422, qts, w, h, gm, dest)
    assert e.value.code == A.UHDR_CODEC_INVALID_PARAM
    w3, h3 = 264, 48  # a 3 x 3 map scale: refused by the operator (no silent fallback)
    c3, q3, _ = coef_case(w3, h3, 80)
    with pytest.raises(A.UhdrError) as e:
        call(to_dev(c3), q3, w3, h3, synth.make_gainmap(w3 // 3, h3 // 3, 1), Image(F16, w3, h3, align=2, device=DEV))
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    wo = 257  # odd width
    co = [torch.zeros((bh, bw, 64), dtype=torch.int16, device=DEV) for bw, bh in grids(wo, h, S444)]
    with pytest.raises(A.UhdrError) as e:
        call(co, qts, wo, h, synth.make_gainmap(wo, h, 1), Image(F16, wo, h, align=2, device=DEV))
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    # the one-call decode: grayscale and 1x2 (4:4:0) base headers stay refused
    qy, qc = uhdr.quant_table(95, False), uhdr.quant_table(95, True)
    data = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    h444 = uhdr.jpeg_header(w, h, S444, [qy, qc, qc])
    dst = Image(F16, w, h, align=64, device=DEV)
    for base in (uhdr.jpeg_header(w, h, [(1, 1)], [qy]), uhdr.jpeg_header(w, h, [(1, 2), (1, 1), (1, 1)], [qy, qc, qc])):
        with pytest.raises(A.UhdrError) as e:
            uhdr.decodeApi1ScansAny(base, data, A.UHDR_CG_BT_709, h444, data, A.UHDR_CG_BT_709, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dst)
        assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    # one good call follows
    got = run_coef444(uhdr, coefs, qts, w, h, gm, md, A.UHDR_CT_LINEAR)
    assert np.array_equal(got.valid(0), L.apply_gainmap(oracle_kind(), dec, gm, md, A.UHDR_CT_LINEAR).valid(0))
