"""GPU: the fused API-1 encode for RGBA8888 SDR intents (uhdr_hip_encode_api1_fused_any_dev, uhdr_hip_encode_api1_scans_any and
uhdr_hip_encode_api1_scans_any_dev).  The yardstick is the staged route through operators that are held to the reference elsewhere --
generateGainMap on the RGBA intent, convert_raw_input_to_ycbcr -> convertYuv -> fdct_quant x 3 for the base image, fdct_quant_rgb /
fdct_quant for the map, huffman_encode for the scans -- and every comparison against it is bit for bit.  One test goes to the oracle
chain instead, under the bars of test_gpu_api1_scans.py::test_round_trip_entry_points_equal_the_reference."""
import ctypes as C

import numpy as np
import pytest

import code_lattice as CL
from libultrahdr_amd import capi as A
from libultrahdr_amd import stripes, synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RGBA, S420 = A.UHDR_IMG_FMT_32bppRGBA8888, A.UHDR_IMG_FMT_12bppYCbCr420
P3, BT709, BT2100, UNSPEC = A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100, A.UHDR_CG_UNSPECIFIED
SAMP420, SAMP444 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3
# w, h, scale: one block (seven idle block slots); exactly one full strip; a full strip + one ragged block, two block rows; map 24 x 8
SHAPES = [(8, 8, 1), (64, 8, 1), (72, 16, 1), (96, 32, 4)]
# (sdr gamut, base encoding): two different convertYuv matrices, then the two ways of getting none
GAMUTS = [(BT709, P3), (BT2100, P3), (P3, P3), (BT709, UNSPEC)]
HDRS = ["1010102-pq", "1010102-hlg", "f16"]


def _hdr(kind, w, h, seed, align=64):
    if kind == "1010102-pq":
        return synth.make_hdr_rgba1010102(w, h, seed=seed, ct=A.UHDR_CT_PQ, noise=0.05, align=align)
    if kind == "1010102-hlg":
        return synth.make_hdr_rgba1010102(w, h, seed=seed, ct=A.UHDR_CT_HLG, noise=0.05, align=align)
    return synth.make_hdr_rgba_f16(w, h, seed=seed, noise=0.05, align=align)


def _uhdr(hip_ctx, scale=1, multi=True, **kw):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx, mapDimensionScaleFactor=scale, useMultiChannelGainMap=bool(multi), preset=kw.pop("preset", A.UHDR_USAGE_BEST_QUALITY), **kw)


def _tables():
    return (L.quant_table_port(95, False), L.quant_table_port(95, True)), (L.quant_table_port(90, False), L.quant_table_port(90, True))


def _staged(hip_ctx, u, ds, dh, enc, qb, qm):
    """The staged route on device images: (base coefficients [3], map coefficients [1 or 3], metadata, map image)."""
    w, h = ds.w, ds.h
    md, gm = u.generateGainMap(ds, dh)
    ycc = u.convert_raw_input_to_ycbcr(ds, False)
    assert ycc.raw.fmt == A.UHDR_IMG_FMT_24bppYCbCr444 and ycc.raw.cg == ds.raw.cg
    if enc != UNSPEC:
        u.convertYuv(ycc, ds.raw.cg, enc)
    base = [u.fdct_quant(ycc.plane_tensor(i), ycc.raw.stride[i], w // 8, h // 8, qb[0 if i == 0 else 1]) for i in range(3)]
    if gm.raw.fmt == A.UHDR_IMG_FMT_24bppRGB888:
        mapc = list(u.fdct_quant_rgb(gm, qm[0], qm[1]))
    else:
        mapc = [u.fdct_quant(gm.plane_tensor(0), gm.raw.stride[0], gm.w // 8, gm.h // 8, qm[0])]
    hip_ctx.synchronize()
    return base, mapc, md, gm


def _assert_blocks_equal(got, want, what):
    import torch

    assert len(got) == len(want), what
    for i, (g, s) in enumerate(zip(got, want)):
        assert torch.equal(g, s.reshape(g.shape)), f"{what} component {i}: {int((g != s.reshape(g.shape)).sum())} coefficients differ"


def _planes_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.to_host().planes_valid(), b.to_host().planes_valid()))


# every shape with every gamut pair and both map forms (the HDR intent rotating), then every shape with every HDR intent
FUSED_CASES = [(*s, *g, HDRS[(i + j) % 3], m) for i, s in enumerate(SHAPES) for j, g in enumerate(GAMUTS) for m in (1, 0)] + \
              [(*s, *GAMUTS[0], k, 1) for s in SHAPES for k in HDRS]


@pytest.mark.parametrize("w,h,scale,cg,enc,kind,multi", FUSED_CASES)
def test_fused_any_dev_on_rgba_equals_the_staged_operators(hip_ctx, w, h, scale, cg, enc, kind, multi):
    """All base and map coefficient arrays, the metadata and the optional 8-bit map of uhdr_hip_encode_api1_fused_any_dev equal the
    staged route's, bit for bit; without the map image the coefficients are the same."""
    u = _uhdr(hip_ctx, scale, multi)
    ds = synth.make_sdr_rgba8888(w, h, seed=w + h, cg=cg, noise=0.05).to(DEV)
    dh = _hdr(kind, w, h, seed=3 * w + h).to(DEV)
    qb, qm = _tables()
    base_f, map_f, md_f, gm_f = u.encodeApi1FusedAny(ds, dh, enc, qb, qm, want_map=True)
    base_n, map_n, md_n, gm_n = u.encodeApi1FusedAny(ds, dh, enc, qb, qm, want_map=False)
    hip_ctx.synchronize()
    assert gm_n is None and [tuple(b.shape) for b in base_f] == [(h // 8, w // 8, 64)] * 3
    base_s, map_s, md_s, gm_s = _staged(hip_ctx, u, ds, dh, enc, qb, qm)
    _assert_blocks_equal(base_f, base_s, "base")
    _assert_blocks_equal(map_f, map_s, "map")
    _assert_blocks_equal(base_n, base_s, "base (no map image)")
    _assert_blocks_equal(map_n, map_s, "map (no map image)")
    assert md_f.as_dict() == md_s.as_dict() == md_n.as_dict()
    assert _planes_equal(gm_f, gm_s), "8-bit map"
    assert (gm_f.raw.fmt, gm_f.raw.w, gm_f.raw.h, gm_f.raw.cg, gm_f.raw.ct) == (gm_s.raw.fmt, gm_s.raw.w, gm_s.raw.h, gm_s.raw.cg, gm_s.raw.ct)


@pytest.mark.parametrize("cg,enc", [(BT709, P3), (BT2100, P3), (BT709, UNSPEC)])
def test_fused_base_launch_on_the_code_lattice(hip_ctx, cg, enc):
    """The RGBA8888 lattice image of tests/code_lattice.py -- every code of every channel, the black and white corners -- through the fused
    base launch: both roundings to 8 bits see the full code range."""
    w, h = CL.SIZE_MAIN
    u = _uhdr(hip_ctx)
    ds = CL.sdr(CL.SRGBA, w, h, cg=cg).to(DEV)
    dh = CL.hdr(CL.H1010102, w, h, ct=CL.PQ).to(DEV)
    qb, qm = _tables()
    base_f, map_f, md_f, gm_f = u.encodeApi1FusedAny(ds, dh, enc, qb, qm, want_map=True)
    hip_ctx.synchronize()
    px = ds.to_host().valid(0)
    for sh in (0, 8, 16):
        assert len(np.unique((px >> sh) & 0xff)) == 256
    base_s, map_s, md_s, gm_s = _staged(hip_ctx, u, ds, dh, enc, qb, qm)
    _assert_blocks_equal(base_f, base_s, "base")
    _assert_blocks_equal(map_f, map_s, "map")
    assert md_f.as_dict() == md_s.as_dict() and _planes_equal(gm_f, gm_s)


@pytest.mark.parametrize("w,h,align", [(72, 16, 5), (64, 8, 3)])
def test_rows_that_are_not_16_byte_aligned_are_read_dword_by_dword(hip_ctx, w, h, align):
    """The alignment answer of base_blocks_rgba_kernel: any pitch is taken.  A stride of 75 pixels (300 bytes: three rows in four start
    off a 16-byte boundary) and one of 66 pixels (264 bytes) give the coefficients of the staged route, which reads the same image."""
    u = _uhdr(hip_ctx)
    ds = synth.make_sdr_rgba8888(w, h, seed=9, noise=0.05, align=align).to(DEV)
    assert (ds.raw.stride[0] * 4) % 16 != 0
    dh = _hdr("1010102-pq", w, h, seed=10).to(DEV)
    qb, qm = _tables()
    base_f, map_f, md_f, _ = u.encodeApi1FusedAny(ds, dh, P3, qb, qm, want_map=False)
    hip_ctx.synchronize()
    base_s, map_s, md_s, _ = _staged(hip_ctx, u, ds, dh, P3, qb, qm)
    _assert_blocks_equal(base_f, base_s, "base")
    _assert_blocks_equal(map_f, map_s, "map")
    assert md_f.as_dict() == md_s.as_dict()


def _expected_scans(hip_ctx, u, ds, dh, enc, qb, qm):
    base_s, map_s, md_s, gm_s = _staged(hip_ctx, u, ds, dh, enc, qb, qm)
    eb = u.huffman_encode(base_s, ds.w, ds.h, SAMP444, 0)
    em = u.huffman_encode(map_s, gm_s.w, gm_s.h, [(1, 1)] * len(map_s), 0)
    hip_ctx.synchronize()
    return eb.cpu().numpy().tobytes(), em.cpu().numpy().tobytes(), md_s, gm_s


@pytest.mark.parametrize("w,h,scale,multi,kind", [(72, 16, 1, 1, "1010102-pq"), (96, 32, 4, 1, "f16"), (64, 8, 1, 0, "1010102-hlg"), (8, 8, 1, 1, "1010102-pq")])
def test_scans_any_forms_on_rgba_equal_huffman_encode_of_the_staged_coefficients(hip_ctx, w, h, scale, multi, kind):
    """uhdr_hip_encode_api1_scans_any_dev (device images) and uhdr_hip_encode_api1_scans_any (host images): both scans byte for byte
    huffman_encode of the staged coefficients with a 1x1 / 1x1 / 1x1 base scan, the metadata, the gain-map description."""
    import torch

    u = _uhdr(hip_ctx, scale, multi)
    sdr = synth.make_sdr_rgba8888(w, h, seed=w + 2 * h, noise=0.05)
    hdr = _hdr(kind, w, h, seed=w + 3 * h)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = _tables()
    want_b, want_m, md_s, gm_s = _expected_scans(hip_ctx, u, ds, dh, P3, qb, qm)
    # the base scan is 1x1 / 1x1 / 1x1: it decodes, as such, back to the staged coefficients on three full-resolution grids
    rc, back = L.huffman_decode_port([(h // 8, w // 8)] * 3, w, h, SAMP444, 0, want_b)
    assert rc == 0
    ob = torch.full((w * h * 3 + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    om = torch.full((w * h * 3 + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    nb, nm, md_d = u.encodeApi1ScansAny(ds, dh, P3, qb, qm, ob, om)
    hip_ctx.synchronize()
    assert (nb, nm) == (len(want_b), len(want_m))
    assert ob[:nb].cpu().numpy().tobytes() == want_b, "base scan (device form)"
    assert om[:nm].cpu().numpy().tobytes() == want_m, "map scan (device form)"
    assert md_d.as_dict() == md_s.as_dict()
    base, mp, md_h, desc = u.encodeApi1ScansAny(sdr, hdr, P3, qb, qm, w * h * 3 + 4096, w * h * 3 + 4096)
    assert base == want_b, "base scan (host form)"
    assert mp == want_m, "map scan (host form)"
    assert md_h.as_dict() == md_s.as_dict()
    assert (desc.fmt, desc.w, desc.h, desc.cg, desc.ct, desc.range) == (gm_s.raw.fmt, w // scale, h // scale, hdr.raw.cg, hdr.raw.ct, hdr.raw.range)
    nch = 3 if multi else 1
    rc, mback = L.huffman_decode_port([(h // scale // 8, w // scale // 8)] * nch, desc.w, desc.h, [(1, 1)] * nch, 0, mp)
    assert rc == 0 and len(mback) == nch
    st = A.Stats()
    hip_ctx.lib.uhdr_hip_get_stats(hip_ctx.handle, C.byref(st))
    assert st.last_encode_api1_scans_ns > 0


def test_a_420_intent_through_the_any_forms_gives_what_the_siblings_give(hip_ctx):
    import torch

    w, h = 96, 32
    u = _uhdr(hip_ctx)
    sdr, hdr = synth.make_sdr_yuv420(w, h, seed=4, noise=0.05), synth.make_hdr_p010(w, h, ct=A.UHDR_CT_HLG, seed=5, noise=0.05)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = _tables()
    base_a, map_a, md_a, gm_a = u.encodeApi1FusedAny(ds, dh, P3, qb, qm)
    base_b, map_b, md_b, gm_b = u.encodeApi1Fused(ds, dh, P3, qb, qm)
    hip_ctx.synchronize()
    assert [tuple(b.shape) for b in base_a] == [(h // 8, w // 8, 64), (h // 16, w // 16, 64), (h // 16, w // 16, 64)]
    _assert_blocks_equal(base_a, base_b, "base")
    _assert_blocks_equal(map_a, map_b, "map")
    assert md_a.as_dict() == md_b.as_dict() and _planes_equal(gm_a, gm_b)
    outs = [torch.zeros(w * h * 3 + 4096, dtype=torch.uint8, device=DEV) for _ in range(4)]
    nb_a, nm_a, md_a = u.encodeApi1ScansAny(ds, dh, P3, qb, qm, outs[0], outs[1])
    nb_b, nm_b, md_b = u.encodeApi1Scans(ds, dh, P3, qb, qm, outs[2], outs[3])
    hip_ctx.synchronize()
    assert (nb_a, nm_a) == (nb_b, nm_b) and nb_a > 0 and nm_a > 0 and md_a.as_dict() == md_b.as_dict()
    assert torch.equal(outs[0][:nb_a], outs[2][:nb_b]) and torch.equal(outs[1][:nm_a], outs[3][:nm_b])
    # ... and the host form: the bytes of uhdr_hip_encode_api1_scans
    base, mp, md_h, _ = u.encodeApi1ScansAny(sdr, hdr, P3, qb, qm, w * h * 3 + 4096, w * h * 3 + 4096)
    md_c, nb_c, nm_c = A.GainmapMetadata(), C.c_size_t(0), C.c_size_t(0)
    bb, bm = np.zeros(w * h * 3 + 4096, np.uint8), np.zeros(w * h * 3 + 4096, np.uint8)
    cfg = u.encode_cfg()
    qbb, qmm = u._qt_pair(qb), u._qt_pair(qm)
    A.check(hip_ctx.lib.uhdr_hip_encode_api1_scans(hip_ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                  C.c_void_p(qmm.ctypes.data), C.byref(md_c), None, C.c_void_p(bb.ctypes.data), bb.size, C.byref(nb_c),
                                                  C.c_void_p(bm.ctypes.data), bm.size, C.byref(nm_c)))
    assert base == bb[:nb_c.value].tobytes() == outs[2][:nb_b].cpu().numpy().tobytes()
    assert mp == bm[:nm_c.value].tobytes() and md_h.as_dict() == md_c.as_dict()


def test_host_form_reports_the_sizes_it_needs(hip_ctx):
    """A capacity of 16 bytes: UHDR_CODEC_MEM_ERROR with both needed sizes; a second call with those sizes succeeds with the same bytes."""
    w, h = 72, 16
    u = _uhdr(hip_ctx)
    sdr, hdr = synth.make_sdr_rgba8888(w, h, seed=2, noise=0.05), _hdr("1010102-pq", w, h, seed=3)
    qb, qm = _tables()
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi1ScansAny(sdr, hdr, P3, qb, qm, 16, 16)
    assert e.value.code == A.UHDR_CODEC_MEM_ERROR
    nb, nm = e.value.needed
    assert nb > 16 and nm > 16
    base, mp, md, _ = u.encodeApi1ScansAny(sdr, hdr, P3, qb, qm, nb, nm)
    roomy = u.encodeApi1ScansAny(sdr, hdr, P3, qb, qm, 1 << 16, 1 << 16)
    assert 16 < len(base) <= nb and 16 < len(mp) <= nm and (base, mp) == (roomy[0], roomy[1]) and md.as_dict() == roomy[2].as_dict()


def _new_entry_points_refuse(hip_ctx, u, sdr, hdr, code, ctx=None):
    """All three new entry points answer `code` for these intents and leave every output buffer untouched."""
    import torch

    ctx = ctx or hip_ctx
    lib, w, h = ctx.lib, sdr.w, sdr.h
    qb, qm = _tables()
    qbb, qmm = u._qt_pair(qb), u._qt_pair(qm)
    cfg = u.encode_cfg()
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    n = max(w * h * 3, 4096)
    # fused_any_dev: coefficient buffers sized for the largest layout
    bufs = [torch.full((max(w // 8, 1) * max(h // 8, 1) * 64 + 64,), 0x5A5A, dtype=torch.int16, device=DEV) for _ in range(6)]
    blocks = A.Api1Blocks()
    for i in range(3):
        blocks.base_coef[i], blocks.map_coef[i] = bufs[i].data_ptr(), bufs[3 + i].data_ptr()
    md = A.GainmapMetadata()
    with ctx.ordered():
        st = lib.uhdr_hip_encode_api1_fused_any_dev(ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                    C.c_void_p(qmm.ctypes.data), C.byref(blocks), C.byref(md), None)
    ctx.synchronize()
    assert st.error_code == code, (st.error_code, st.detail)
    assert all(bool((b == 0x5A5A).all()) for b in bufs), "a coefficient buffer was written"
    # scans_any_dev
    ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    with ctx.ordered():
        st = lib.uhdr_hip_encode_api1_scans_any_dev(ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                    C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(ob.data_ptr()), n, C.byref(nb),
                                                    C.c_void_p(om.data_ptr()), n, C.byref(nm))
    ctx.synchronize()
    assert st.error_code == code, (st.error_code, st.detail)
    assert bool((ob == 0xA5).all()) and bool((om == 0xA5).all()) and (nb.value, nm.value) == (0, 0)
    # scans_any
    hb, hm = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
    st = lib.uhdr_hip_encode_api1_scans_any(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                            C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(hb.ctypes.data), n, C.byref(nb),
                                            C.c_void_p(hm.ctypes.data), n, C.byref(nm))
    assert st.error_code == code, (st.error_code, st.detail)
    assert (hb == 0xA5).all() and (hm == 0xA5).all() and (nb.value, nm.value) == (0, 0)


UNSUP, INVAL = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM


@pytest.mark.parametrize("case", ["12x8", "40x40@4", "realtime", "gamma1.3", "rgb888", "ycbcr444", "hdr-size"])
def test_new_entry_points_refuse_what_they_cannot_take(hip_ctx, case):
    w, h, kw, scale, code = 64, 32, {}, 1, UNSUP
    if case == "12x8":
        w, h = 12, 8
    elif case == "40x40@4":  # map 10 x 10
        w, h, scale = 40, 40, 4
    elif case == "realtime":
        kw = dict(preset=A.UHDR_USAGE_REALTIME)
    elif case == "gamma1.3":
        kw = dict(gamma=1.3)
    u = _uhdr(hip_ctx, scale, True, **kw)
    sdr = synth.make_sdr_rgba8888(w, h, seed=1)
    hdr = _hdr("1010102-pq", w, h, seed=2)
    if case == "rgb888":
        sdr = Image(A.UHDR_IMG_FMT_24bppRGB888, w, h, BT709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, 64)
    elif case == "ycbcr444":
        sdr = synth.make_sdr_planar(A.UHDR_IMG_FMT_24bppYCbCr444, w, h)
    elif case == "hdr-size":
        hdr, code = _hdr("1010102-pq", w, h + 8, seed=2), INVAL
    _new_entry_points_refuse(hip_ctx, u, sdr, hdr, code)


def test_new_entry_points_refuse_rgba_on_a_context_with_a_communicator():
    """Row stripes stay 4:2:0: a context with an injected (one-rank, host-relay) communicator refuses an RGBA8888 intent before anything
    is launched or exchanged."""
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    try:
        assert stripes.init_comm_relay(ctx) == 1
        u = _uhdr(ctx)
        _new_entry_points_refuse(ctx, u, synth.make_sdr_rgba8888(64, 32, seed=1), _hdr("1010102-pq", 64, 32, seed=2), UNSUP, ctx=ctx)
    finally:
        ctx.close()


def test_old_entry_points_keep_refusing_rgba(hip_ctx):
    import torch

    w, h = 64, 32
    u = _uhdr(hip_ctx)
    sdr, hdr = synth.make_sdr_rgba8888(w, h, seed=1), _hdr("1010102-pq", w, h, seed=2)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = _tables()
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi1Fused(ds, dh, P3, qb, qm)
    assert e.value.code == UNSUP and "UHDR_IMG_FMT_12bppYCbCr420 base image" in str(e.value)
    ob, om = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi1Scans(ds, dh, P3, qb, qm, ob, om)
    assert e.value.code == UNSUP and "UHDR_IMG_FMT_12bppYCbCr420 base image" in str(e.value)
    md, nb, nm = A.GainmapMetadata(), C.c_size_t(0), C.c_size_t(0)
    hb, hm = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    cfg, qbb, qmm = u.encode_cfg(), u._qt_pair(qb), u._qt_pair(qm)
    st = hip_ctx.lib.uhdr_hip_encode_api1_scans(hip_ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(hb.ctypes.data), hb.size, C.byref(nb),
                                                C.c_void_p(hm.ctypes.data), hm.size, C.byref(nm))
    assert st.error_code == UNSUP and b"UHDR_IMG_FMT_12bppYCbCr420 base image" in st.detail


@pytest.mark.parametrize("w,h", [(72, 16), (96, 32)])
def test_scans_any_on_rgba_against_the_oracle_chain(hip_ctx, w, h):
    """End to end against the oracle's API-1 operators on the same intents (the real reference where oracle/_ref is loadable, the C
    restatement otherwise), under the bars of test_gpu_api1_scans.py::test_round_trip_entry_points_equal_the_reference: the metadata
    equal, and both scans -- decoded to coefficients with the oracle's Huffman decoder -- the FDCT of the oracle's own images; where
    oracle/_ref is loadable also byte for byte what its JpegEncoderHelper writes.  The base coefficients are held to that where the
    oracle's SDR bytes are the device's, which the operator tests require."""
    kind = "ref" if L.ref() is not None else "port"
    u = _uhdr(hip_ctx)
    sdr = synth.make_sdr_rgba8888(w, h, seed=77, noise=0.05)
    hdr = synth.make_hdr_rgba1010102(w, h, seed=77, ct=A.UHDR_CT_PQ, noise=0.05)
    qy, qc = u.quant_table(95, False), u.quant_table(95, True)
    base, mp, md, desc = u.encodeApi1ScansAny(sdr, hdr, P3, (qy, qc), (qy, qc), w * h * 3 + 4096, w * h * 3 + 4096)
    md_o, gm_o = L.generate_gainmap(kind, sdr, hdr, u.encode_cfg())
    for name in ("max_content_boost", "min_content_boost", "gamma", "offset_sdr", "offset_hdr"):
        assert list(getattr(md, name)) == list(getattr(md_o, name)), name
    assert (md.hdr_capacity_min, md.hdr_capacity_max, md.use_base_cg) == (md_o.hdr_capacity_min, md_o.hdr_capacity_max, md_o.use_base_cg)
    ycc_o = L.convert_raw_input_to_ycbcr(kind, sdr, False)
    ycc_o.raw.cg = sdr.raw.cg
    base_o = L.convert_yuv(kind, ycc_o, sdr.raw.cg, P3)
    # the device's own SDR bytes (operators held to the oracle elsewhere)
    dycc = u.convert_raw_input_to_ycbcr(sdr.to(DEV), False)
    u.convertYuv(dycc, sdr.raw.cg, P3)
    hip_ctx.synchronize()
    same_sdr = all(np.array_equal(a, b) for a, b in zip(dycc.to_host().planes_valid(), base_o.planes_valid()))
    print(f"{w}x{h}: oracle ({kind}) SDR bytes {'equal' if same_sdr else 'differ from'} the device's")
    rc, got_b = L.huffman_decode_port([(h // 8, w // 8)] * 3, w, h, SAMP444, 0, base)
    assert rc == 0
    rc, got_m = L.huffman_decode_port([(h // 8, w // 8)] * 3, w, h, SAMP444, 0, mp)
    assert rc == 0
    if same_sdr:
        for i in range(3):
            want = L.fdct_quant_port(np.ascontiguousarray(base_o.valid(i)), w, w // 8, h // 8, qy if i == 0 else qc)
            assert np.array_equal(got_b[i], want), f"base component {i}: {int((got_b[i] != want).sum())} coefficients differ"
    rgb = np.ascontiguousarray(gm_o.valid(0)).reshape(h, w * 3)
    for i, p in enumerate(L.jpeg_rgb_to_ycc_port(rgb, w, w, h)):
        want = L.fdct_quant_port(p, w, w // 8, h // 8, qy if i == 0 else qc)
        assert np.array_equal(got_m[i], want), f"map component {i}: {int((got_m[i] != want).sum())} coefficients differ"
    if kind == "ref":
        jb, jm = L.ref_jpeg_compress(base_o, 95), L.ref_jpeg_compress(gm_o, 95)
        hb, hm = u.jpeg_parse(jb), u.jpeg_parse(jm)
        assert [(hb.scan.h_samp[i], hb.scan.v_samp[i]) for i in range(3)] == SAMP444
        if same_sdr:
            assert base == jb[hb.scan_offset: hb.scan_offset + hb.scan_bytes], "base scan differs from the reference encoder's"
        assert mp == jm[hm.scan_offset: hm.scan_offset + hm.scan_bytes], "gain-map scan differs from the reference encoder's"
