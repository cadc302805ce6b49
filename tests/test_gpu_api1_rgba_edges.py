"""GPU: the fused API-1 encode for RGBA8888 SDR intents that are off the block grid, in the frame or in the map
(UHDR_HIP_ENCODE_RGBA_EDGES on uhdr_hip_encode_api1_fused_edges_dev, uhdr_hip_encode_api1_scans_edges / _edges_dev).  Every comparison is
for equality, against two yardsticks outside the code under test:

  1. the staged public chain -- uhdr_hip_convert_raw_input_to_ycbcr into a fresh zero-filled YCbCr 4:4:4 image of stride ALIGN(w, 64),
     uhdr_hip_convert_yuv on it, uhdr_hip_jpeg_encode_image on its three planes (the base scan), uhdr_hip_generate_gainmap_ex into a
     zero-filled map of stride ALIGN(mw, 64), uhdr_hip_jpeg_encode_image on that map (the map scan), the metadata of that call;
  2. the real reference's compressImage on the same converted image (one test).

Per case: the front end's coefficient arrays against the coefficients decoded from the yardstick's scans, the 8-bit map inside a 0xA5
frame that stays intact, the metadata, the gain-map description, both scans byte for byte (device and host form).  The yardstick is always
computed from the intent at its tight pitch: a wider pitch with a pattern behind the width must change nothing."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_api1_edges as E
import test_gpu_api1_rgba as R
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from oracle import loader as L
from test_gpu_api1_edges import comm_ctx  # noqa: F401  (the fixture: a context with a communicator)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P3, UNSPEC = R.P3, R.UNSPEC
REALTIME, BEST = A.UHDR_USAGE_REALTIME, A.UHDR_USAGE_BEST_QUALITY
UNSUP, INVAL, OK = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM, A.UHDR_CODEC_OK
TABLE, EDGES = A.UHDR_HIP_GENERATE_GAMMA_TABLE, A.UHDR_HIP_ENCODE_RGBA_EDGES
GAMMA = E.GAMMA
SAMP444 = R.SAMP444
_cdiv = E._cdiv

# (w, h, S).  64 x 56 at 4: base whole blocks, map 16 x 14 (1080p's pattern: only the map is partial); 48 x 36 at 4: h % 8 == 4, map 12 x 9;
# 44 x 40: w % 8 == 4, partial columns in base and map; 37 x 27: odd both ways (RGBA1010102 / half-float HDR only); 140 x 20 at 2: 17.5 blocks
# per row -- three strips, the last one two blocks with the second partial --, map 70 x 10; 264 x 24 at 4: base whole, map 66 x 6 -- nine map
# blocks per row, a second strip of one partial block; 6 x 6: one block, partial both ways; 8 x 3: whole width, rows past the height only
SHAPES = [(64, 56, 4), (48, 36, 4), (44, 40, 1), (37, 27, 1), (140, 20, 2), (264, 24, 4), (6, 6, 1), (8, 3, 1)]
# pitch in pixels: w; ALIGN(w, 64) with a pattern behind the width; w + 1 (rows that are not 16-byte aligned: the dword-load instantiation)
MODES = ["tight", "wide", "plus1"]
KINDS = ["1010102", "f16", "p010"]


def _config(i, j, w, h):
    """Shape i in mode j -> (preset, channels, gamma, hdr kind, base_encoding): the bits of (5 i + 3 j) mod 8 walk through all eight
    combinations of the first three, three times over; the HDR kind rotates, P010 on even shapes only."""
    n = (5 * i + 3 * j) % 8
    kind = KINDS[(i + 2 * j) % 3]
    if kind == "p010" and (w % 2 or h % 2):
        kind = "1010102"
    return (REALTIME if n & 1 else BEST, 3 if n & 2 else 1, GAMMA if n & 4 else 1.0, kind, P3 if (i + j) % 2 == 0 else UNSPEC)


CASES = [(*s, m, *_config(i, j, s[0], s[1])) for i, s in enumerate(SHAPES) for j, m in enumerate(MODES)]


def _sdr(w, h, mode):
    align = {"tight": 1, "wide": 64, "plus1": w + 1}[mode]
    sdr = synth.make_sdr_rgba8888(w, h, seed=w + 2 * h, noise=0.05, align=align)
    stride = sdr.raw.stride[0]
    assert stride == {"tight": w, "wide": _cdiv(w, 64) * 64, "plus1": w + 1}[mode]
    if stride > w:  # nothing behind the width is input: make it something no padding rule produces
        pl = sdr.plane(0)
        y, x = np.mgrid[0:h, w:stride]
        pl[:, w:] = ((x * 7 + y * 13 + 5) & 0xff).astype(np.uint32) * 0x01010101
    return sdr


def _hdr(w, h, kind):
    if kind == "p010":
        return synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=A.UHDR_CT_HLG, noise=0.05)
    if kind == "f16":
        return synth.make_hdr_rgba_f16(w, h, seed=w + 3 * h, noise=0.05)
    return synth.make_hdr_rgba1010102(w, h, seed=w + 3 * h, ct=A.UHDR_CT_PQ, noise=0.05)


def _staged(hip_ctx, u, sdr, hdr, enc, qb, qm, flags):
    """Yardstick 1 on the tight intent: (base scan, map scan, metadata, host map image, the converted YCbCr 4:4:4 image)."""
    w, h = sdr.w, sdr.h
    ycc = u.convert_raw_input_to_ycbcr(sdr, False)
    aw = _cdiv(w, 64) * 64
    assert ycc.raw.fmt == A.UHDR_IMG_FMT_24bppYCbCr444 and [ycc.raw.stride[i] for i in range(3)] == [aw] * 3
    if enc != UNSPEC:
        u.convertYuv(ycc, sdr.raw.cg, enc)
    assert all(not ycc.plane(i)[:, w:].any() for i in range(3)), "the yardstick's image is zero behind the width"
    base = u.jpeg_encode_image([ycc.plane(i) for i in range(3)], w, h, SAMP444, qb[0], qb[1])
    md, gm = u.generateGainMapEx(sdr.to(DEV), hdr.to(DEV), flags)  # (a fresh zero-filled device image of stride ALIGN(mw, 64))
    hip_ctx.synchronize()
    gm = gm.to_host()
    assert gm.raw.stride[0] == _cdiv(gm.w, 64) * 64
    if gm.raw.fmt == A.UHDR_IMG_FMT_24bppRGB888:
        mp = u.jpeg_encode_image(gm.plane(0).reshape(gm.h, gm.raw.stride[0], 3), gm.w, gm.h, [(1, 1)] * 3, qm[0], qm[1], rgb_channels=3)
    else:
        mp = u.jpeg_encode_image([gm.plane(0)], gm.w, gm.h, [(1, 1)], qm[0], qm[1])
    return base, mp, md, gm, ycc


@pytest.mark.parametrize("w,h,scale,mode,preset,nch,gamma,kind,enc", CASES)
def test_rgba_edges_equal_the_staged_chain(hip_ctx, w, h, scale, mode, preset, nch, gamma, kind, enc):
    import torch

    flags = EDGES | (TABLE if gamma != 1.0 else 0)
    u = R._uhdr(hip_ctx, scale, nch == 3, preset=preset, gamma=gamma)
    qb, qm = R._tables()
    tight, hdr = _sdr(w, h, "tight"), _hdr(w, h, kind)
    sdr = tight if mode == "tight" else _sdr(w, h, mode)
    assert np.array_equal(sdr.valid(0), tight.valid(0))
    mw, mh = w // scale, h // scale
    want_b, want_m, md_s, gm_s, _ = _staged(hip_ctx, u, tight, hdr, enc, qb, qm, flags & TABLE)
    assert (gm_s.w, gm_s.h) == (mw, mh)
    ds, dh = sdr.to(DEV), hdr.to(DEV)

    # the front end: coefficient arrays, metadata, the 8-bit map in its frame
    gm_f, frame, off, stride = E._framed_map(nch, mw, mh)
    base_f, map_f, md_f, _ = u.encodeApi1FusedEdges(ds, dh, enc, qb, qm, flags, gm=gm_f)
    hip_ctx.synchronize()
    assert [tuple(t.shape[:2]) for t in base_f] == [(_cdiv(h, 8), _cdiv(w, 8))] * 3
    assert [tuple(t.shape[:2]) for t in map_f] == [(_cdiv(mh, 8), _cdiv(mw, 8))] * nch
    assert md_f.as_dict() == md_s.as_dict()
    assert (gm_f.raw.fmt, gm_f.raw.w, gm_f.raw.h, gm_f.raw.cg, gm_f.raw.ct, gm_f.raw.range) == \
           (gm_s.raw.fmt, mw, mh, hdr.raw.cg, hdr.raw.ct, hdr.raw.range)
    got = frame.cpu().numpy()
    rows = got[off: off + mh * stride * nch].reshape(mh, stride * nch)
    assert np.array_equal(rows[:, : mw * nch], gm_s.valid(0)), "map bytes"
    rest = got.copy()
    rest[off: off + mh * stride * nch].reshape(mh, stride * nch)[:, : mw * nch] = 0xA5
    assert (rest == 0xA5).all(), "bytes beside the map were written"
    sb = torch.from_numpy(np.frombuffer(want_b, np.uint8).copy()).to(DEV)
    sm = torch.from_numpy(np.frombuffer(want_m, np.uint8).copy()).to(DEV)
    dec_b = u.huffman_decode(sb, [tuple(t.shape[:2]) for t in base_f], w, h, SAMP444, 0)
    dec_m = u.huffman_decode(sm, [tuple(t.shape[:2]) for t in map_f], mw, mh, [(1, 1)] * nch, 0)
    hip_ctx.synchronize()
    for i in range(3):
        assert torch.equal(base_f[i], dec_b[i]), f"base component {i}: {int((base_f[i] != dec_b[i]).sum())} coefficients differ"
    for i in range(nch):
        assert torch.equal(map_f[i], dec_m[i]), f"map component {i}: {int((map_f[i] != dec_m[i]).sum())} coefficients differ"
    # without the map image: the same coefficients
    base_n, map_n, md_n, none = u.encodeApi1FusedEdges(ds, dh, enc, qb, qm, flags, want_map=False)
    hip_ctx.synchronize()
    assert none is None and md_n.as_dict() == md_s.as_dict()
    assert all(torch.equal(a, b) for a, b in zip(base_n + map_n, base_f + map_f))

    # the scans forms, capacities from block counts
    cap_b = E._capacity(sum(int(t.shape[0] * t.shape[1]) for t in base_f))
    cap_m = E._capacity(sum(int(t.shape[0] * t.shape[1]) for t in map_f))
    ob, om = torch.full((cap_b,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((cap_m,), 0xA5, dtype=torch.uint8, device=DEV)
    nb, nm, md_d = u.encodeApi1ScansEdges(ds, dh, enc, qb, qm, ob, om, flags)
    hip_ctx.synchronize()
    assert (nb, nm) == (len(want_b), len(want_m))
    assert ob[:nb].cpu().numpy().tobytes() == want_b, "base scan (device form)"
    assert om[:nm].cpu().numpy().tobytes() == want_m, "map scan (device form)"
    assert md_d.as_dict() == md_s.as_dict()
    base, mp, md_h, desc = u.encodeApi1ScansEdges(sdr, hdr, enc, qb, qm, cap_b, cap_m, flags)
    assert base == want_b, "base scan (host form)"
    assert mp == want_m, "map scan (host form)"
    assert md_h.as_dict() == md_s.as_dict()
    assert (desc.fmt, desc.w, desc.h, desc.cg, desc.ct, desc.range) == (gm_s.raw.fmt, mw, mh, hdr.raw.cg, hdr.raw.ct, hdr.raw.range)


@pytest.mark.parametrize("w,h", [(44, 40), (37, 27), (8, 3)])
def test_base_scan_equals_the_reference_encoder(hip_ctx, w, h):
    """Yardstick 2: JpegEncoderHelper::compressImage of the real reference on the staged chain's converted YCbCr 4:4:4 image -- the
    zero-filled one of stride ALIGN(w, 64) --, its entropy-coded bytes under its own quantisation tables."""
    if L.ref() is None:
        pytest.skip("oracle/_ref not built")
    u = R._uhdr(hip_ctx, 1, False, preset=REALTIME)
    sdr, hdr = _sdr(w, h, "tight"), _hdr(w, h, "1010102")
    ycc = u.convert_raw_input_to_ycbcr(sdr, False)
    u.convertYuv(ycc, sdr.raw.cg, P3)
    assert ycc.raw.stride[0] == _cdiv(w, 64) * 64 and not ycc.plane(0)[:, w:].any()
    jpeg = L.ref_jpeg_compress(ycc, 95)
    hd = u.jpeg_parse(jpeg)
    want = jpeg[hd.scan_offset: hd.scan_offset + hd.scan_bytes]
    ql, qc = np.array(hd.qtable[0][:], dtype=np.uint16), np.array(hd.qtable[1][:], dtype=np.uint16)
    cap = E._capacity(3 * _cdiv(w, 8) * _cdiv(h, 8))
    base, mp, md, desc = u.encodeApi1ScansEdges(sdr, hdr, P3, (ql, qc), R._tables()[1], cap, cap, EDGES)
    assert base == want, f"{len(base)} bytes against the reference's {len(want)}"


@pytest.mark.parametrize("preset", [REALTIME, BEST])
def test_a_whole_block_request_is_the_request_without_the_flag(hip_ctx, preset):
    import torch

    w, h = 144, 48
    sdr, hdr = _sdr(w, h, "tight"), _hdr(w, h, "1010102")
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    u = R._uhdr(hip_ctx, 1, True, preset=preset, gamma=GAMMA)
    n = w * h * 3 + 4096
    outs = [torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(4)]
    nb_a, nm_a, md_a = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, outs[0], outs[1], TABLE | EDGES)
    nb_b, nm_b, md_b = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, outs[2], outs[3], TABLE)
    hip_ctx.synchronize()
    assert (nb_a, nm_a) == (nb_b, nm_b) and nb_a > 0 and nm_a > 0 and md_a.as_dict() == md_b.as_dict()
    assert torch.equal(outs[0][:nb_a], outs[2][:nb_b]) and torch.equal(outs[1][:nm_a], outs[3][:nm_b])
    host_a, host_b = u.encodeApi1ScansEdges(sdr, hdr, P3, qb, qm, n, n, TABLE | EDGES), u.encodeApi1ScansEdges(sdr, hdr, P3, qb, qm, n, n, TABLE)
    assert host_a[:2] == host_b[:2] and host_a[2].as_dict() == host_b[2].as_dict()
    assert host_a[0] == outs[0][:nb_a].cpu().numpy().tobytes()


def test_a_420_intent_ignores_the_flag(hip_ctx):
    import torch

    w, h = 38, 26
    sdr = synth.make_sdr_yuv420(w, h, seed=w + 2 * h, noise=0.05, align=1)
    hdr = synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=A.UHDR_CT_HLG, noise=0.05)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    u = R._uhdr(hip_ctx, 1, True)
    outs = [torch.zeros(1 << 16, dtype=torch.uint8, device=DEV) for _ in range(4)]
    nb_a, nm_a, md_a = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, outs[0], outs[1], EDGES)
    nb_b, nm_b, md_b = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, outs[2], outs[3], 0)
    hip_ctx.synchronize()
    assert (nb_a, nm_a) == (nb_b, nm_b) and nb_a > 0 and nm_a > 0 and md_a.as_dict() == md_b.as_dict()
    assert torch.equal(outs[0][:nb_a], outs[2][:nb_b]) and torch.equal(outs[1][:nm_a], outs[3][:nm_b])


def _send_ex(ctx, u, sdr, hdr, flags, dev):
    """_send_scans of the sibling test on the _ex entry points."""
    import torch

    qb, qm = R._tables()
    qbb, qmm, cfg, md = u._qt_pair(qb), u._qt_pair(qm), u.encode_cfg(), A.GainmapMetadata()
    n = 1 << 16
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    if dev:
        ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.current_stream().synchronize()
        with ctx.ordered():
            st = ctx.lib.uhdr_hip_encode_api1_scans_ex_dev(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                           C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(ob.data_ptr()), n, C.byref(nb),
                                                           C.c_void_p(om.data_ptr()), n, C.byref(nm), flags)
        ctx.synchronize()
        clean = bool((ob == 0xA5).all()) and bool((om == 0xA5).all())
    else:
        hb, hm = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        st = ctx.lib.uhdr_hip_encode_api1_scans_ex(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                   C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(hb.ctypes.data), n, C.byref(nb),
                                                   C.c_void_p(hm.ctypes.data), n, C.byref(nm), flags)
        clean = bool((hb == 0xA5).all()) and bool((hm == 0xA5).all())
    return st, clean and (nb.value, nm.value) == (0, 0)


@pytest.mark.parametrize("dev", [True, False])
def test_what_stays_declined_with_the_flag(hip_ctx, comm_ctx, dev):  # noqa: F811
    from libultrahdr_amd.ultrahdr import UltraHdr

    def pair(w, h, kind="1010102"):
        sdr, hdr = _sdr(w, h, "tight"), _hdr(w, h, kind)
        return (sdr.to(DEV), hdr.to(DEV)) if dev else (sdr, hdr)

    u1, u8, u0 = R._uhdr(hip_ctx, 1, True), R._uhdr(hip_ctx, 8, True), R._uhdr(hip_ctx, 0, True)
    uc = UltraHdr(ctx=comm_ctx, mapDimensionScaleFactor=1, useMultiChannelGainMap=True, preset=BEST)
    requests = [("a communicator", comm_ctx, uc, pair(44, 40), EDGES, UNSUP, b"communicator"),
                ("too small for the scale factor", hip_ctx, u8, pair(6, 6), EDGES, UNSUP, b"too small for scale factor 8"),
                ("scale factor 0", hip_ctx, u0, pair(44, 40), EDGES, INVAL, b"not positive"),
                ("an unknown flag bit beside the flag", hip_ctx, u1, pair(44, 40), EDGES | 0x10, INVAL, b"flag")]
    for name, ctx, u, (sdr, hdr), flags, code, text in requests:
        st, untouched = E._send_scans(ctx, u, sdr, hdr, flags, dev)
        assert st.error_code == code and text in st.detail, (name, st.error_code, st.detail)
        assert untouched, name
    # the _ex siblings share the flag check and keep the bit unknown
    st, untouched = _send_ex(hip_ctx, u1, *pair(48, 40), EDGES, dev)
    assert st.error_code == INVAL and b"flag" in st.detail and untouched, (st.error_code, st.detail)
    # the front end declines the same requests
    if dev:
        import torch

        coef = torch.zeros(1 << 16, dtype=torch.int16, device=DEV)
        for name, ctx, u, (sdr, hdr), flags, code, text in requests:
            blocks = A.Api1Blocks()
            for i in range(3):
                blocks.base_coef[i] = blocks.map_coef[i] = coef.data_ptr()
            qb, qm = R._tables()
            qbb, qmm, cfg, md = u._qt_pair(qb), u._qt_pair(qm), u.encode_cfg(), A.GainmapMetadata()
            with ctx.ordered():
                st = ctx.lib.uhdr_hip_encode_api1_fused_edges_dev(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                                  C.c_void_p(qmm.ctypes.data), C.byref(blocks), C.byref(md), None, flags)
            ctx.synchronize()
            assert st.error_code == code and text in st.detail, (name, st.error_code, st.detail)
            assert not bool(coef.any()), name


@pytest.mark.parametrize("dev", [True, False])
def test_an_odd_frame_with_a_p010_intent_gets_the_operators_answer(hip_ctx, dev):
    """The chain adds no parity rule of its own.  uhdr_hip_generate_gainmap takes an odd RGBA8888 frame with a P010 HDR intent (P010 views of
    ceil(w / 2) chroma pairs and ceil(h / 2) chroma rows: the call below raises otherwise), so the chain takes it too, and its scans and
    metadata are the staged chain's."""
    w, h = 37, 27
    u = R._uhdr(hip_ctx, 1, True)
    sdr, hdr = _sdr(w, h, "tight"), _hdr(w, h, "p010")
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    u.generateGainMapEx(ds, dh, 0)  # the operators' status: OK
    hip_ctx.synchronize()
    st, _ = E._send_scans(hip_ctx, u, *((ds, dh) if dev else (sdr, hdr)), EDGES, dev)
    assert st.error_code == OK, (st.error_code, st.detail)
    qb, qm = R._tables()
    want_b, want_m, md_s, _, _ = _staged(hip_ctx, u, sdr, hdr, P3, qb, qm, 0)
    if dev:
        import torch

        ob, om = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
        nb, nm, md = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, ob, om, EDGES)
        hip_ctx.synchronize()
        got_b, got_m = ob[:nb].cpu().numpy().tobytes(), om[:nm].cpu().numpy().tobytes()
    else:
        got_b, got_m, md, _ = u.encodeApi1ScansEdges(sdr, hdr, P3, qb, qm, 1 << 16, 1 << 16, EDGES)
    assert got_b == want_b and got_m == want_m and md.as_dict() == md_s.as_dict()
