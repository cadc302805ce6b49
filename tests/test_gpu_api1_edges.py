"""GPU: the fused API-1 encode for frames that are not whole MCUs and maps that are not whole blocks (uhdr_hip_encode_api1_fused_edges_dev,
uhdr_hip_encode_api1_scans_edges / _edges_dev).  Every comparison is for equality, against two yardsticks outside the code under test:

  1. the staged public chain -- uhdr_hip_convert_yuv in place on a copy of the SDR intent, uhdr_hip_jpeg_encode_image on its planes with the
     caller's strides (the base scan), uhdr_hip_generate_gainmap / _ex into a zero-filled map of stride ALIGN(mw, 64),
     uhdr_hip_jpeg_encode_image on that map (the map scan), the metadata of that call;
  2. the real reference's compressImage on the same converted planes (one test).

Per case: both scans byte for byte (device and host form), the metadata, the gain-map description, the 8-bit map inside a 0xA5 frame that
stays intact, and the front end's coefficient arrays against the coefficients decoded from the yardstick's scans."""
import ctypes as C
import types

import numpy as np
import pytest

import test_gpu_api1_rgba as R
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P3, UNSPEC = R.P3, R.UNSPEC
S420, RGBA = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_32bppRGBA8888
REALTIME, BEST = A.UHDR_USAGE_REALTIME, A.UHDR_USAGE_BEST_QUALITY
UNSUP, INVAL = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM
FLAG = A.UHDR_HIP_GENERATE_GAMMA_TABLE
GAMMA = 1.571
SAMP420 = R.SAMP420

# (w, h, S).  48 x 40: luma whole blocks, chroma 24 x 20 partial in both directions, h % 16 == 8 (the 1080p pattern of the base image);
# 40 x 48: w % 16 == 8, map 20 x 24; 38 x 26: every plane partial in both directions, luma rows past the height inside an existing block;
# 64 x 56 at 4: map 16 x 14 (1080p's map pattern); 48 x 40 at 4: map 12 x 10; 40 x 8: one MCU row, column mode 1 repeats zeros;
# 280 x 72 at 2 and 296 x 24 at 4: more than one strip of eight map blocks / luma blocks, 18 and 19 MCUs per row (the last pair whole and
# half), a partial last MCU inside a pair; 38 x 6 at 2: one MCU row whose LUMA rows past the height repeat zeros in column mode 1 too (40 x 8
# has whole luma blocks), map 19 x 3
SHAPES = [(48, 40, 1), (40, 48, 2), (38, 26, 1), (64, 56, 4), (48, 40, 4), (40, 8, 1), (280, 72, 2), (296, 24, 4), (38, 6, 2)]
MODES = ["tight", "wide"]  # strides equal to the plane widths / ALIGN(w, 64) with a pattern behind the width


def _config(i, j):
    """Shape i in mode j -> (preset, channels, gamma, hdr kind, base_encoding): the bits of (5 i + 3 j) mod 16 walk through all sixteen
    combinations of the first four."""
    n = (5 * i + 3 * j) % 16
    return (REALTIME if n & 1 else BEST, 3 if n & 2 else 1, GAMMA if n & 4 else 1.0, "1010102" if n & 8 else "p010", P3 if (i + j) % 2 == 0 else UNSPEC)


CASES = [(*s, m, *_config(i, j)) for i, s in enumerate(SHAPES) for j, m in enumerate(MODES)]


def _cdiv(a, b):
    return -(-a // b)


def _intents(w, h, mode, kind):
    align = 1 if mode == "tight" else 64
    sdr = synth.make_sdr_yuv420(w, h, seed=w + 2 * h, noise=0.05, align=align)
    if mode == "wide":  # what sits behind the width is input in column mode 0: make it something no padding rule produces
        for i in range(3):
            pl, wv = sdr.plane(i), sdr.layout[i][2]
            y, x = np.mgrid[0:pl.shape[0], wv:pl.shape[1]]
            pl[:, wv:] = ((x * 7 + y * 13 + 31 * i + 5) & 0xff).astype(np.uint8)
    if kind == "p010":
        hdr = synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=A.UHDR_CT_HLG, noise=0.05, align=align)
    else:
        hdr = synth.make_hdr_rgba1010102(w, h, seed=w + 3 * h, ct=A.UHDR_CT_PQ, noise=0.05, align=align)
    return sdr, hdr


def _staged(hip_ctx, u, sdr, hdr, enc, qb, qm, flags):
    """Yardstick 1: (base scan, map scan, metadata, host map image, the converted SDR image)."""
    w, h = sdr.w, sdr.h
    conv = sdr.clone()
    if enc != UNSPEC:
        u.convertYuv(conv, sdr.raw.cg, enc)
    base = u.jpeg_encode_image([conv.plane(i) for i in range(3)], w, h, SAMP420, qb[0], qb[1])
    md, gm = u.generateGainMapEx(sdr.to(DEV), hdr.to(DEV), flags)  # (a fresh zero-filled device image of stride ALIGN(mw, 64))
    hip_ctx.synchronize()
    gm = gm.to_host()
    assert gm.raw.stride[0] == _cdiv(gm.w, 64) * 64
    if gm.raw.fmt == A.UHDR_IMG_FMT_24bppRGB888:
        mp = u.jpeg_encode_image(gm.plane(0).reshape(gm.h, gm.raw.stride[0], 3), gm.w, gm.h, [(1, 1)] * 3, qm[0], qm[1], rgb_channels=3)
    else:
        mp = u.jpeg_encode_image([gm.plane(0)], gm.w, gm.h, [(1, 1)], qm[0], qm[1])
    return base, mp, md, gm, conv


def _framed_map(nch, mw, mh):
    """A device map image inside a 0xA5 frame: one row above, two below, 3 pixels + 1 byte to the left, an odd pitch."""
    import torch

    stride = mw + 5
    buf = torch.full(((mh + 3) * stride * nch + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.current_stream().synchronize()
    off = (stride + 3) * nch + 1
    raw = A.RawImage()
    raw.planes[0] = buf.data_ptr() + off
    raw.stride[0] = stride
    return types.SimpleNamespace(raw=raw, sync_meta_from_raw=lambda: None), buf, off, stride


def _capacity(blocks):
    return blocks * 416 + 4096  # 1660 bits per block at most, every byte stuffed


@pytest.mark.parametrize("w,h,scale,mode,preset,nch,gamma,kind,enc", CASES)
def test_edges_equal_the_staged_chain(hip_ctx, w, h, scale, mode, preset, nch, gamma, kind, enc):
    import torch

    flags = FLAG if gamma != 1.0 else 0
    u = R._uhdr(hip_ctx, scale, nch == 3, preset=preset, gamma=gamma)
    qb, qm = R._tables()
    sdr, hdr = _intents(w, h, mode, kind)
    mw, mh = w // scale, h // scale
    assert [sdr.raw.stride[i] for i in range(3)] == ([w, w // 2, w // 2] if mode == "tight" else [_cdiv(w, 64) * 64] + [_cdiv(w, 64) * 32] * 2)
    want_b, want_m, md_s, gm_s, conv = _staged(hip_ctx, u, sdr, hdr, enc, qb, qm, flags)
    assert (gm_s.w, gm_s.h) == (mw, mh)
    if mode == "wide" and enc != UNSPEC:  # the pattern behind the width reached the yardstick unconverted
        assert all(np.array_equal(conv.plane(i)[:, conv.layout[i][2]:], sdr.plane(i)[:, sdr.layout[i][2]:]) for i in range(3))
        assert not np.array_equal(conv.valid(0), sdr.valid(0))
    ds, dh = sdr.to(DEV), hdr.to(DEV)

    # the front end: coefficient arrays, metadata, the 8-bit map in its frame
    gm_f, frame, off, stride = _framed_map(nch, mw, mh)
    base_f, map_f, md_f, _ = u.encodeApi1FusedEdges(ds, dh, enc, qb, qm, flags, gm=gm_f)
    hip_ctx.synchronize()
    assert [tuple(t.shape[:2]) for t in base_f] == [(_cdiv(h, 8), _cdiv(w, 8))] + [(_cdiv(h, 16), _cdiv(w, 16))] * 2
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
    dec_b = u.huffman_decode(sb, [tuple(t.shape[:2]) for t in base_f], w, h, SAMP420, 0)
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
    cap_b = _capacity(sum(int(t.shape[0] * t.shape[1]) for t in base_f))
    cap_m = _capacity(sum(int(t.shape[0] * t.shape[1]) for t in map_f))
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


@pytest.mark.parametrize("w,h,mode", [(48, 40, "tight"), (38, 26, "wide"), (40, 8, "tight")])
def test_base_scan_equals_the_reference_encoder(hip_ctx, w, h, mode):
    """Yardstick 2: JpegEncoderHelper::compressImage of the real reference on the converted planes, its entropy-coded bytes."""
    if L.ref() is None:
        pytest.skip("oracle/_ref not built")
    u = R._uhdr(hip_ctx, 1, False, preset=REALTIME)
    sdr, hdr = _intents(w, h, mode, "p010")
    conv = sdr.clone()
    u.convertYuv(conv, sdr.raw.cg, P3)
    jpeg = L.ref_jpeg_compress(conv, 95)
    hd = u.jpeg_parse(jpeg)
    want = jpeg[hd.scan_offset: hd.scan_offset + hd.scan_bytes]
    ql, qc = np.array(hd.qtable[0][:], dtype=np.uint16), np.array(hd.qtable[1][:], dtype=np.uint16)
    cap = _capacity(_cdiv(w, 8) * _cdiv(h, 8) + 2 * _cdiv(w, 16) * _cdiv(h, 16))
    base, mp, md, desc = u.encodeApi1ScansEdges(sdr, hdr, P3, (ql, qc), R._tables()[1], cap, cap, 0)
    assert base == want, f"{len(base)} bytes against the reference's {len(want)}"


@pytest.mark.parametrize("preset", [REALTIME, BEST])
def test_a_whole_mcu_request_is_the_ex_sibling(hip_ctx, preset):
    import torch

    w, h = 144, 48
    sdr = synth.make_sdr_yuv420(w, h, seed=w + 2 * h, noise=0.05)
    hdr = synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=A.UHDR_CT_HLG, noise=0.05)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    u = R._uhdr(hip_ctx, 1, True, preset=preset, gamma=GAMMA)
    n = w * h * 3 + 4096
    outs = [torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(4)]
    nb_a, nm_a, md_a = u.encodeApi1ScansEdges(ds, dh, P3, qb, qm, outs[0], outs[1], FLAG)
    nb_b, nm_b, md_b = u.encodeApi1ScansEx(ds, dh, P3, qb, qm, outs[2], outs[3], FLAG)
    hip_ctx.synchronize()
    assert (nb_a, nm_a) == (nb_b, nm_b) and nb_a > 0 and nm_a > 0 and md_a.as_dict() == md_b.as_dict()
    assert torch.equal(outs[0][:nb_a], outs[2][:nb_b]) and torch.equal(outs[1][:nm_a], outs[3][:nm_b])
    host_a, host_b = u.encodeApi1ScansEdges(sdr, hdr, P3, qb, qm, n, n, FLAG), u.encodeApi1ScansEx(sdr, hdr, P3, qb, qm, n, n, FLAG)
    assert host_a[:2] == host_b[:2] and host_a[2].as_dict() == host_b[2].as_dict()
    assert host_a[0] == outs[0][:nb_a].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def comm_ctx():
    from libultrahdr_amd import stripes
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    assert stripes.init_comm_relay(ctx) == 1
    yield ctx
    ctx.close()


def _send_scans(ctx, u, sdr, hdr, flags, dev):
    """One scans call on raw descriptors -> (status, both outputs still 0xA5 and both sizes 0)."""
    import torch

    qb, qm = R._tables()
    qbb, qmm, cfg, md = u._qt_pair(qb), u._qt_pair(qm), u.encode_cfg(), A.GainmapMetadata()
    n = 1 << 16
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    if dev:
        ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.current_stream().synchronize()
        with ctx.ordered():
            st = ctx.lib.uhdr_hip_encode_api1_scans_edges_dev(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                              C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(ob.data_ptr()), n, C.byref(nb),
                                                              C.c_void_p(om.data_ptr()), n, C.byref(nm), flags)
        ctx.synchronize()
        clean = bool((ob == 0xA5).all()) and bool((om == 0xA5).all())
    else:
        hb, hm = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        st = ctx.lib.uhdr_hip_encode_api1_scans_edges(ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                      C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(hb.ctypes.data), n, C.byref(nb),
                                                      C.c_void_p(hm.ctypes.data), n, C.byref(nm), flags)
        clean = bool((hb == 0xA5).all()) and bool((hm == 0xA5).all())
    return st, clean and (nb.value, nm.value) == (0, 0)


@pytest.mark.parametrize("dev", [True, False])
def test_what_stays_declined(hip_ctx, comm_ctx, dev):
    from libultrahdr_amd.ultrahdr import UltraHdr

    def pair(w, h, rgba=False):
        sdr = synth.make_sdr_rgba8888(w, h, noise=0.05) if rgba else synth.make_sdr_yuv420(w, h, noise=0.05, align=1)
        hdr = synth.make_hdr_p010(w, h, noise=0.05)
        return (sdr.to(DEV), hdr.to(DEV)) if dev else (sdr, hdr)

    u1, u4, u2, u0 = R._uhdr(hip_ctx, 1, True), R._uhdr(hip_ctx, 4, True), R._uhdr(hip_ctx, 2, True), R._uhdr(hip_ctx, 0, True)
    u2r = R._uhdr(hip_ctx, 2, False, preset=REALTIME)
    uc = UltraHdr(ctx=comm_ctx, mapDimensionScaleFactor=1, useMultiChannelGainMap=True, preset=BEST)
    requests = [("RGBA8888 not a multiple of 8", hip_ctx, u1, pair(20, 12, rgba=True), 0, UNSUP, b"multiples of 8"),
                ("a communicator", comm_ctx, uc, pair(48, 40), 0, UNSUP, b"communicator"),
                ("a communicator, whole MCUs", comm_ctx, uc, pair(48, 32), 0, UNSUP, b"communicator"),
                ("too small for the scale factor", hip_ctx, u4, pair(6, 2), 0, UNSUP, b"too small for scale factor 4"),
                ("an odd 4:2:0 frame", hip_ctx, u1, pair(39, 26), 0, UNSUP, b"even dimensions"),
                # (the edge handling, the map's included, is for 4:2:0 intents: 24 x 24 at scale 2 has a 12 x 12 map)
                ("RGBA8888 with a map that is not whole blocks", hip_ctx, u2, pair(24, 24, rgba=True), 0, UNSUP, b"map dimensions that are multiples of 8"),
                ("RGBA8888 with a map that is not whole blocks, one pass", hip_ctx, u2r, pair(24, 24, rgba=True), 0, UNSUP, b"map dimensions that are multiples of 8"),
                ("scale factor 0", hip_ctx, u0, pair(48, 40), 0, INVAL, b"not positive"),
                ("unknown flag bits", hip_ctx, u1, pair(48, 40), 0x12, INVAL, b"flag")]
    for name, ctx, u, (sdr, hdr), flags, code, text in requests:
        st, untouched = _send_scans(ctx, u, sdr, hdr, flags, dev)
        assert st.error_code == code and text in st.detail, (name, st.error_code, st.detail)
        assert untouched, name
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
