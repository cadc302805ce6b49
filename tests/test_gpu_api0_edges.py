"""GPU: the fused API-0 encode for frames that are not whole MCUs and maps that are not whole blocks (uhdr_hip_encode_api0_scans_edges /
_edges_dev).  Every comparison is for equality against a yardstick outside the code under test: the staged public chain on the same
context, in the reference's situation on this path (jpegr.cpp:179-244) --

  toneMap into a fresh zero-filled image of stride ALIGN(w, 64); for RGB intents convert_raw_input_to_ycbcr into the same kind of image;
  generateGainMap(.., False, False) with the real-time preset into a zero-filled map of stride ALIGN(mw, 64); both images to the host;
  uhdr_hip_jpeg_encode_image on their planes with their own strides, i.e. JpegEncoderHelper::compressYCbCr's column mode 0 reading the
  zeros behind every width (a three-channel map: jpeg_write_scanlines' edge replication).

The yardstick asserts its own strides and zeros.  Per case: both scans byte for byte in host and device form, the metadata, sdr_cg, the
gain-map description, and the device buffers' 0xA5 frame."""
import ctypes as C

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L
from test_gpu_api0_p010 import _uhdr_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P010, RGBA, F16 = A.UHDR_IMG_FMT_24bppYCbCrP010, A.UHDR_IMG_FMT_32bppRGBA1010102, A.UHDR_IMG_FMT_64bppRGBAHalfFloat
S420, S444, RGBA8 = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_24bppYCbCr444, A.UHDR_IMG_FMT_32bppRGBA8888
RGB888, Y400 = A.UHDR_IMG_FMT_24bppRGB888, A.UHDR_IMG_FMT_8bppYCbCr400
HLG, PQ = A.UHDR_CT_HLG, A.UHDR_CT_PQ
GAMUTS = [A.UHDR_CG_BT_709, A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_2100]
FULL, LIMITED = A.UHDR_CR_FULL_RANGE, A.UHDR_CR_LIMITED_RANGE
UNSUP, INVAL, MEM = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM, A.UHDR_CODEC_MEM_ERROR
SAMP420, SAMP444 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3

# (format, w, h, S), the smallest that reach each branch.
# P010 -- 48 x 40: h % 16 == 8, chroma 24 x 20 partial both ways (1080p's base pattern); 40 x 48: w % 16 == 8, a dummy luma block column;
# 38 x 26: every plane partial both ways; 40 x 8: one MCU row; 280 x 72 at 2: more than one 128-pixel front-end tile per row, 18 MCUs;
# 64 x 56 at 4: map 16 x 14 (1080p's map pattern); 48 x 40 at 4: map 12 x 10; 296 x 24 at 4: map 74 x 6.
# RGBA1010102 -- 44 x 36: the 4-pixel kernel, w % 8 == 4; 38 x 26: w % 4 != 0, the one-pixel-per-thread kernel; 268 x 12: two 256-pixel
# tiles; 44 x 36 at 2; 64 x 56 at 4; 268 x 12 at 4: map 67 x 3.  Half float -- 44 x 36 and 38 x 26.
SHAPES = [(P010, 48, 40, 1), (P010, 40, 48, 1), (P010, 38, 26, 1), (P010, 40, 8, 1), (P010, 280, 72, 2), (P010, 64, 56, 4), (P010, 48, 40, 4),
          (P010, 296, 24, 4), (RGBA, 44, 36, 1), (RGBA, 38, 26, 1), (RGBA, 268, 12, 1), (RGBA, 44, 36, 2), (RGBA, 64, 56, 4), (RGBA, 268, 12, 4),
          (F16, 44, 36, 1), (F16, 38, 26, 1)]


def _config(i):
    """Shape i -> (channels, gamma, transfer, gamut, P010 range): the bits of 5 i mod 16 walk through all sixteen combinations of the two-valued
    ones over the sixteen shapes, the gamut goes round its three values."""
    n = (5 * i) % 16
    return (3 if n & 1 else 1, 1.3 if n & 2 else 1.0, PQ if n & 4 else HLG, GAMUTS[i % 3], LIMITED if n & 8 else FULL)


CASES = [(*s, *_config(i)) for i, s in enumerate(SHAPES)]


def _cdiv(a, b):
    return -(-a // b)


def _quant():
    return ((L.quant_table_port(95, False), L.quant_table_port(95, True)), (L.quant_table_port(85, False), L.quant_table_port(85, True)))


def _uhdr(hip_ctx, scale, nch=1, gamma=1.0, preset=A.UHDR_USAGE_REALTIME):
    return _uhdr_for(hip_ctx, A.default_encode_cfg(use_luminance=0, preset=preset, map_dimension_scale_factor=scale,
                                                   use_multi_channel_gainmap=int(nch == 3), gamma=gamma))


def _intent(fmt, w, h, ct=PQ, cg=A.UHDR_CG_BT_2100, rng=FULL, noise=0.05, seed=None):
    seed = w * 7 + h if seed is None else seed
    if fmt == P010:
        return synth.make_hdr_p010(w, h, seed=seed, ct=ct, cg=cg, noise=noise, rng_range=rng)
    if fmt == RGBA:
        return synth.make_hdr_rgba1010102(w, h, seed=seed, ct=ct, cg=cg, noise=noise)
    return synth.make_hdr_rgba_f16(w, h, seed=seed, cg=cg, noise=noise)


def _capacity(fmt, w, h, mw, mh, nch):
    """416 bytes per block hold its 1660 bits at most with every byte stuffed."""
    cdiv = 16 if fmt == P010 else 8
    return ((_cdiv(w, 8) * _cdiv(h, 8) + 2 * _cdiv(w, cdiv) * _cdiv(h, cdiv)) * 416 + 4096, _cdiv(mw, 8) * _cdiv(mh, 8) * nch * 416 + 4096)


def _yardstick(hip_ctx, u, hdr, qb, qm):
    """(base scan, map scan, metadata, host map image, gamut of the rendition) of the staged chain."""
    w, h = hdr.w, hdr.h
    dh = hdr.to(DEV)
    a64 = _cdiv(w, 64) * 64
    if hdr.fmt == P010:
        sdr = Image(S420, w, h, align=64, device=DEV)
        u.toneMap(dh, sdr)
        base, samp, strides = sdr, SAMP420, [a64, a64 // 2, a64 // 2]
    else:
        sdr = Image(RGBA8, w, h, align=64, device=DEV)
        u.toneMap(dh, sdr)
        base, samp, strides = u.convert_raw_input_to_ycbcr(sdr, False), SAMP444, [a64] * 3
    md, gm = u.generateGainMap(sdr, dh, False, False)
    hip_ctx.synchronize()
    base, gm = base.to_host(), gm.to_host()
    # the reference's situation: strides of ALIGN(w, 64) (halved for 4:2:0 chroma) and zeros behind every width
    assert [base.raw.stride[i] for i in range(3)] == strides
    for i in range(3):
        assert base.layout[i][2] == (w if i == 0 or hdr.fmt != P010 else w // 2)
        assert not base.plane(i)[:, base.layout[i][2]:].any(), f"base plane {i}: bytes behind the width"
    nch = 3 if gm.raw.fmt == RGB888 else 1
    assert gm.raw.stride[0] == _cdiv(gm.w, 64) * 64 and not gm.plane(0)[:, gm.w * nch:].any()
    bs = u.jpeg_encode_image([base.plane(i) for i in range(3)], w, h, samp, qb[0], qb[1])
    if nch == 3:
        ms = u.jpeg_encode_image(gm.plane(0).reshape(gm.h, gm.raw.stride[0], 3), gm.w, gm.h, [(1, 1)] * 3, qm[0], qm[1], rgb_channels=3)
    else:
        ms = u.jpeg_encode_image([gm.plane(0)], gm.w, gm.h, [(1, 1)], qm[0], qm[1])
    return bs, ms, md, gm, base.raw.cg


def _desc(r):
    return (r.fmt, r.w, r.h, r.cg, r.ct, r.range)


def _framed(cap):
    """A device buffer of `cap` bytes inside a 0xA5 frame of 32 bytes on either side: (frame, the buffer)."""
    import torch

    frame = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.current_stream().synchronize()
    return frame, frame[32: 32 + cap]


def _frame_intact(frame, cap):
    got = frame.cpu().numpy()
    return bool((got[:32] == 0xA5).all()) and bool((got[32 + cap:] == 0xA5).all())


def _assert_equals_yardstick(hip_ctx, u, hdr, qb, qm, want, what=""):
    want_b, want_m, md_s, gm_s, cg_s = want
    nch = 3 if gm_s.raw.fmt == RGB888 else 1
    cap_b, cap_m = _capacity(hdr.fmt, hdr.w, hdr.h, gm_s.w, gm_s.h, nch)
    base, mp, md, desc, cg = u.encodeApi0ScansEdges(hdr, qb, qm, cap_b, cap_m)
    print(f"{what} host form: base {len(base)} / {len(want_b)} bytes, map {len(mp)} / {len(want_m)} bytes")
    assert base == want_b, f"base scan (host form) {what}"
    assert mp == want_m, f"map scan (host form) {what}"
    assert md.as_dict() == md_s.as_dict() and cg == cg_s == A.UHDR_CG_DISPLAY_P3
    assert _desc(desc) == _desc(gm_s.raw)
    fb, ob = _framed(cap_b)
    fm, om = _framed(cap_m)
    d_base, d_mp, md_d, desc_d, cg_d = u.encodeApi0ScansEdgesDev(hdr.to(DEV), qb, qm, ob, om)
    hip_ctx.synchronize()
    assert d_base.cpu().numpy().tobytes() == want_b, f"base scan (device form) {what}"
    assert d_mp.cpu().numpy().tobytes() == want_m, f"map scan (device form) {what}"
    assert md_d.as_dict() == md_s.as_dict() and cg_d == cg_s and _desc(desc_d) == _desc(gm_s.raw)
    assert _frame_intact(fb, cap_b) and _frame_intact(fm, cap_m), "bytes outside [0, capacity) were written"


@pytest.mark.parametrize("fmt,w,h,scale,nch,gamma,ct,cg,rng", CASES)
def test_edges_equal_the_staged_chain(hip_ctx, fmt, w, h, scale, nch, gamma, ct, cg, rng):
    u = _uhdr(hip_ctx, scale, nch, gamma)
    qb, qm = _quant()
    hdr = _intent(fmt, w, h, ct, cg, rng)
    want = _yardstick(hip_ctx, u, hdr, qb, qm)
    assert (want[3].w, want[3].h) == (w // scale, h // scale) and want[3].raw.fmt == (RGB888 if nch == 3 else Y400)
    _assert_equals_yardstick(hip_ctx, u, hdr, qb, qm, want)
    # the caller's BEST_QUALITY is overridden (jpegr.cpp:207)
    ub = _uhdr(hip_ctx, scale, nch, gamma, preset=A.UHDR_USAGE_BEST_QUALITY)
    cap_b, cap_m = _capacity(fmt, w, h, w // scale, h // scale, nch)
    base, mp, md, _, _ = ub.encodeApi0ScansEdges(hdr, qb, qm, cap_b, cap_m)
    assert (base, mp) == want[:2] and md.as_dict() == want[2].as_dict()


@pytest.mark.parametrize("fmt,w,h,scale,nch", [(P010, 38, 26, 1, 3), (P010, 48, 40, 4, 1), (RGBA, 44, 36, 1, 1), (RGBA, 268, 12, 4, 1), (F16, 38, 26, 1, 1)])
def test_scratch_an_earlier_call_left_dirty_does_not_reach_the_scans(hip_ctx, fmt, w, h, scale, nch):
    """The chain keeps its base planes and its map in context scratch whose pitches cover the block-aligned widths: a larger whole-MCU frame
    of noise goes first, on the same context, so that whatever lies behind the edge case's widths and below its heights is not zero.
    A load past a width would show here."""
    qb, qm = _quant()
    for nfmt in (P010, RGBA):  # (both base layouts: 4:2:0 and 4:4:4 planes; a three-channel full-resolution map)
        noise = _intent(nfmt, 320, 96, noise=1.0, seed=3)
        nb, nm, _, _, _ = _uhdr(hip_ctx, 1, 3).encodeApi0ScansEdges(noise, qb, qm, 1 << 20, 1 << 20)
        assert len(nb) > 320 * 96 // 8 and len(nm) > 64  # (noise: far from an image of zeros)
    u = _uhdr(hip_ctx, scale, nch)
    hdr = _intent(fmt, w, h, PQ, A.UHDR_CG_BT_2100, FULL)
    cap_b, cap_m = _capacity(fmt, w, h, w // scale, h // scale, nch)
    got = u.encodeApi0ScansEdges(hdr, qb, qm, cap_b, cap_m)  # (straight behind the noise: nothing else has used the scratch)
    want = _yardstick(hip_ctx, u, hdr, qb, qm)
    assert got[0] == want[0], "base scan"
    assert got[1] == want[1], "map scan"
    _assert_equals_yardstick(hip_ctx, u, hdr, qb, qm, want, "after the yardstick")


@pytest.mark.parametrize("fmt,scale", [(P010, 1), (RGBA, 1), (F16, 1), (P010, 2), (RGBA, 4)])
def test_a_whole_mcu_request_is_the_scaled_sibling(hip_ctx, fmt, scale):
    w, h = 64, 32
    u = _uhdr(hip_ctx, scale, 3)
    hdr = _intent(fmt, w, h)
    qb, qm = _quant()
    a = u.encodeApi0ScansEdges(hdr, qb, qm, 1 << 16, 1 << 16)
    b = u.encodeApi0ScansScaled(hdr, qb, qm, 1 << 16, 1 << 16)
    assert a[0] == b[0] and a[1] == b[1] and a[2].as_dict() == b[2].as_dict() and a[4] == b[4] and _desc(a[3]) == _desc(b[3])
    assert len(a[0]) > 0 and len(a[1]) > 0
    fb, ob = _framed(1 << 16)
    fm, om = _framed(1 << 16)
    d = u.encodeApi0ScansEdgesDev(hdr.to(DEV), qb, qm, ob, om)
    hip_ctx.synchronize()
    assert d[0].cpu().numpy().tobytes() == b[0] and d[1].cpu().numpy().tobytes() == b[1] and d[2].as_dict() == b[2].as_dict()
    assert _frame_intact(fb, 1 << 16) and _frame_intact(fm, 1 << 16)


@pytest.mark.parametrize("fmt,w,h,scale", [(P010, 48, 40, 1), (RGBA, 268, 12, 4)])
def test_a_small_capacity_reports_both_sizes(hip_ctx, fmt, w, h, scale):
    u = _uhdr(hip_ctx, scale, 1)
    hdr = _intent(fmt, w, h)
    qb, qm = _quant()
    roomy = u.encodeApi0ScansEdges(hdr, qb, qm, 1 << 16, 1 << 16)
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi0ScansEdges(hdr, qb, qm, 64, 64)
    assert e.value.code == MEM
    nb, nm = e.value.needed
    assert nb > 64 and nm > 64
    base, mp, _, _, _ = u.encodeApi0ScansEdges(hdr, qb, qm, nb, nm)
    assert 64 < len(base) <= nb and 64 < len(mp) <= nm and (base, mp) == (roomy[0], roomy[1])
    # the device form: 64-byte buffers inside their frames, then buffers of the reported sizes
    dh = hdr.to(DEV)
    fb, ob = _framed(64)
    fm, om = _framed(64)
    with pytest.raises(A.UhdrError) as e:
        u.encodeApi0ScansEdgesDev(dh, qb, qm, ob, om)
    hip_ctx.synchronize()
    assert e.value.code == MEM and e.value.needed == (nb, nm)
    assert _frame_intact(fb, 64) and _frame_intact(fm, 64)
    fb, ob = _framed(nb)
    fm, om = _framed(nm)
    d = u.encodeApi0ScansEdgesDev(dh, qb, qm, ob, om)
    hip_ctx.synchronize()
    assert d[0].cpu().numpy().tobytes() == roomy[0] and d[1].cpu().numpy().tobytes() == roomy[1]
    assert _frame_intact(fb, nb) and _frame_intact(fm, nm)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _send(ctx, u, hdr, dev, fn=None, nulls=()):
    """One call on raw descriptors -> (status, both outputs still 0xA5 and both sizes 0).  nulls: argument positions sent as NULL."""
    import torch

    qb, qm = _quant()
    qbb, qmm, cfg = u._qt_pair(qb), u._qt_pair(qm), u.encode_cfg(False, False)
    md, desc, cg = A.GainmapMetadata(), A.RawImage(), C.c_int(0)
    n = 1 << 16
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    if dev:
        ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.current_stream().synchronize()
        pb, pm = ob.data_ptr(), om.data_ptr()
    else:
        ob, om = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
        pb, pm = ob.ctypes.data, om.ctypes.data
    args = [ctx.handle, C.byref(hdr.raw), C.byref(cfg), C.c_void_p(qbb.ctypes.data), C.c_void_p(qmm.ctypes.data), C.byref(md), C.byref(desc), C.byref(cg),
            C.c_void_p(pb), n, C.byref(nb), C.c_void_p(pm), n, C.byref(nm)]
    for i in nulls:
        args[i] = None
    fn = fn or (ctx.lib.uhdr_hip_encode_api0_scans_edges_dev if dev else ctx.lib.uhdr_hip_encode_api0_scans_edges)
    with ctx.ordered():
        st = fn(*args)
    ctx.synchronize()
    clean = bool((ob == 0xA5).all()) and bool((om == 0xA5).all())
    return st, clean and (nb.value, nm.value) == (0, 0)


@pytest.fixture(scope="module")
def comm_ctx():
    from libultrahdr_amd import stripes
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    stripes.init_comm_relay(ctx)
    yield ctx
    ctx.lib.uhdr_hip_comm_destroy(ctx.handle)
    ctx.close()


@pytest.mark.parametrize("dev", [False, True])
def test_what_stays_declined(hip_ctx, comm_ctx, dev):
    def intent(fmt, w, h):
        img = _intent(fmt, w, h)
        return img.to(DEV) if dev else img

    u1, u2, u4, u3 = (_uhdr(hip_ctx, s) for s in (1, 2, 4, 3))
    uc = _uhdr(comm_ctx, 1)
    requests = [("an odd width", hip_ctx, u1, intent(RGBA, 39, 26), b"even dimensions"),
                ("an odd height", hip_ctx, u1, intent(F16, 38, 25), b"even dimensions"),
                ("w % 4 at scale factor 2", hip_ctx, u2, intent(P010, 38, 26), b"multiple of 4"),
                ("w % 4 at scale factor 4", hip_ctx, u4, intent(RGBA, 38, 28), b"multiple of 4"),
                ("h % S at scale factor 4", hip_ctx, u4, intent(P010, 40, 26), b"multiple of 4"),
                ("half float at scale factor 2", hip_ctx, u2, intent(F16, 44, 36), b"half-float"),
                ("half float at scale factor 4", hip_ctx, u4, intent(F16, 44, 36), b"half-float"),
                ("too small for the scale factor", hip_ctx, u4, intent(P010, 2, 2), b"too small for scale factor 4"),
                ("scale factor 3", hip_ctx, u3, intent(P010, 48, 42), b"scale factors 1, 2 and 4"),
                ("a communicator", comm_ctx, uc, intent(P010, 48, 40), b"communicator"),
                ("a communicator, whole MCUs", comm_ctx, uc, intent(RGBA, 64, 32), b"communicator")]
    for name, ctx, u, hdr, text in requests:
        st, untouched = _send(ctx, u, hdr, dev)
        assert st.error_code == UNSUP and text in st.detail and b"use the operators" in st.detail, (name, st.error_code, st.detail)
        assert untouched, name
    # null arguments: the context, the intent, the configuration, either table, the metadata, either buffer, either size
    hdr = intent(P010, 48, 40)
    for i in (0, 1, 2, 3, 4, 5, 8, 10, 11, 13):
        st, untouched = _send(hip_ctx, u1, hdr, dev, nulls=(i,))
        assert st.error_code == INVAL and untouched, (i, st.error_code, st.detail)


def test_the_old_entry_points_still_refuse_these_frames(hip_ctx):
    lib = hip_ctx.lib
    for fn in (lib.uhdr_hip_encode_api0_scans, lib.uhdr_hip_encode_api0_scans_any, lib.uhdr_hip_encode_api0_scans_scaled):
        st, untouched = _send(hip_ctx, _uhdr(hip_ctx, 1), _intent(P010, 48, 40), False, fn=fn)
        assert st.error_code == UNSUP and untouched, st.detail
        st, untouched = _send(hip_ctx, _uhdr(hip_ctx, 4), _intent(P010, 64, 56), False, fn=fn)
        assert st.error_code == UNSUP and untouched, st.detail
        st, untouched = _send(hip_ctx, _uhdr(hip_ctx, 4), _intent(RGBA, 64, 56), False, fn=fn)
        assert st.error_code == UNSUP and untouched, st.detail
