"""GPU: 4:2:2 JPEG -> RGB888 / RGBA8888 on the device, libjpeg-exact (uhdr_hip_idct_upsample_rgb422_dev and the whole-file
uhdr_hip_jpeg_decode_rgb_any).  Checked bit for bit against the numpy restatements of tests/upsample422_port.py, against
Pillow's libjpeg-turbo (variant 0) and against oracle/_ref's IJG libjpeg 9 (variant 1)."""
import ctypes as C
import io

import numpy as np
import pytest

import upsample422_port as U
from libultrahdr_amd import capi as A
from oracle import loader as L
from test_upsample422_port import grids_422, impulse_chroma_422, pillow_422, synthetic_422
from test_upsample_port import pillow_420, ref_rgb

pytestmark = pytest.mark.gpu

FMT = {3: A.UHDR_IMG_FMT_24bppRGB888, 4: A.UHDR_IMG_FMT_32bppRGBA8888}
# 1x1 .. 5x3: the cw <= 2 replication boundary on both sides; 17x9: odd width, the last real chroma column is not the last
# IDCT column; 37x23: a partial 32x16 tile both ways; 100x60, 333x211: RGB888 pitches that break the 8-byte vector store;
# 1283x721, 3840x2160: the grid-stride loop wraps
DEV_SIZES = [(1, 1), (2, 2), (4, 4), (5, 3), (17, 9), (37, 23), (100, 60), (333, 211), (1283, 721), (3840, 2160)]


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def _pixels(img, w, h, ch):
    return np.ascontiguousarray(img.to_host().valid(0)).view(np.uint8).reshape(h, w, ch)


def _dense_coefs(rng, w, h):
    """Smooth-ish content: a DC field plus small random AC, so the samples sit around the legal range and clamp now and then."""
    out = []
    for bh, bw in grids_422(w, h):
        c = rng.integers(-3, 4, (bh, bw, 64)).astype(np.int16)
        c[..., 0] = rng.integers(-60, 61, (bh, bw))
        out.append(c)
    return out


@pytest.mark.parametrize("w,h", DEV_SIZES)
@pytest.mark.parametrize("variant", [0, 1])
def test_dev_entry_equals_the_ports(uhdr, w, h, variant):
    import torch

    rng = np.random.default_rng(w * 31 + h + variant)
    coefs = _dense_coefs(rng, w, h)
    qts = [L.quant_table_port(75, False), L.quant_table_port(75, True), L.quant_table_port(60, True)]  # Cb and Cr tables differ
    want = {ch: U.decode422_rgb(coefs, qts, w, h, variant, ch) for ch in (3, 4)}
    dev = [torch.from_numpy(c).to("cuda:0") for c in coefs]
    for ch in (3, 4):
        img = uhdr.idct_upsample_rgb422(dev, qts, w, h, FMT[ch], variant)
        uhdr.ctx.synchronize()
        got = _pixels(img, w, h, ch)
        assert np.array_equal(got, want[ch]), (ch, int((got != want[ch]).any(-1).sum()))


def test_dev_entry_on_chroma_impulses(uhdr):
    """All 64 positions; variant 1 at baseline's extreme amplitude needs the 8-point column pass in more than 32 bits."""
    import torch

    w, h = 128, 64  # 8 x 8 chroma blocks: every position once
    rng = np.random.default_rng(3)
    for amp, q in ((1, 7), (1023, 255)):
        cb, cr = impulse_chroma_422(w, h, amp)
        coefs = [rng.integers(-3, 4, grids_422(w, h)[0] + (64,)).astype(np.int16), cb, cr]
        qts = [L.quant_table_port(90, False), np.full(64, q, np.uint16), np.full(64, q, np.uint16)]
        for variant in (0, 1):
            img = uhdr.idct_upsample_rgb422([torch.from_numpy(c).to("cuda:0") for c in coefs], qts, w, h, FMT[4], variant)
            uhdr.ctx.synchronize()
            assert np.array_equal(_pixels(img, w, h, 4), U.decode422_rgb(coefs, qts, w, h, variant, 4)), (amp, variant)


def test_dev_entry_refuses_bad_arguments_and_the_context_stays_usable(uhdr):
    import torch

    from libultrahdr_amd.images import Image

    w, h = 37, 23
    rng = np.random.default_rng(4)
    coefs = _dense_coefs(rng, w, h)
    dev = [torch.from_numpy(c).to("cuda:0") for c in coefs]
    qts = [L.quant_table_port(75, False), L.quant_table_port(75, True), L.quant_table_port(60, True)]
    q = [(C.c_uint16 * 64)(*[int(v) for v in t]) for t in qts]
    zero = (C.c_uint16 * 64)(*([0] + [1] * 63))
    ptrs = [C.c_void_p(c.data_ptr()) for c in dev]
    fn = uhdr.lib.uhdr_hip_idct_upsample_rgb422_dev
    dst = Image(FMT[4], w, h, align=64, device="cuda:0")
    assert fn(uhdr.ctx.handle, *ptrs, w, h, *q, 2, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM  # variant
    assert fn(uhdr.ctx.handle, *ptrs, w, h, q[0], zero, q[2], 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM  # zero table entry
    assert fn(uhdr.ctx.handle, *ptrs, 0, h, *q, 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM
    assert fn(uhdr.ctx.handle, *ptrs, 65536, h, *q, 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM
    assert fn(uhdr.ctx.handle, *ptrs, w + 1, h, *q, 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM  # destination of another size
    assert fn(uhdr.ctx.handle, ptrs[0], C.c_void_p(dev[1].data_ptr() + 2), ptrs[2], w, h, *q, 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM
    assert fn(uhdr.ctx.handle, None, ptrs[1], ptrs[2], w, h, *q, 0, C.byref(dst.raw)).error_code == A.UHDR_CODEC_INVALID_PARAM
    planar = Image(A.UHDR_IMG_FMT_24bppYCbCr444, w, h, align=64, device="cuda:0")
    assert fn(uhdr.ctx.handle, *ptrs, w, h, *q, 0, C.byref(planar.raw)).error_code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    img = uhdr.idct_upsample_rgb422(dev, qts, w, h, FMT[3], 1)
    uhdr.ctx.synchronize()
    assert np.array_equal(_pixels(img, w, h, 3), U.decode422_rgb(coefs, qts, w, h, 1, 3))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (37, 23), (200, 136), (1283, 721)])
def test_whole_file_equals_pillows_libjpeg_turbo(uhdr, ref, w, h):
    from PIL import Image as PImage, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(w + 7 * h)
    for quality in (30, 90):
        jpeg = pillow_422(rng, w, h, quality)
        want = np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))
        assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 3, 0), want)
        assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 4, 0)[..., :3], want)
    for ri in (0, 7):  # restart markers take the interval decoder
        ql, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
        jpeg, _ = synthetic_422(rng, w, h, 6, ql, qc, restart_interval=ri)
        assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 3, 0), np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))), ri


@pytest.mark.parametrize("w,h", [(2, 2), (17, 9), (200, 136), (1283, 721)])
def test_whole_file_equals_ijg9(uhdr, ref, w, h):
    rng = np.random.default_rng(w + 5 * h)
    jpeg = pillow_422(rng, w, h, 80)
    assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 3, 1), ref_rgb(jpeg, w, h))
    for ri in (0, 7):
        ql, qc = L.quant_table_port(50, False), L.quant_table_port(50, True)
        # large images with dense random AC take the CPU-length serial route the parallel entropy decoder declines: keep them small
        jpeg, _ = synthetic_422(rng, w, h, 30 if w * h <= 200 * 136 else 4, ql, qc, restart_interval=ri)
        assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 3, 1), ref_rgb(jpeg, w, h)), ri
        assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, 4, 1)[..., :3], ref_rgb(jpeg, w, h)), ri


def _pillow(a, **kw):
    from PIL import Image as PImage

    buf = io.BytesIO()
    PImage.fromarray(a, "RGB" if a.ndim == 3 else "L").save(buf, format="JPEG", quality=85, **kw)
    return buf.getvalue()


def test_any_runs_the_existing_entry_for_420_and_444_and_refuses_the_rest(uhdr, ref):
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    j420, j444 = pillow_420(rng, 48, 40, 85), _pillow(a, subsampling=0)
    for jpeg in (j420, j444):
        for channels, variant in ((3, 0), (4, 0), (3, 1), (4, 1)):
            assert np.array_equal(uhdr.jpeg_decode_rgb_any(jpeg, channels, variant), uhdr.jpeg_decode_rgb(jpeg, channels, variant))
    # 4:4:0 (1x2 / 1x1 / 1x1), written by the oracle's encoder, and grayscale
    grids = [(6, 6), (3, 6), (3, 6)]
    coefs = [rng.integers(-5, 6, g + (64,)).astype(np.int16) for g in grids]
    sampling = [(1, 2), (1, 1), (1, 1)]
    ql, qc = L.quant_table_port(90, False), L.quant_table_port(90, True)
    j440 = L.jpeg_assemble_port(coefs, 48, 48, sampling, 0, ql, qc, L.huffman_encode_port(coefs, 48, 48, sampling, 0))
    for jpeg in (j440, _pillow(a[..., 0])):
        with pytest.raises(A.UhdrError) as e:
            uhdr.jpeg_decode_rgb_any(jpeg, 3, 0)
        assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    j422 = pillow_422(rng, 48, 40, 85)
    for channels, variant in ((2, 0), (3, 2)):
        with pytest.raises(A.UhdrError) as e:
            uhdr.jpeg_decode_rgb_any(j422, channels, variant, out=np.empty((40, 48, channels), np.uint8))
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM
    hdr = uhdr.jpeg_parse(j422)
    buf8 = np.frombuffer(j422, dtype=np.uint8)
    out = np.empty((40, 48, 3), np.uint8)
    st = uhdr.lib.uhdr_hip_jpeg_decode_rgb_any(uhdr.ctx.handle, C.byref(hdr), C.c_void_p(buf8.ctypes.data + hdr.scan_offset),
                                               buf8.size - hdr.scan_offset, 3, 0, C.c_void_p(out.ctypes.data), 47)  # stride < width
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM
    st = uhdr.lib.uhdr_hip_jpeg_decode_rgb_any(uhdr.ctx.handle, C.byref(hdr), C.c_void_p(buf8.ctypes.data + hdr.scan_offset),
                                               buf8.size - hdr.scan_offset, 3, 0, None, 48)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM
    # the same context decodes a 4:2:2 file afterwards, and reports the call's time where the 4:2:0 entry does
    assert np.array_equal(uhdr.jpeg_decode_rgb_any(j422, 3, 1), ref_rgb(j422, 48, 40))
    st = A.Stats()
    uhdr.lib.uhdr_hip_get_stats(uhdr.ctx.handle, C.byref(st))
    assert st.last_jpeg_decode_rgb_ns > 0
