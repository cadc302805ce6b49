"""GPU: 4:2:0 JPEG -> RGB888 / RGBA8888 on the device, libjpeg-exact (uhdr_hip_idct_upsample_rgb_dev and the whole-file
uhdr_hip_jpeg_decode_rgb).  Checked bit for bit against the numpy restatements of tests/upsample_port.py, against Pillow's
libjpeg-turbo (variant 0) and against oracle/_ref's IJG libjpeg 9 (variant 1)."""
import io

import numpy as np
import pytest

import upsample_port as U
from libultrahdr_amd import capi as A
from oracle import loader as L
from test_upsample_port import coefficients, impulse_chroma, pillow_420, ref_rgb, synthetic_420

pytestmark = pytest.mark.gpu

FMT = {3: A.UHDR_IMG_FMT_24bppRGB888, 4: A.UHDR_IMG_FMT_32bppRGBA8888}
DEV_SIZES = [(1, 1), (2, 2), (4, 4), (5, 3), (17, 9), (37, 23), (100, 60), (333, 211), (1283, 721), (3840, 2160), (7680, 4320)]


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def _grids(w, h):
    return [((h + 7) // 8, (w + 7) // 8), ((h + 15) // 16, (w + 15) // 16), ((h + 15) // 16, (w + 15) // 16)]


def _pixels(img, w, h, ch):
    return np.ascontiguousarray(img.to_host().valid(0)).view(np.uint8).reshape(h, w, ch)


def _dense_coefs(rng, w, h):
    """Smooth-ish content: a DC field plus small random AC, so the samples sit around the legal range and clamp now and then."""
    out = []
    for bh, bw in _grids(w, h):
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
    want = {ch: U.decode420_rgb(coefs, qts, w, h, variant, ch) for ch in (3, 4)}
    dev = [torch.from_numpy(c).to("cuda:0") for c in coefs]
    for ch in (3, 4):
        img = uhdr.idct_upsample_rgb(dev, qts, w, h, FMT[ch], variant)
        uhdr.ctx.synchronize()
        got = _pixels(img, w, h, ch)
        assert np.array_equal(got, want[ch]), (ch, int((got != want[ch]).any(-1).sum()))


def test_dev_entry_on_chroma_impulses(uhdr):
    """Variant 1 at baseline's extreme amplitude: the 16-point column pass needs more than 32 bits there."""
    import torch

    w, h = 128, 128
    rng = np.random.default_rng(3)
    for amp, q in ((1, 7), (1023, 255)):
        cb, cr = impulse_chroma(w, h, amp)
        coefs = [rng.integers(-3, 4, _grids(w, h)[0] + (64,)).astype(np.int16), cb, cr]
        qts = [L.quant_table_port(90, False), np.full(64, q, np.uint16), np.full(64, q, np.uint16)]
        for variant in (0, 1):
            img = uhdr.idct_upsample_rgb([torch.from_numpy(c).to("cuda:0") for c in coefs], qts, w, h, FMT[4], variant)
            uhdr.ctx.synchronize()
            assert np.array_equal(_pixels(img, w, h, 4), U.decode420_rgb(coefs, qts, w, h, variant, 4)), (amp, variant)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (37, 23), (200, 136), (1283, 721)])
def test_whole_file_equals_pillows_libjpeg_turbo(uhdr, ref, w, h):
    from PIL import Image as PImage, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(w + 7 * h)
    for quality in (30, 90):
        jpeg = pillow_420(rng, w, h, quality)
        want = np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 3, 0), want)
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 4, 0)[..., :3], want)
    for ri in (0, 7):  # restart markers take the interval decoder
        ql, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
        jpeg, _ = synthetic_420(rng, w, h, 6, ql, qc, restart_interval=ri)
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 3, 0), np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))), ri


@pytest.mark.parametrize("w,h", [(2, 2), (17, 9), (200, 136), (1283, 721)])
def test_whole_file_equals_ijg9(uhdr, ref, w, h):
    rng = np.random.default_rng(w + 5 * h)
    jpeg = pillow_420(rng, w, h, 80)
    assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 3, 1), ref_rgb(jpeg, w, h))
    for ri in (0, 7):
        ql, qc = L.quant_table_port(50, False), L.quant_table_port(50, True)
        # large images with dense random AC take the CPU-length serial route the parallel entropy decoder declines: keep them small
        jpeg, _ = synthetic_420(rng, w, h, 30 if w * h <= 200 * 136 else 4, ql, qc, restart_interval=ri)
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 3, 1), ref_rgb(jpeg, w, h)), ri
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 4, 1)[..., :3], ref_rgb(jpeg, w, h)), ri


def test_whole_file_444_takes_the_fused_path(uhdr, ref):
    from PIL import Image as PImage

    rng = np.random.default_rng(44)
    a = rng.integers(0, 256, (96, 130, 3), dtype=np.uint8)
    buf = io.BytesIO()
    PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=85, subsampling=0)
    jpeg = buf.getvalue()
    coefs, qt = coefficients(jpeg, ref)
    planes = [np.ascontiguousarray(L.idct_dequant_port(coefs[c], qt[c])[:96, :130]) for c in range(3)]
    for variant in (0, 1):
        want = L.jpeg_ycc_to_rgb_port(*planes, out_bpp=4, variant=variant).reshape(96, 130, 4)
        assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 4, variant), want)


def test_other_samplings_and_bad_arguments_are_refused_and_the_context_stays_usable(uhdr, ref):
    from PIL import Image as PImage

    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    for sub in (1,):  # 4:2:2
        buf = io.BytesIO()
        PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=85, subsampling=sub)
        with pytest.raises(A.UhdrError) as e:
            uhdr.jpeg_decode_rgb(buf.getvalue(), 3, 0)
        assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    buf = io.BytesIO()
    PImage.fromarray(a[..., 0], "L").save(buf, format="JPEG", quality=85)
    with pytest.raises(A.UhdrError) as e:
        uhdr.jpeg_decode_rgb(buf.getvalue(), 3, 0)
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    jpeg = pillow_420(rng, 48, 40, 85)
    for channels, variant in ((2, 0), (3, 2)):
        with pytest.raises(A.UhdrError) as e:
            uhdr.jpeg_decode_rgb(jpeg, channels, variant, out=np.empty((40, 48, channels), np.uint8))
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM
    import ctypes as C

    hdr = uhdr.jpeg_parse(jpeg)
    buf8 = np.frombuffer(jpeg, dtype=np.uint8)
    out = np.empty((40, 48, 3), np.uint8)
    st = uhdr.lib.uhdr_hip_jpeg_decode_rgb(uhdr.ctx.handle, C.byref(hdr), C.c_void_p(buf8.ctypes.data + hdr.scan_offset),
                                           buf8.size - hdr.scan_offset, 3, 0, C.c_void_p(out.ctypes.data), 47)  # stride < width
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM
    st = uhdr.lib.uhdr_hip_jpeg_decode_rgb(uhdr.ctx.handle, C.byref(hdr), C.c_void_p(buf8.ctypes.data + hdr.scan_offset),
                                           buf8.size - hdr.scan_offset, 3, 0, None, 48)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM
    # the same context decodes afterwards, and the planar entry's refusal of RGB from a subsampled file is unchanged
    assert np.array_equal(uhdr.jpeg_decode_rgb(jpeg, 3, 1), ref_rgb(jpeg, 48, 40))
    with pytest.raises(A.UhdrError) as e:
        uhdr.jpeg_decode(jpeg, 3)
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
