"""GPU: uhdr_decode to UHDR_CT_SRGB / RGBA8888 of a JpegR whose base image is a 4:2:2 camera JPEG (the compressed SDR intent of
API-2/3/4, jpegr.cpp:538, 1587) on the device behind the drop-in libuhdr.so: the base image goes to
uhdr_hip_jpeg_decode_rgb_any.  The facade links IJG libjpeg 9, so the device rebuilds the chroma with IJG 9's 16x8 IDCT
(variant 1).  Checked byte for byte against the facade's own CPU route and the real reference's uhdr_decode; the library's stage
table (uhdr_hip_seam_stats) shows which route ran, and UHDR_HIP_SEAM_CPU_UPSAMPLE=1 keeps libjpeg."""
import ctypes as C
import io
import os
import tempfile

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from oracle import loader as L
from tests import facade_util as F
from tests import fixture720

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

W, H = 1280, 720


def _camera_jpeg():
    """A Pillow-written 1280x720 4:2:2 JPEG: a smooth scene with some noise."""
    from PIL import Image as PImage

    rng = np.random.default_rng(422)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([xx * 255 // W, yy * 255 // H, (xx + yy) * 97 % 256], -1)
    a = np.clip(a + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=90, subsampling=1)
    return buf.getvalue()


def build_jpegr():
    """API-3 through the drop-in's own C API, GPU acceleration off: the 720p fixture's HDR intent + the 4:2:2 JPEG as the
    compressed SDR intent."""
    from libultrahdr_amd import facade as FA

    lib = FA.load()
    lib.uhdr_enc_set_compressed_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_compressed_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.c_int]
    _, hdr = fixture720.inputs()
    sdr = _camera_jpeg()
    buf = (C.c_uint8 * len(sdr)).from_buffer_copy(sdr)
    ci = FA.CompressedImage(C.cast(buf, C.c_void_p), len(sdr), len(sdr), A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE)
    h = lib.uhdr_create_encoder()
    try:
        FA._chk(lib.uhdr_enc_set_raw_image(h, C.byref(hdr.raw), FA.UHDR_HDR_IMG))
        FA._chk(lib.uhdr_enc_set_compressed_image(h, C.byref(ci), FA.UHDR_SDR_IMG))
        FA._chk(lib.uhdr_encode(h))
        o = lib.uhdr_get_encoded_stream(h).contents
        out = C.string_at(o.data, o.data_sz)
    finally:
        lib.uhdr_release_encoder(h)
    # the base image really is 2x1 / 1x1 / 1x1
    hd = A.JpegHeader()
    b = np.frombuffer(out, dtype=np.uint8)
    assert A.load().uhdr_hip_jpeg_parse(C.c_void_p(b.ctypes.data), b.size, C.byref(hd)) == 0
    sc = hd.scan
    assert (sc.w, sc.h, sc.num_components) == (W, H, 3)
    assert [(sc.h_samp[c], sc.v_samp[c]) for c in range(3)] == [(2, 1), (1, 1), (1, 1)]
    return out


@pytest.fixture(scope="module")
def jpegr():
    return build_jpegr()


@pytest.fixture(scope="module")
def ref_srgb(jpegr, ref):
    dest = np.zeros(W * H * 4, np.uint8)
    assert L.ref_uhdr_decode(jpegr, A.UHDR_CT_SRGB, A.UHDR_IMG_FMT_32bppRGBA8888, dest) == (W, H)
    return dest.reshape(H, W, 4)


def test_base_image_of_the_jpegr_equals_the_references_srgb_decode(hip_ctx, jpegr, ref_srgb):
    from libultrahdr_amd.ultrahdr import UltraHdr

    u = UltraHdr(ctx=hip_ctx)
    assert (ref_srgb[..., 3] == 255).all()
    # the whole JpegR goes in: the decoder stops at the base image's EOI as libjpeg does
    assert np.array_equal(u.jpeg_decode_rgb_any(jpegr, 3, 1), ref_srgb[..., :3])
    assert np.array_equal(u.jpeg_decode_rgb_any(jpegr, 4, 1), ref_srgb)


def test_facade_srgb_decode_runs_on_the_device_and_equals_the_cpu_route(jpegr, ref_srgb):
    from libultrahdr_amd import facade as FA

    cpu = FA.decode(jpegr, A.UHDR_CT_SRGB, A.UHDR_IMG_FMT_32bppRGBA8888, gpu=False)
    A.seam_stats(reset=True)
    gpu = FA.decode(jpegr, A.UHDR_CT_SRGB, A.UHDR_IMG_FMT_32bppRGBA8888, gpu=True)
    st = A.seam_stats(reset=True)
    assert st.get("jpeg_decode_rgb", {}).get("device", 0) == 1, st
    assert st["jpeg_decode_rgb"]["reference"] == 0, st
    assert np.array_equal(gpu, cpu), int((gpu != cpu).any(-1).sum())
    assert np.array_equal(gpu, ref_srgb)


def test_cpu_upsample_switch_keeps_libjpeg_in_a_fresh_process(jpegr, ref_srgb):
    """The reference's own app with -u 1 and UHDR_HIP_SEAM_CPU_UPSAMPLE=1: the decode is declined to libjpeg, tallied as the
    reference route, and gives the same bytes."""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in.jpg"), "wb") as f:
            f.write(jpegr)
        rc, _, err, trace = F.decode("in.jpg", 3, 3, "cpu_upsample.raw", True, d, env_extra={"UHDR_HIP_SEAM_CPU_UPSAMPLE": "1"})
        assert rc == 0, err
        assert trace.n("jpeg_decode_rgb") == 0 and trace.n("jpeg_decode_rgb", "reference") == 1, trace
        assert np.array_equal(F.read(os.path.join(d, "cpu_upsample.raw")), ref_srgb.reshape(-1))
