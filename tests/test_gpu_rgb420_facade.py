"""GPU: uhdr_decode to UHDR_CT_SRGB / RGBA8888 -- the call the reference answers with the base JPEG alone, decoded by libjpeg
with DECODE_TO_RGB_CS (jpegr.cpp:1479-1525, jpegdecoderhelper.cpp:349-375) -- on the device behind the drop-in libuhdr.so:
the 4:2:0 base image goes to uhdr_hip_jpeg_decode_rgb.  The facade links IJG libjpeg 9, so the device rebuilds the chroma with
IJG 9's 16x16 IDCT (variant 1).  Checked byte for byte against the facade's own CPU route and the real reference's uhdr_decode;
the library's stage table (uhdr_hip_seam_stats) shows which route ran, and UHDR_HIP_SEAM_CPU_UPSAMPLE=1 keeps libjpeg."""
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


@pytest.fixture(scope="module")
def jpegr(ref):
    """The 720p fixture's JpegR (API-1, the C API's defaults), written by the real reference on the host."""
    sdr, hdr = fixture720.inputs()
    return L.ref_uhdr_encode(hdr, sdr)


@pytest.fixture(scope="module")
def ref_srgb(jpegr):
    dest = np.zeros(W * H * 4, np.uint8)
    assert L.ref_uhdr_decode(jpegr, A.UHDR_CT_SRGB, A.UHDR_IMG_FMT_32bppRGBA8888, dest) == (W, H)
    return dest.reshape(H, W, 4)


def test_base_image_of_a_jpegr_equals_the_references_srgb_decode(hip_ctx, jpegr, ref_srgb):
    from libultrahdr_amd.ultrahdr import UltraHdr

    u = UltraHdr(ctx=hip_ctx)
    assert (ref_srgb[..., 3] == 255).all()
    # the whole JpegR goes in: the decoder stops at the base image's EOI as libjpeg does
    assert np.array_equal(u.jpeg_decode_rgb(jpegr, 3, 1), ref_srgb[..., :3])
    rgba = u.jpeg_decode_rgb(jpegr, 4, 1)
    assert np.array_equal(rgba, ref_srgb)


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


def test_app_routes_in_fresh_processes(jpegr):
    """The reference's own app with -u 1, one process per route: the device route by default, libjpeg's with
    UHDR_HIP_SEAM_CPU_UPSAMPLE=1 -- the same bytes either way."""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in.jpg"), "wb") as f:
            f.write(jpegr)
        rc, _, err, _ = F.decode("in.jpg", 3, 3, "cpu.raw", False, d)
        assert rc == 0, err
        rc, _, err, trace = F.decode("in.jpg", 3, 3, "gpu.raw", True, d)
        assert rc == 0, err
        assert trace.n("jpeg_decode_rgb") == 1 and trace.n("jpeg_decode_rgb", "reference") == 0, trace
        rc, _, err, trace = F.decode("in.jpg", 3, 3, "cpu_upsample.raw", True, d, env_extra={"UHDR_HIP_SEAM_CPU_UPSAMPLE": "1"})
        assert rc == 0, err
        assert trace.n("jpeg_decode_rgb") == 0 and trace.n("jpeg_decode_rgb", "reference") == 1, trace
        a = F.read(os.path.join(d, "cpu.raw"))
        assert a.size == W * H * 4
        assert np.array_equal(a, F.read(os.path.join(d, "gpu.raw")))
        assert np.array_equal(a, F.read(os.path.join(d, "cpu_upsample.raw")))
