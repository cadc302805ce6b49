"""GPU: uhdr_decode of a JpegR whose gain map has gamma 1.571 at scale 4, behind the drop-in libuhdr.so.  With
UHDR_HIP_SEAM_GAMMA_TABLE set the facade's apply_gainmap seam hands the stage to uhdr_hip_apply_gainmap_ex with
UHDR_HIP_APPLY_GAMMA_TABLE -- the GainLUT index (gainmapmath.h:483-489) from host-built thresholds -- and the decode equals the CPU
decode byte for byte; without it the stage runs on the device through the pow per sample, as before, within the allowance that route
has always had (one output code on at most 0.1 % of the samples)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from tests import facade_util as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

W, H, MW, MH = 256, 144, 64, 36
GAMMA = 1.571


def _jpeg(a, **kw):
    from PIL import Image as PImage

    buf = io.BytesIO()
    PImage.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def build_jpegr():
    """API-4 through the drop-in's own C API, GPU acceleration off: a compressed 256x144 4:2:0 base image, a compressed 64x36 Y400
    gain map and metadata with gamma 1.571."""
    from libultrahdr_amd import facade as FA

    lib = FA.load()
    lib.uhdr_enc_set_compressed_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_compressed_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.c_int]
    lib.uhdr_enc_set_gainmap_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_gainmap_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.POINTER(A.GainmapMetadata)]
    rng = np.random.default_rng(47)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([96 + xx * 150 // W, 96 + yy * 150 // H, 96 + (xx + yy) * 61 % 150], -1)
    base = _jpeg(np.clip(base + rng.integers(-8, 9, base.shape), 0, 255).astype(np.uint8), quality=92, subsampling=2)
    yy, xx = np.mgrid[0:MH, 0:MW]
    gm = _jpeg(np.clip((xx * 4 + yy * 5) % 256 + rng.integers(-6, 7, (MH, MW)), 0, 255).astype(np.uint8), quality=95)
    md = synth.default_metadata(use_base_cg=1, gamma=GAMMA)
    keep = []

    def ci(data):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        keep.append(buf)
        return FA.CompressedImage(C.cast(buf, C.c_void_p), len(data), len(data), A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE)

    b, g = ci(base), ci(gm)
    h = lib.uhdr_create_encoder()
    try:
        FA._chk(lib.uhdr_enc_set_compressed_image(h, C.byref(b), FA.UHDR_BASE_IMG))
        FA._chk(lib.uhdr_enc_set_gainmap_image(h, C.byref(g), C.byref(md)))
        FA._chk(lib.uhdr_encode(h))
        o = lib.uhdr_get_encoded_stream(h).contents
        return C.string_at(o.data, o.data_sz)
    finally:
        lib.uhdr_release_encoder(h)


@pytest.fixture(scope="module")
def jpegr():
    return build_jpegr()


def _decode(jpegr, ct, fmt, gpu, switch):
    """-> (pixels, how often apply_gainmap ran on the device, ... was left to the reference)"""
    from libultrahdr_amd import facade as FA

    old = os.environ.pop("UHDR_HIP_SEAM_GAMMA_TABLE", None)
    if switch:
        os.environ["UHDR_HIP_SEAM_GAMMA_TABLE"] = "1"
    try:
        A.seam_stats(reset=True)
        px = FA.decode(jpegr, ct, fmt, gpu=gpu)
        st = A.seam_stats(reset=True)
    finally:
        os.environ.pop("UHDR_HIP_SEAM_GAMMA_TABLE", None)
        if old is not None:
            os.environ["UHDR_HIP_SEAM_GAMMA_TABLE"] = old
    row = st.get("apply_gainmap", {})
    return px, row.get("device", 0), row.get("reference", 0)


def _codes(px, ct):
    """Per-channel output codes: half-float bit patterns (linear) or the 10-bit fields (PQ)."""
    if ct == A.UHDR_CT_LINEAR:
        return np.ascontiguousarray(px).view(np.uint16).astype(np.int64)
    v = np.ascontiguousarray(px).view(np.uint32).astype(np.int64)
    return np.stack([(v >> s) & 0x3FF for s in (0, 10, 20)], -1)


@pytest.mark.parametrize("ct,fmt", [(A.UHDR_CT_LINEAR, A.UHDR_IMG_FMT_64bppRGBAHalfFloat), (A.UHDR_CT_PQ, A.UHDR_IMG_FMT_32bppRGBA1010102)],
                         ids=["linear", "pq"])
def test_with_the_switch_the_device_decode_is_the_cpu_decode(jpegr, ct, fmt):
    cpu, dev0, _ = _decode(jpegr, ct, fmt, gpu=False, switch=False)
    assert cpu.shape[:2] == (H, W) and dev0 == 0
    tab, dev1, ref1 = _decode(jpegr, ct, fmt, gpu=True, switch=True)
    assert dev1 == 1 and ref1 == 0, "the stage table shows apply_gainmap on the device"
    assert np.array_equal(tab, cpu), int((tab != cpu).sum())
    # without the switch: on the device as before, through the pow per sample, within that route's allowance
    pw, dev2, ref2 = _decode(jpegr, ct, fmt, gpu=True, switch=False)
    assert dev2 == 1 and ref2 == 0
    d = np.abs(_codes(pw, ct) - _codes(cpu, ct))
    print(f"without the switch: max code diff {d.max()}, {(d != 0).mean():.4%} of samples differ")
    assert d.max() <= 1 and (d != 0).mean() <= 0.001
