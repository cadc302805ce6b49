"""The 4:2:0 -> RGB checkers of tests/upsample_port.py pinned against real libjpegs: variant 0 (h2v2 fancy upsampling)
against Pillow's libjpeg-turbo, variant 1 (IJG 9's 16x16 chroma IDCT) against oracle/_ref's IJG libjpeg 9
(JpegDecoderHelper::decompressImage in DECODE_STREAM mode = DECODE_TO_RGB_CS for a YCbCr file).  Plus the ABI check
for the two entries that run this decode on the device."""
import ctypes as C
import io
import itertools
import os
import re

import numpy as np
import pytest

import upsample_port as U
from oracle import loader as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (17, 9), (37, 23), (200, 136), (1283, 721)]
NEW_SYMBOLS = ("uhdr_hip_idct_upsample_rgb_dev", "uhdr_hip_jpeg_decode_rgb")


def coefficients(jpeg: bytes, ref):
    data = np.frombuffer(jpeg, dtype=np.uint8)
    qt = np.zeros((3, 64), dtype=np.uint16)
    bw, bh, nc = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    null = (C.c_void_p * 3)(None, None, None)
    assert ref.ref_jpeg_read_coefficients(data.ctypes.data, data.size, null, qt.ctypes.data, bw, bh, C.byref(nc)) == 0
    coefs = [np.zeros((bh[c], bw[c], 64), dtype=np.int16) for c in range(3)]
    ptrs = (C.c_void_p * 3)(*[c.ctypes.data for c in coefs])
    assert ref.ref_jpeg_read_coefficients(data.ctypes.data, data.size, ptrs, qt.ctypes.data, bw, bh, C.byref(nc)) == 0
    return coefs, qt


def pillow_420(rng, w, h, quality):
    from PIL import Image as PImage

    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: h // 2] = (a[: h // 2].astype(np.int32) // 64 * 85).astype(np.uint8)  # flat saturated patches
    buf = io.BytesIO()
    PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def synthetic_420(rng, w, h, amp, qt_luma, qt_chroma, restart_interval=0, chroma=None):
    """A 4:2:0 file with arbitrary coefficients (libjpeg's width_in_blocks grids), written by the oracle's encoder."""
    grids = [((h + 7) // 8, (w + 7) // 8), ((h + 15) // 16, (w + 15) // 16), ((h + 15) // 16, (w + 15) // 16)]
    coefs = [rng.integers(-amp, amp + 1, (bh, bw, 64)).astype(np.int16) for bh, bw in grids]
    if chroma is not None:
        coefs[1], coefs[2] = chroma
    for c in coefs:
        c[..., 0] = np.clip(c[..., 0], -1023 // 2, 1023 // 2)  # DC differences stay within baseline's 11 bits
    sampling = [(2, 2), (1, 1), (1, 1)]
    scan = L.huffman_encode_port(coefs, w, h, sampling, restart_interval)
    return L.jpeg_assemble_port(coefs, w, h, sampling, restart_interval, qt_luma, qt_chroma, scan), coefs


def impulse_chroma(w, h, amp):
    """One nonzero chroma coefficient per block, cycling through all 64 positions; Cr carries the opposite sign."""
    bh, bw = (h + 15) // 16, (w + 15) // 16
    cb = np.zeros((bh, bw, 64), dtype=np.int16)
    for i in range(bh * bw):
        pos = i % 64
        cb.reshape(-1, 64)[i, pos] = amp if pos else amp // 2
    return cb, (-cb).astype(np.int16)


def ref_rgb(jpeg, w, h):
    desc, buf = L.ref_jpeg_decompress(jpeg, 1)
    assert desc.fmt == 11 and desc.w == w and desc.h == h  # UHDR_IMG_FMT_24bppRGB888
    return buf[: desc.stride[0] * h * 3].reshape(h, desc.stride[0], 3)[:, :w]


@pytest.mark.parametrize("w,h", SIZES)
def test_variant0_port_equals_pillows_libjpeg_turbo(ref, w, h):
    PIL = pytest.importorskip("PIL")  # noqa: F841
    from PIL import Image as PImage, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(w * 1000 + h)
    for quality in (30, 75, 100):
        jpeg = pillow_420(rng, w, h, quality)
        coefs, qt = coefficients(jpeg, ref)
        want = np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))
        got = U.decode420_rgb(coefs, qt, w, h, 0)
        assert np.array_equal(got, want), (quality, int((got != want).any(-1).sum()))
        # the triangle filter matters: plain 2x2 replication is not what turbo does (beyond the tiny widths)
        if (w + 1) // 2 > 2 and h > 8:
            box = L.jpeg_ycc_to_rgb_port(np.ascontiguousarray(L.idct_dequant_port(coefs[0], qt[0])[:h, :w]),
                                         *[np.ascontiguousarray(np.repeat(np.repeat(L.idct_dequant_port(coefs[i], qt[i]), 2, 0), 2, 1)[:h, :w])
                                           for i in (1, 2)], out_bpp=3, variant=0).reshape(h, w, 3)
            assert not np.array_equal(box, want)


def test_variant0_port_on_dense_synthetic_coefficients():
    """Every coefficient nonzero, but samples near the legal range: turbo's SIMD IDCT keeps 16-bit intermediates, so far
    out-of-range blocks compare the IDCTs, not the upsampling."""
    PIL = pytest.importorskip("PIL")  # noqa: F841
    from PIL import Image as PImage, features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    rng = np.random.default_rng(11)
    for (w, h), (amp, quality) in itertools.product(((37, 23), (200, 136)), ((6, 95), (10, 98))):
        ql, qc = L.quant_table_port(quality, False), L.quant_table_port(quality, True)
        jpeg, coefs = synthetic_420(rng, w, h, amp, ql, qc, restart_interval=7)
        want = np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))
        got = U.decode420_rgb(coefs, [ql, qc, qc], w, h, 0)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("w,h", SIZES)
def test_variant1_port_equals_ijg9(ref, w, h):
    rng = np.random.default_rng(w * 7 + h)
    for quality in (30, 75, 100):
        jpeg = pillow_420(rng, w, h, quality)
        coefs, qt = coefficients(jpeg, ref)
        got = U.decode420_rgb(coefs, qt, w, h, 1)
        assert np.array_equal(got, ref_rgb(jpeg, w, h)), quality


def test_variant1_port_on_dense_synthetic_coefficients(ref):
    rng = np.random.default_rng(12)
    for (w, h) in ((37, 23), (200, 136), (64, 48)):
        ql, qc = L.quant_table_port(50, False), L.quant_table_port(50, True)
        jpeg, coefs = synthetic_420(rng, w, h, 60, ql, qc)
        assert np.array_equal(U.decode420_rgb(coefs, [ql, qc, qc], w, h, 1), ref_rgb(jpeg, w, h))


@pytest.mark.parametrize("amp", [1, 37, 1023])
def test_variant1_port_on_chroma_impulses(ref, amp):
    """All 64 chroma positions, up to baseline's extreme amplitude with the coarsest 8-bit table (pass 1 beyond 2^31)."""
    rng = np.random.default_rng(amp)
    w, h = 128, 128
    ql = L.quant_table_port(90, False)
    qc = np.full(64, 255 if amp > 1 else 7, dtype=np.uint16)
    jpeg, coefs = synthetic_420(rng, w, h, 3, ql, qc, chroma=impulse_chroma(w, h, amp))
    assert np.array_equal(U.decode420_rgb(coefs, [ql, qc, qc], w, h, 1), ref_rgb(jpeg, w, h))


def test_the_device_entries_are_in_the_header_and_the_library():
    with open(os.path.join(ROOT, "include", "uhdr_hip.h")) as f:
        header = f.read()
    from libultrahdr_amd import capi

    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
