"""The 4:2:2 -> RGB checkers of tests/upsample422_port.py pinned against real libjpegs: variant 0 (h2v1 fancy upsampling)
against Pillow's libjpeg-turbo, variant 1 (IJG 9's 16x8 chroma IDCT) against oracle/_ref's IJG libjpeg 9
(JpegDecoderHelper::decompressImage in DECODE_STREAM mode = DECODE_TO_RGB_CS for a YCbCr file).  Plus the ABI check for the
two entries that run this decode on the device."""
import io
import itertools
import os
import re

import numpy as np
import pytest

import upsample422_port as U
from oracle import loader as L
from test_upsample_port import coefficients, ref_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (17, 9), (37, 23), (200, 136)]
NEW_SYMBOLS = ("uhdr_hip_idct_upsample_rgb422_dev", "uhdr_hip_jpeg_decode_rgb_any")
SAMPLING = [(2, 1), (1, 1), (1, 1)]


def grids_422(w, h):
    """libjpeg's width_in_blocks grids of a 2x1 / 1x1 / 1x1 file."""
    cw = (w + 1) // 2
    return [((h + 7) // 8, (w + 7) // 8), ((h + 7) // 8, (cw + 7) // 8), ((h + 7) // 8, (cw + 7) // 8)]


def pillow_422(rng, w, h, quality):
    from PIL import Image as PImage

    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: h // 2] = (a[: h // 2].astype(np.int32) // 64 * 85).astype(np.uint8)  # flat saturated patches
    buf = io.BytesIO()
    PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=quality, subsampling=1)
    return buf.getvalue()


def synthetic_422(rng, w, h, amp, qt_luma, qt_chroma, restart_interval=0, chroma=None):
    """A 4:2:2 file with arbitrary coefficients (libjpeg's width_in_blocks grids), written by the oracle's encoder."""
    coefs = [rng.integers(-amp, amp + 1, (bh, bw, 64)).astype(np.int16) for bh, bw in grids_422(w, h)]
    if chroma is not None:
        coefs[1], coefs[2] = chroma
    for c in coefs:
        c[..., 0] = np.clip(c[..., 0], -1023 // 2, 1023 // 2)  # DC differences stay within baseline's 11 bits
    scan = L.huffman_encode_port(coefs, w, h, SAMPLING, restart_interval)
    return L.jpeg_assemble_port(coefs, w, h, SAMPLING, restart_interval, qt_luma, qt_chroma, scan), coefs


def impulse_chroma_422(w, h, amp):
    """One nonzero chroma coefficient per block, cycling through all 64 positions; Cr carries the opposite sign."""
    bh, bw = grids_422(w, h)[1]
    cb = np.zeros((bh, bw, 64), dtype=np.int16)
    for i in range(bh * bw):
        pos = i % 64
        cb.reshape(-1, 64)[i, pos] = amp if pos else amp // 2
    return cb, (-cb).astype(np.int16)


def _turbo():
    pytest.importorskip("PIL")
    from PIL import features

    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo")


def _pillow_rgb(jpeg):
    from PIL import Image as PImage

    return np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGB"))


def test_the_files_are_422(ref):
    rng = np.random.default_rng(0)
    for jpeg in (pillow_422(rng, 37, 23, 75), synthetic_422(rng, 37, 23, 5, L.quant_table_port(90, False), L.quant_table_port(90, True))[0]):
        coefs, _ = coefficients(jpeg, ref)
        assert [c.shape[:2] for c in coefs] == grids_422(37, 23)


@pytest.mark.parametrize("w,h", SIZES)
def test_variant0_port_equals_pillows_libjpeg_turbo(ref, w, h):
    _turbo()
    rng = np.random.default_rng(w * 1000 + h)
    for quality in (30, 75, 100):
        jpeg = pillow_422(rng, w, h, quality)
        coefs, qt = coefficients(jpeg, ref)
        want = _pillow_rgb(jpeg)
        got = U.decode422_rgb(coefs, qt, w, h, 0)
        assert np.array_equal(got, want), (quality, int((got != want).any(-1).sum()))
        # the triangle filter matters: plain replication is not what turbo does (beyond the tiny widths)
        if (w + 1) // 2 > 2 and h > 8:
            box = L.jpeg_ycc_to_rgb_port(np.ascontiguousarray(L.idct_dequant_port(coefs[0], qt[0])[:h, :w]),
                                         *[np.ascontiguousarray(np.repeat(L.idct_dequant_port(coefs[i], qt[i]), 2, 1)[:h, :w]) for i in (1, 2)],
                                         out_bpp=3, variant=0).reshape(h, w, 3)
            assert not np.array_equal(box, want)


def test_variant0_port_on_dense_synthetic_coefficients():
    """Every coefficient nonzero, but samples near the legal range: turbo's SIMD IDCT keeps 16-bit intermediates, so far
    out-of-range blocks compare the IDCTs, not the upsampling."""
    _turbo()
    rng = np.random.default_rng(11)
    for (w, h), (amp, quality) in itertools.product(((37, 23), (200, 136)), ((6, 95), (10, 98))):
        ql, qc = L.quant_table_port(quality, False), L.quant_table_port(quality, True)
        jpeg, coefs = synthetic_422(rng, w, h, amp, ql, qc, restart_interval=7)
        got = U.decode422_rgb(coefs, [ql, qc, qc], w, h, 0)
        assert np.array_equal(got, _pillow_rgb(jpeg))


@pytest.mark.parametrize("w,h", SIZES)
def test_variant1_port_equals_ijg9(ref, w, h):
    rng = np.random.default_rng(w * 7 + h)
    for quality in (30, 75, 100):
        jpeg = pillow_422(rng, w, h, quality)
        coefs, qt = coefficients(jpeg, ref)
        got = U.decode422_rgb(coefs, qt, w, h, 1)
        assert np.array_equal(got, ref_rgb(jpeg, w, h)), quality


@pytest.mark.parametrize("w,h", SIZES)
def test_variant1_port_on_files_from_arbitrary_coefficients(ref, w, h):
    rng = np.random.default_rng(w * 13 + h)
    ql, qc = L.quant_table_port(50, False), L.quant_table_port(50, True)
    for ri in (0, 3):
        jpeg, coefs = synthetic_422(rng, w, h, 60, ql, qc, restart_interval=ri)
        assert np.array_equal(U.decode422_rgb(coefs, [ql, qc, qc], w, h, 1), ref_rgb(jpeg, w, h)), ri


def test_larger_grids_are_accepted(ref):
    """MCU-padded arrays (what a decoder's coefficient buffers may hold) give the same pixels as the width_in_blocks grids."""
    rng = np.random.default_rng(5)
    w, h = 17, 9
    ql, qc = L.quant_table_port(50, False), L.quant_table_port(50, True)
    _, coefs = synthetic_422(rng, w, h, 60, ql, qc)
    padded = [np.pad(c, ((0, 1), (0, 2), (0, 0)), constant_values=7) for c in coefs]
    for variant in (0, 1):
        assert np.array_equal(U.decode422_rgb(padded, [ql, qc, qc], w, h, variant), U.decode422_rgb(coefs, [ql, qc, qc], w, h, variant))


@pytest.mark.parametrize("amp", [1, 1023])
def test_variant1_port_on_chroma_impulses(ref, amp):
    """All 64 chroma positions, up to baseline's extreme amplitude with the coarsest 8-bit table (the column pass beyond 2^31)."""
    rng = np.random.default_rng(amp)
    w, h = 256, 64  # 8 x 8 chroma blocks: every position once
    ql = L.quant_table_port(90, False)
    qc = np.full(64, 255 if amp > 1 else 7, dtype=np.uint16)
    jpeg, coefs = synthetic_422(rng, w, h, 3, ql, qc, chroma=impulse_chroma_422(w, h, amp))
    assert np.array_equal(U.decode422_rgb(coefs, [ql, qc, qc], w, h, 1), ref_rgb(jpeg, w, h))


def test_the_device_entries_are_in_the_header_and_the_library():
    with open(os.path.join(ROOT, "include", "uhdr_hip.h")) as f:
        header = f.read()
    from libultrahdr_amd import capi

    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
