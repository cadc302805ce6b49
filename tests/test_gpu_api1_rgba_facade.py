"""GPU: an RGBA8888 SDR intent with an RGBA1010102 (or half-float) HDR intent through the reference's sample app (ultrahdr_app -m 0,
API-1: the app's default formats) linked against the facade libuhdr.so, with the fused RGBA route of the seam switched on
(UHDR_HIP_SEAM_FUSED_RGBA_SDR): one device stage, the file the per-stage seams write, and the CPU reference's pixels within the bar of
tests/test_gpu_api0_p010_facade.py.  Without the variable, and for sizes the route declines, the per-stage seams run as before."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

FUSED = {"UHDR_HIP_SEAM_FUSED_RGBA_SDR": "1"}


def _write_intents(d, w, h, half=False):
    """-> the command line: BT.2100 PQ RGBA1010102 (or linear half float) + BT.709 RGBA8888, best-quality preset and gamma 1 spelled out."""
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth

    synth.make_sdr_rgba8888(w, h, align=1).valid(0).tofile(os.path.join(d, "in.rgba8888"))
    if half:
        synth.make_hdr_rgba_f16(w, h, specials=False, align=1).valid(0).tofile(os.path.join(d, "in.f16"))
        hdr = ["-p", "in.f16", "-a", 4, "-t", 0]
    else:
        synth.make_hdr_rgba1010102(w, h, ct=A.UHDR_CT_PQ, align=1).valid(0).tofile(os.path.join(d, "in.rgba1010102"))
        hdr = ["-p", "in.rgba1010102", "-a", 5, "-t", 2]
    return ["-m", 0] + hdr + ["-y", "in.rgba8888", "-b", 3, "-w", w, "-h", h, "-C", 2, "-c", 0, "-R", 1, "-D", 1, "-G", 1.0]


def _decoded(d, name):
    rc, _, err, _ = F.decode(name + ".jpg", 0, 4, name + ".raw", False, d)
    assert rc == 0, (name, err)
    return np.fromfile(os.path.join(d, name + ".raw"), dtype=np.float16).astype(np.float32)


def _assert_pixels_close(a, b, n, what):
    assert a.size == b.size == n
    # a +-1 8-bit sample before the JPEG DCT moves a handful of decoded pixels slightly
    assert (a != b).mean() < 1e-3 and np.abs(a - b).max() < 0.25, (what, float((a != b).mean()), float(np.abs(a - b).max()))


def _is_per_stage(trace):
    st = trace.on("device")
    return "encode_api1_fused" not in st and "generate_gainmap" in st and trace.n("jpeg_encode_scan") == 2


def test_rgba_api1_encode_takes_the_fused_route_when_asked_to():
    w, h = 640, 368
    with tempfile.TemporaryDirectory() as d:
        args = _write_intents(d, w, h)
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        rc, _, err, trace = F.run_app(args + ["-z", "fused.jpg"], True, d, env_extra=FUSED)
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        # the file the per-stage seams write, byte for byte
        rc, _, err, trace = F.run_app(args + ["-z", "stages.jpg"], True, d, env_extra={"UHDR_HIP_SEAM_NO_FUSED_ENCODE": "1"})
        assert rc == 0, err
        assert _is_per_stage(trace), trace
        a, b = F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "stages.jpg"))
        assert a.size == b.size and np.array_equal(a, b), (a.size, b.size)
        _assert_pixels_close(_decoded(d, "cpu"), _decoded(d, "fused"), w * h * 4, "fused")
        # without the variable nothing changes: the per-stage seams, the same file
        rc, _, err, trace = F.run_app(args + ["-z", "default.jpg"], True, d)
        assert rc == 0, err
        assert _is_per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "default.jpg")), b)


def test_rgba_api1_encode_of_a_size_the_fused_route_declines():
    """644 x 368: 644 is not a multiple of 8, so the seam leaves the intent to the per-stage seams even with the variable set."""
    w, h = 644, 368
    with tempfile.TemporaryDirectory() as d:
        args = _write_intents(d, w, h)
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        rc, _, err, trace = F.run_app(args + ["-z", "gpu.jpg"], True, d, env_extra=FUSED)
        assert rc == 0, err
        assert _is_per_stage(trace), trace
        _assert_pixels_close(_decoded(d, "cpu"), _decoded(d, "gpu"), w * h * 4, "per-stage seams")


def test_rgba_api1_encode_with_a_half_float_hdr_intent_takes_the_fused_route():
    w, h = 640, 368
    with tempfile.TemporaryDirectory() as d:
        args = _write_intents(d, w, h, half=True)
        rc, _, err, trace = F.run_app(args + ["-z", "fused.jpg"], True, d, env_extra=FUSED)
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        rc, _, err, trace = F.run_app(args + ["-z", "stages.jpg"], True, d, env_extra={"UHDR_HIP_SEAM_NO_FUSED_ENCODE": "1"})
        assert rc == 0, err
        assert _is_per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "stages.jpg")))
