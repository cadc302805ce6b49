"""GPU: API-1 encodes with the real-time preset through the facade -- the reference's sample app on the drop-in libuhdr.so with -u 1.
With UHDR_HIP_SEAM_FUSED_REALTIME set the seam at JpegR::encodeJPEGR API-1 hands the one-pass preset at scale factor 1 to
uhdr_hip_encode_api1_scans_onepass: one device stage, the file of the per-stage seams byte for byte.  Without the variable nothing changes.
A one-channel map at scale factor 4 (the legacy JpegR() defaults) is the row of tools/api1_onepass_time.py that misses its bar, so the seam
declines it with the variable set as well -- on a shape the entry point would take (1280 x 704) and on one it would refuse (1280 x 720: a
320 x 180 map is not whole blocks) -- and the per-stage seams write the same file."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

FUSED = {"UHDR_HIP_SEAM_FUSED_REALTIME": "1"}
# scale factor 1: three channels and one channel
CASES = {"three-channel-s1": (1280, 720, ["-D", 0, "-M", 1, "-s", 1]), "one-channel-s1": (1280, 720, ["-D", 0, "-M", 0, "-s", 1])}


def _write_intents(w, h, d):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth

    hdr, sdr = synth.make_hdr_p010(w, h, ct=A.UHDR_CT_HLG), synth.make_sdr_yuv420(w, h)
    np.concatenate([hdr.valid(0).ravel(), hdr.valid(1).ravel()]).tofile(os.path.join(d, "in.p010"))
    np.concatenate([sdr.valid(c).ravel() for c in range(3)]).tofile(os.path.join(d, "in.yuv420"))


def _per_stage(trace):
    st = trace.on("device")
    return "encode_api1_fused" not in st and "generate_gainmap" in st and trace.n("jpeg_encode_scan") == 2


def _decoded_within_the_bar(d, a_jpg, b_jpg, w, h):
    """The bar of the facade's one-pass encodes (test_gpu_api0_scaled_facade.py, test_gpu_facade.py::test_api0_encode_through_the_facade) on
    decoded pixels: a +-1 map code before the JPEG DCT moves a handful of them slightly."""
    for name in (a_jpg, b_jpg):
        rc, _, err, _ = F.decode(name + ".jpg", 0, 4, name + ".raw", False, d)
        assert rc == 0, (name, err)
    a = np.fromfile(os.path.join(d, a_jpg + ".raw"), dtype=np.float16).astype(np.float32)
    b = np.fromfile(os.path.join(d, b_jpg + ".raw"), dtype=np.float16).astype(np.float32)
    assert a.size == b.size == w * h * 4
    assert (a != b).mean() < 1e-3 and np.abs(a - b).max() < 0.25, (float((a != b).mean()), float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", list(CASES))
def test_api1_realtime_encode_through_the_facade(case):
    w, h, extra = CASES[case]
    with tempfile.TemporaryDirectory() as d:
        _write_intents(w, h, d)
        # without the variable: the stage table of today -- the fused entry point declines the preset, the per-stage seams run
        rc, _, err, trace = F.encode_api1("in.p010", "in.yuv420", w, h, "plain.jpg", True, d, extra=extra)
        assert rc == 0, err
        assert _per_stage(trace), trace
        # with it: one device stage, and the same file byte for byte
        rc, _, err, trace = F.encode_api1("in.p010", "in.yuv420", w, h, "fused.jpg", True, d, extra=extra, env_extra=FUSED)
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        a, b = F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "plain.jpg"))
        assert a.size == b.size and np.array_equal(a, b), f"{a.size} / {b.size} bytes, {int((a[:min(a.size, b.size)] != b[:min(a.size, b.size)]).sum())} differ"
        # the switch that forces the per-stage seams wins over it
        rc, _, err, trace = F.encode_api1("in.p010", "in.yuv420", w, h, "staged.jpg", True, d, extra=extra,
                                          env_extra=dict(FUSED, UHDR_HIP_SEAM_NO_FUSED_ENCODE="1"))
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(a, F.read(os.path.join(d, "staged.jpg")))
        if os.path.isdir(os.path.join(F.ROOT, "oracle", "_ref")):  # the CPU reference's own file of the same command line
            rc, _, err, _ = F.encode_api1("in.p010", "in.yuv420", w, h, "cpu.jpg", False, d, extra=extra)
            assert rc == 0, err
            _decoded_within_the_bar(d, "cpu", "fused", w, h)


@pytest.mark.parametrize("w,h", [(1280, 704), (1280, 720)], ids=["whole-blocks", "ragged-map"])
def test_one_channel_at_scale_4_stays_on_the_per_stage_seams(w, h):
    """-s 4 -M 0 with the real-time preset: declined by the seam before anything goes up, variable or not, and the file is the same.
    (uhdr_hip_encode_api1_scans_onepass itself takes the 1280 x 704 pair: tests/test_gpu_api1_onepass.py covers scale factor 4 there.)"""
    extra = ["-D", 0, "-M", 0, "-s", 4]
    with tempfile.TemporaryDirectory() as d:
        _write_intents(w, h, d)
        rc, _, err, trace = F.encode_api1("in.p010", "in.yuv420", w, h, "plain.jpg", True, d, extra=extra)
        assert rc == 0, err
        assert _per_stage(trace), trace
        rc, _, err, trace = F.encode_api1("in.p010", "in.yuv420", w, h, "switch.jpg", True, d, extra=extra, env_extra=FUSED)
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "plain.jpg")), F.read(os.path.join(d, "switch.jpg")))
