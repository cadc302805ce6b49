"""GPU: API-0 encodes with a sub-sampled gain map through the facade -- the reference's sample app on the drop-in libuhdr.so with -u 1.
With UHDR_HIP_SEAM_FUSED_SCALED_MAP set (and UHDR_HIP_SEAM_FUSED_P010 for a P010 intent) the seam at JpegR::encodeJPEGR API-0 hands scale
factors 2 and 4 to uhdr_hip_encode_api0_scans_scaled: one device stage, the file of the five per-stage seams byte for byte.  Without the
variable nothing changes, and a shape the entry point would decline (a map that is not whole blocks) stays on the per-stage seams."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

W, H = 640, 384  # 160 x 96 and 320 x 192 maps: whole blocks at both scale factors
SCALED = {"UHDR_HIP_SEAM_FUSED_SCALED_MAP": "1"}
# (intent, sample-app arguments of the intent, environment that selects the fused route)
INTENTS = {"rgba1010102": (["-a", 5, "-C", 2, "-t", 2, "-R", 1], SCALED),
           "p010": (["-a", 0, "-C", 2, "-t", 1, "-R", 0], dict(SCALED, UHDR_HIP_SEAM_FUSED_P010="1"))}
MAPS = {"android": ["-s", 4, "-M", 0], "s2-three-channel": ["-s", 2, "-M", 1]}


def _write_intent(intent, w, h, d):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth

    path = os.path.join(d, "in.raw")
    if intent == "p010":
        hp = synth.make_hdr_p010(w, h, ct=A.UHDR_CT_HLG)
        np.concatenate([hp.valid(0).ravel(), hp.valid(1).ravel()]).tofile(path)
    else:
        synth.make_hdr_rgba1010102(w, h, ct=A.UHDR_CT_PQ).valid(0).tofile(path)


def _per_stage(trace):
    st = trace.on("device")
    return "encode_api0_fused" not in st and "tone_map" in st and "generate_gainmap" in st and trace.n("jpeg_encode_scan") == 2


def _decoded_within_the_bar(d, a_jpg, b_jpg, w, h):
    """test_api0_encode_through_the_facade's bar on decoded pixels: a +-1 8-bit sample before the JPEG DCT moves a handful of them slightly."""
    for name in (a_jpg, b_jpg):
        rc, _, err, _ = F.decode(name + ".jpg", 0, 4, name + ".raw", False, d)
        assert rc == 0, (name, err)
    a = np.fromfile(os.path.join(d, a_jpg + ".raw"), dtype=np.float16).astype(np.float32)
    b = np.fromfile(os.path.join(d, b_jpg + ".raw"), dtype=np.float16).astype(np.float32)
    assert a.size == b.size == w * h * 4
    assert (a != b).mean() < 1e-3 and np.abs(a - b).max() < 0.25, (float((a != b).mean()), float(np.abs(a - b).max()))


@pytest.mark.parametrize("map_kind", list(MAPS))
@pytest.mark.parametrize("intent", list(INTENTS))
def test_api0_encode_with_a_scaled_map_through_the_facade(intent, map_kind):
    fmt_args, fused_env = INTENTS[intent]
    with tempfile.TemporaryDirectory() as d:
        _write_intent(intent, W, H, d)
        args = ["-m", 0, "-p", "in.raw", "-w", W, "-h", H] + fmt_args + MAPS[map_kind]
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        # with the variable(s): one device stage ...
        rc, _, err, trace = F.run_app(args + ["-z", "fused.jpg"], True, d, env_extra=fused_env)
        assert rc == 0, err
        assert trace.on("device") == ["encode_api0_fused"], trace
        # ... and the file of the per-stage seams, byte for byte
        rc, _, err, trace = F.run_app(args + ["-z", "staged.jpg"], True, d, env_extra={"UHDR_HIP_SEAM_NO_FUSED_ENCODE": "1"})
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "staged.jpg")))
        # without the variable: the per-stage seams and the same file
        rc, _, err, trace = F.run_app(args + ["-z", "plain.jpg"], True, d)
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "plain.jpg")), F.read(os.path.join(d, "staged.jpg")))
        _decoded_within_the_bar(d, "cpu", "fused", W, H)


@pytest.mark.parametrize("intent", list(INTENTS))
def test_a_map_that_is_not_whole_blocks_stays_on_the_per_stage_seams(intent):
    """640 x 360 at -s 4 gives a 160 x 90 map: the seam declines before anything goes up, variable or not."""
    w, h = 640, 360
    fmt_args, fused_env = INTENTS[intent]
    with tempfile.TemporaryDirectory() as d:
        _write_intent(intent, w, h, d)
        args = ["-m", 0, "-p", "in.raw", "-w", w, "-h", h] + fmt_args + ["-s", 4, "-M", 0]
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        rc, _, err, trace = F.run_app(args + ["-z", "gpu.jpg"], True, d, env_extra=fused_env)
        assert rc == 0, err
        assert _per_stage(trace), trace
        _decoded_within_the_bar(d, "cpu", "gpu", w, h)
