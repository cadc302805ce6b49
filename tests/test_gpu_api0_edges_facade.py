"""GPU: API-0 encodes of frames that are not whole MCUs, or whose gain map is not whole blocks, through the facade -- the reference's
sample app on the drop-in libuhdr.so with -u 1.  With UHDR_HIP_SEAM_FUSED_API0_EDGES set (next to UHDR_HIP_SEAM_FUSED_P010 for a P010
intent and UHDR_HIP_SEAM_FUSED_SCALED_MAP for a sub-sampled map, which keep gating what they gate) the seam at JpegR::encodeJPEGR API-0
hands such a frame to uhdr_hip_encode_api0_scans_edges: one device stage, the file of the five per-stage seams byte for byte.  Without
the variable nothing changes: the per-stage seams run."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F
from tests.test_gpu_api0_scaled_facade import _decoded_within_the_bar, _per_stage, _write_intent

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

EDGES = {"UHDR_HIP_SEAM_FUSED_API0_EDGES": "1"}
RGBA_ARGS, P010_ARGS = ["-a", 5, "-C", 2, "-t", 2, "-R", 1], ["-a", 0, "-C", 2, "-t", 1, "-R", 0]
# (intent, w, h, sample-app arguments of the intent and the map, the variables that gate the rest of the request)
# 640 x 360 P010 at -s 4: h % 16 == 8 and a 160 x 90 map (1080p's patterns); 648 x 360 P010 at -s 1 with a three-channel map: w % 16 == 8
# as well; 636 x 356 RGBA1010102 at -s 4: w % 8 == 4, h % 8 == 4, a 159 x 89 map
CASES = [("p010", 640, 360, P010_ARGS + ["-s", 4, "-M", 0], {"UHDR_HIP_SEAM_FUSED_P010": "1", "UHDR_HIP_SEAM_FUSED_SCALED_MAP": "1"}),
         ("p010", 648, 360, P010_ARGS + ["-s", 1, "-M", 1], {"UHDR_HIP_SEAM_FUSED_P010": "1"}),
         ("rgba1010102", 636, 356, RGBA_ARGS + ["-s", 4, "-M", 0], {"UHDR_HIP_SEAM_FUSED_SCALED_MAP": "1"})]


@pytest.mark.parametrize("intent,w,h,more,gates", CASES)
def test_api0_encode_of_a_frame_that_is_not_whole_mcus_through_the_facade(intent, w, h, more, gates):
    with tempfile.TemporaryDirectory() as d:
        _write_intent(intent, w, h, d)
        args = ["-m", 0, "-p", "in.raw", "-w", w, "-h", h] + more
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        # with the variables: one device stage ...
        rc, _, err, trace = F.run_app(args + ["-z", "fused.jpg"], True, d, env_extra=dict(gates, **EDGES))
        assert rc == 0, err
        assert trace.on("device") == ["encode_api0_fused"], trace
        # ... and the file of the per-stage seams, byte for byte
        rc, _, err, trace = F.run_app(args + ["-z", "staged.jpg"], True, d, env_extra={"UHDR_HIP_SEAM_NO_FUSED_ENCODE": "1"})
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "staged.jpg")))
        # without the new variable: the per-stage seams and the same file
        rc, _, err, trace = F.run_app(args + ["-z", "plain.jpg"], True, d, env_extra=gates)
        assert rc == 0, err
        assert _per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "plain.jpg")), F.read(os.path.join(d, "staged.jpg")))
        _decoded_within_the_bar(d, "cpu", "fused", w, h)
