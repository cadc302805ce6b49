"""GPU: an RGBA8888 SDR intent that is off the block grid -- in the frame (44 x 40) or in the map only (64 x 56 at scale factor 4, 1080p's
pattern) -- through the reference's sample app (ultrahdr_app -m 0, API-1) linked against the facade libuhdr.so.  With
UHDR_HIP_SEAM_FUSED_RGBA_SDR and UHDR_HIP_SEAM_FUSED_RGBA_EDGES the seam hands it to uhdr_hip_encode_api1_scans_edges with
UHDR_HIP_ENCODE_RGBA_EDGES: one device stage, the file the per-stage seams write, the CPU reference's pixels within the bar of
tests/test_gpu_api1_rgba_facade.py.  Without the new variable the per-stage seams run as before."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F
from tests import test_gpu_api1_rgba_facade as RF

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

FUSED = {"UHDR_HIP_SEAM_FUSED_RGBA_SDR": "1", "UHDR_HIP_SEAM_FUSED_RGBA_EDGES": "1"}


@pytest.mark.parametrize("w,h,scale", [(64, 56, 4), (44, 40, 1)])
def test_rgba_api1_encode_off_the_block_grid_takes_the_fused_route_when_asked_to(w, h, scale):
    with tempfile.TemporaryDirectory() as d:
        args = RF._write_intents(d, w, h) + ["-s", scale]
        rc, _, err, _ = F.run_app(args + ["-z", "cpu.jpg"], False, d)
        assert rc == 0, err
        rc, _, err, trace = F.run_app(args + ["-z", "fused.jpg"], True, d, env_extra=FUSED)
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        # the file the per-stage seams write, byte for byte
        rc, _, err, trace = F.run_app(args + ["-z", "stages.jpg"], True, d, env_extra={"UHDR_HIP_SEAM_NO_FUSED_ENCODE": "1"})
        assert rc == 0, err
        assert RF._is_per_stage(trace), trace
        a, b = F.read(os.path.join(d, "fused.jpg")), F.read(os.path.join(d, "stages.jpg"))
        assert a.size == b.size and np.array_equal(a, b), (a.size, b.size)
        RF._assert_pixels_close(RF._decoded(d, "cpu"), RF._decoded(d, "fused"), w * h * 4, "fused")
        # without the new variable nothing changes, whatever else is set: the per-stage seams, the same file
        env = {"UHDR_HIP_SEAM_FUSED_RGBA_SDR": "1", "UHDR_HIP_SEAM_FUSED_EDGES": "1"}
        rc, _, err, trace = F.run_app(args + ["-z", "default.jpg"], True, d, env_extra=env)
        assert rc == 0, err
        assert RF._is_per_stage(trace), trace
        assert np.array_equal(F.read(os.path.join(d, "default.jpg")), b)
