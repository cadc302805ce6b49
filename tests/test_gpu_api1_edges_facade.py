"""GPU: the reference's sample app through the facade on frames that are not whole MCUs / whose map is not whole blocks.  With
UHDR_HIP_SEAM_FUSED_EDGES the seam at JpegR::encodeJPEGR (API-1) hands the encode to uhdr_hip_encode_api1_scans_edges: ONE device stage, and
the file is the CPU reference's byte for byte.  Without the variable nothing changes: the per-stage seams run."""
import os
import tempfile

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from tests import facade_util as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]


def _inputs(d, w, h):
    """Tightly packed raw files, as the app reads them."""
    sdr = synth.make_sdr_yuv420(w, h, seed=w + 2 * h, noise=0.05, align=1)
    hdr = synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=A.UHDR_CT_HLG, noise=0.05, align=1)
    p, y = os.path.join(d, "in.p010"), os.path.join(d, "in.yuv420")
    np.concatenate([hdr.valid(i).reshape(-1) for i in range(2)]).tofile(p)
    np.concatenate([sdr.valid(i).reshape(-1) for i in range(3)]).tofile(y)
    return p, y


# 64 x 56 at scale 4: whole-MCU columns, h % 16 == 8, map 16 x 14 (1080p's pattern); 40 x 48 at scale 1: w % 16 == 8, the map 40 x 48
@pytest.mark.parametrize("w,h,s", [(64, 56, 4), (40, 48, 1)])
def test_edges_encode_through_the_facade_is_one_device_stage_and_the_cpu_reference_file(w, h, s):
    with tempfile.TemporaryDirectory() as d:
        p, y = _inputs(d, w, h)
        extra = ("-M", 1, "-s", s)
        rc, _, err, _ = F.encode_api1(p, y, w, h, "cpu.jpg", False, d, extra=extra)
        assert rc == 0, err
        rc, _, err, trace = F.encode_api1(p, y, w, h, "gpu.jpg", True, d, extra=extra, env_extra={"UHDR_HIP_SEAM_FUSED_EDGES": "1"})
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        a, b = F.read(os.path.join(d, "cpu.jpg")), F.read(os.path.join(d, "gpu.jpg"))
        assert a.size == b.size and np.array_equal(a, b), f"{a.size} / {b.size} bytes, {int((a[:min(a.size, b.size)] != b[:min(a.size, b.size)]).sum())} differ"
        # without the variable: what it is today -- the per-stage seams take the encode
        rc, _, err, trace = F.encode_api1(p, y, w, h, "gpu0.jpg", True, d, extra=extra)
        assert rc == 0, err
        assert "encode_api1_fused" not in trace.on("device") and "generate_gainmap" in trace.on("device"), trace
