"""GPU: the reference's sample app through the facade with a gain-map gamma other than 1 (ultrahdr_app -m 0 ... -G 1.571).  With
UHDR_HIP_SEAM_GAMMA_ENCODE the seam at JpegR::encodeJPEGR (API-1) hands the encode to uhdr_hip_encode_api1_scans_ex with
UHDR_HIP_GENERATE_GAMMA_TABLE: ONE device stage, and the file is the CPU reference's byte for byte (the gain map's bytes come from
thresholds built with the host libm the reference calls).  Without the variable nothing changes: the fused chain declines the gamma and the
per-stage seams run."""
import os
import tempfile

import numpy as np
import pytest

from tests import facade_util as F
from tests import fixture720

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.built(), reason="facade not built")]

GAMMA = ("-G", 1.571)


def _fixture(d):
    g = fixture720.gold()
    g["p010"].tofile(os.path.join(d, "in.p010"))
    g["yuv420"].tofile(os.path.join(d, "in.yuv420"))
    return os.path.join(d, "in.p010"), os.path.join(d, "in.yuv420")


@pytest.mark.parametrize("extra,env", [(("-M", 1, "-s", 1), {}), (("-M", 1, "-s", 1, "-D", 0), {"UHDR_HIP_SEAM_FUSED_REALTIME": "1"})],
                         ids=["best-quality", "realtime"])
def test_gamma_encode_through_the_facade_is_one_device_stage_and_the_cpu_reference_file(extra, env):
    with tempfile.TemporaryDirectory() as d:
        p, y = _fixture(d)
        extra = tuple(extra) + GAMMA
        rc, _, err, _ = F.encode_api1(p, y, 1280, 720, "cpu.jpg", False, d, extra=extra)
        assert rc == 0, err
        rc, _, err, trace = F.encode_api1(p, y, 1280, 720, "gpu.jpg", True, d, extra=extra, env_extra=dict(env, UHDR_HIP_SEAM_GAMMA_ENCODE="1"))
        assert rc == 0, err
        assert trace.on("device") == ["encode_api1_fused"], trace
        a, b = F.read(os.path.join(d, "cpu.jpg")), F.read(os.path.join(d, "gpu.jpg"))
        assert a.size == b.size and np.array_equal(a, b), f"{a.size} / {b.size} bytes, {int((a[:min(a.size, b.size)] != b[:min(a.size, b.size)]).sum())} differ"
        # without the variable: what it is today -- the fused chain declines the gamma, the per-stage seams take the encode
        rc, _, err, trace = F.encode_api1(p, y, 1280, 720, "gpu0.jpg", True, d, extra=extra, env_extra=env)
        assert rc == 0, err
        st = trace.on("device")
        assert "encode_api1_fused" not in st and "generate_gainmap" in st and trace.n("jpeg_encode_scan") == 2, trace
