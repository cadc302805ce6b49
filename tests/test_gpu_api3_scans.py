"""GPU: the one-call API-3 encode (uhdr_hip_encode_api3_scans / _dev: a compressed SDR intent + a raw HDR intent -> the gain map's
scan) against the staged chain of public entry points -- uhdr_hip_jpeg_decode_scan -> uhdr_hip_generate_gainmap_dev (sdr_is_601 = 1)
-> uhdr_hip_fdct_quant_dev / _rgb_dev -> uhdr_hip_huffman_encode_dev: the map's scan byte for byte, metadata and description equal.
The SDR intent's scan is written by the oracle's Huffman coder from the test's coefficients, so no reference binary is needed."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLINGS = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "440": [(1, 2), (1, 1), (1, 1)], "gray": [(1, 1)]}
FMT = {"420": A.UHDR_IMG_FMT_12bppYCbCr420, "422": A.UHDR_IMG_FMT_16bppYCbCr422, "444": A.UHDR_IMG_FMT_24bppYCbCr444}
BT709, BT2100 = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
BEST, REALTIME = A.UHDR_USAGE_BEST_QUALITY, A.UHDR_USAGE_REALTIME
UNSUP = A.UHDR_CODEC_UNSUPPORTED_FEATURE
# (scale factor, w, h): 256 x 144 at 1, 512 x 288 at 4 (a 128 x 72 map)
GEOMETRIES = ((1, 256, 144), (4, 512, 288))


def grids(w, h, sampling):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8) for hs, vs in sampling]


@functools.lru_cache(maxsize=None)
def sdr_case(w, h, sampling):
    """(header, entropy-coded bytes, tables) of a compressed SDR intent: a smooth field + noise through the oracle's FDCT on libjpeg's
    grids, three different tables, the oracle's Huffman coder.  Built once per geometry and left unchanged."""
    from libultrahdr_amd.ultrahdr import UltraHdr

    rng = np.random.default_rng(7 * w + h + int(sampling))
    dims = grids(w, h, SAMPLINGS[sampling])
    qts = [L.quant_table_port(90, False), L.quant_table_port(90, True), L.quant_table_port(80, True)]
    coefs = []
    for c, (bw, bh) in enumerate(dims):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
        pl = 128 + 90 * np.sin(xx / (13.0 + 5 * c)) * np.cos(yy / (9.0 + 3 * c)) + rng.normal(0, 12, (bh * 8, bw * 8))
        coefs.append(L.fdct_quant_port(np.ascontiguousarray(np.clip(pl, 0, 255).astype(np.uint8)), bw * 8, bw, bh, qts[c]))
    scan = L.huffman_encode_port(coefs, w, h, SAMPLINGS[sampling], 0)
    hd = UltraHdr.jpeg_header(w, h, SAMPLINGS[sampling], qts)
    bits, vals = L.std_dht_tables()  # the file's DHT segments: uhdr_hip_jpeg_decode_scan takes them as they are
    for t in range(4):
        for i in range(17):
            hd.tables.bits[t][i] = int(bits[t][i])
        for i in range(256):
            hd.tables.vals[t][i] = int(vals[t][i])
    return hd, scan, qts


@functools.lru_cache(maxsize=None)
def hdr_case(w, h):
    img = synth.make_hdr_p010(w, h, seed=21, ct=A.UHDR_CT_HLG, cg=BT2100, noise=0.05)
    return img, img.to(DEV)


def map_tables():
    return L.quant_table_port(85, False), L.quant_table_port(85, True)


def uhdr_for(ctx, scale, nch, preset, gamma=1.0):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=ctx, mapDimensionScaleFactor=scale, useMultiChannelGainMap=(nch == 3), gamma=gamma, preset=preset)


def _desc(r):
    return (r.fmt, r.w, r.h, r.cg, r.ct, r.range)


def one_call_dev(u, w, h, sampling, zero_dht=False):
    """(map scan bytes, metadata dict, description) through uhdr_hip_encode_api3_scans_dev.  zero_dht: the header's DHT block all zero,
    which selects the Annex K tables."""
    import torch

    hdr_j, scan, _ = sdr_case(w, h, sampling)
    if zero_dht:
        hdr_j = A.JpegHeader.from_buffer_copy(hdr_j)
        C.memset(C.byref(hdr_j.tables), 0, C.sizeof(hdr_j.tables))
    data = torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to(DEV)
    out = torch.empty(w * h * 4 + 4096, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    n, md, desc = u.encodeApi3Scans(hdr_j, data, BT709, hdr_case(w, h)[1], map_tables(), out)
    return out[:n].cpu().numpy().tobytes(), md.as_dict(), _desc(desc)


def one_call_host(u, w, h, sampling, capacity=None):
    hdr_j, scan, _ = sdr_case(w, h, sampling)
    got, md, desc = u.encodeApi3Scans(hdr_j, scan, BT709, hdr_case(w, h)[0], map_tables(), capacity if capacity is not None else w * h * 4 + 4096)
    return got, md.as_dict(), _desc(desc)


def staged_chain(u, w, h, sampling):
    """The public entry points one after the other: jpeg_decode_scan (host planes) -> generateGainMap (sdr_is_601) -> FDCT -> Huffman."""
    hdr_j, scan, _ = sdr_case(w, h, sampling)
    sc = hdr_j.scan
    buf = np.frombuffer(scan, dtype=np.uint8)
    outs = [np.empty((sc.blocks_h[c] * 8, sc.blocks_w[c] * 8), dtype=np.uint8) for c in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
    hs, vs = (C.c_uint * 3)(*[o.shape[1] for o in outs]), (C.c_uint * 3)(*[o.shape[0] for o in outs])
    u._call(False, u.lib.uhdr_hip_jpeg_decode_scan, u.ctx.handle, C.byref(hdr_j), C.c_void_p(buf.ctypes.data), buf.size, 0, 0, ptrs, hs, vs)
    sdr = Image(FMT[sampling], w, h, BT709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, 64)
    for c in range(3):
        sdr.valid(c)[:] = outs[c][: sdr.valid(c).shape[0], : sdr.valid(c).shape[1]]
    md, gm = u.generateGainMap(sdr.to(DEV), hdr_case(w, h)[1], True, True)
    u.ctx.synchronize()
    ql, qc = map_tables()
    if u.mUseMultiChannelGainMap:
        coefs = u.fdct_quant_rgb(gm, ql, qc)
    else:
        pl = gm.plane_tensor(0)
        coefs = [u.fdct_quant(pl, pl.shape[1], gm.w // 8, gm.h // 8, ql)]
    out = u.huffman_encode(coefs, gm.w, gm.h, [(1, 1)] * len(coefs), 0)
    u.ctx.synchronize()
    return out.cpu().numpy().tobytes(), md.as_dict(), _desc(gm.raw)


# ---- the one-call forms against the staged public chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["420", "422", "444"])
@pytest.mark.parametrize("preset", [BEST, REALTIME], ids=["two-pass", "one-pass"])
def test_one_call_equals_the_staged_public_chain(hip_ctx, sampling, preset):
    for nch in (1, 3):
        for (scale, w, h) in GEOMETRIES:
            u = uhdr_for(hip_ctx, scale, nch, preset)
            want = staged_chain(u, w, h, sampling)
            assert want[2][:3] == (A.UHDR_IMG_FMT_24bppRGB888 if nch == 3 else A.UHDR_IMG_FMT_8bppYCbCr400, w // scale, h // scale)
            for name, got in (("_dev", one_call_dev(u, w, h, sampling)), ("host", one_call_host(u, w, h, sampling))):
                what = f"{name} {sampling} ch={nch} S={scale}"
                assert len(got[0]) == len(want[0]) and got[0] == want[0], f"{what}: map scans differ ({len(got[0])} / {len(want[0])} bytes)"
                assert got[1] == want[1], f"{what}: metadata {got[1]} != {want[1]}"
                assert got[2] == want[2], f"{what}: description {got[2]} != {want[2]}"
    assert one_call_dev(u, w, h, sampling, zero_dht=True) == want, "an all-zero DHT block selects the Annex K tables"


# ---- the route switch -------------------------------------------------------------------------------------------------------------------
def probe():
    """What tests/api3_route_probe.py prints: the _dev one-call form's results for 4:2:0 and 4:2:2, both presets."""
    import hashlib

    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    res = {}
    try:
        for sampling in ("420", "422"):
            for preset in (BEST, REALTIME):
                for (nch, (scale, w, h)) in ((3, GEOMETRIES[0]), (1, GEOMETRIES[1])):
                    scan, md, desc = one_call_dev(uhdr_for(ctx, scale, nch, preset), w, h, sampling)
                    res[f"{sampling}-{preset}-{nch}-{scale}"] = [hashlib.sha256(scan).hexdigest(), len(scan), md, list(desc)]
    finally:
        ctx.close()
    return res


def test_both_routes_give_the_same_bytes(hip_ctx):
    """UHDR_HIP_API3_ROUTE=fused (the coefficient kernel) and =staged (three IDCT launches + generate_gainmap), each in a fresh child
    process; and both equal the staged public chain computed here."""
    import hashlib

    results = {}
    for route in ("fused", "staged"):
        env = dict(os.environ)
        env["UHDR_HIP_API3_ROUTE"] = route
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "api3_route_probe.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        results[route] = json.loads(p.stdout.strip().splitlines()[-1])
    assert results["fused"] == results["staged"]
    assert len(results["fused"]) == 8
    want = staged_chain(uhdr_for(hip_ctx, 1, 3, BEST), 256, 144, "422")
    assert results["fused"][f"422-{BEST}-3-1"][:2] == [hashlib.sha256(want[0]).hexdigest(), len(want[0])]


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [True, False], ids=["_dev", "host"])
def test_a_capacity_that_is_too_small_reports_the_needed_size(hip_ctx, dev):
    import torch

    w, h = 256, 144
    u = uhdr_for(hip_ctx, 1, 3, BEST)
    want = staged_chain(u, w, h, "420")
    hdr_j, scan, _ = sdr_case(w, h, "420")
    with pytest.raises(A.UhdrError) as e:
        if dev:
            data = torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to(DEV)
            out = torch.empty(64, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()
            u.encodeApi3Scans(hdr_j, data, BT709, hdr_case(w, h)[1], map_tables(), out)
        else:
            one_call_host(u, w, h, "420", capacity=64)
    # the needed size is the entropy coder's: enough for the scan (the siblings report the same figure), and the second call succeeds with it
    assert e.value.code == A.UHDR_CODEC_MEM_ERROR and len(want[0]) <= e.value.needed < 2 * len(want[0])
    if dev:
        out = torch.empty(e.value.needed, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        n, md, desc = u.encodeApi3Scans(hdr_j, data, BT709, hdr_case(w, h)[1], map_tables(), out)
        got = (out[:n].cpu().numpy().tobytes(), md.as_dict(), _desc(desc))
    else:
        got = one_call_host(u, w, h, "420", capacity=e.value.needed)
    assert got == want


# ---- what the one-call form declines ----------------------------------------------------------------------------------------------------
def _refused(ctx, u, hdr_j, w, h, dev, detail):
    """UNSUPPORTED_FEATURE, the message sends the caller to the operators, and nothing was written: metadata, description, scan buffer,
    byte count."""
    import torch

    md, desc = A.GainmapMetadata(), A.RawImage()
    C.memset(C.byref(md), 0x5A, C.sizeof(md))
    C.memset(C.byref(desc), 0x5A, C.sizeof(desc))
    before = bytes(md), bytes(desc)
    nm = C.c_size_t(12345)
    cfg = u.encode_cfg(True, True)
    qm = np.ascontiguousarray(np.stack(map_tables()))
    himg, dimg = hdr_case(w, h)
    if dev:
        data = torch.zeros(4096, dtype=torch.uint8, device=DEV)
        out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        st = ctx.lib.uhdr_hip_encode_api3_scans_dev(ctx.handle, C.byref(hdr_j), C.c_void_p(data.data_ptr()), 4096, BT709, C.byref(dimg.raw), C.byref(cfg),
                                                    C.c_void_p(qm.ctypes.data), C.byref(md), C.byref(desc), C.c_void_p(out.data_ptr()), 4096, C.byref(nm))
        ctx.synchronize()
        untouched = bool((out == 0x5A).all())
    else:
        data, out = np.zeros(4096, np.uint8), np.full(4096, 0x5A, np.uint8)
        st = ctx.lib.uhdr_hip_encode_api3_scans(ctx.handle, C.byref(hdr_j), C.c_void_p(data.ctypes.data), 4096, BT709, C.byref(himg.raw), C.byref(cfg),
                                                C.c_void_p(qm.ctypes.data), C.byref(md), C.byref(desc), C.c_void_p(out.ctypes.data), 4096, C.byref(nm))
        untouched = bool((out == 0x5A).all())
    assert st.error_code == UNSUP, (st.error_code, st.detail)
    assert detail in st.detail and b"use the operators" in st.detail, st.detail
    assert (bytes(md), bytes(desc)) == before and untouched and nm.value == 12345


@pytest.mark.parametrize("dev", [True, False], ids=["_dev", "host"])
def test_declines_write_nothing(hip_ctx, dev):
    from libultrahdr_amd.ultrahdr import UltraHdr

    w, h = 256, 144
    qts = sdr_case(w, h, "420")[2]
    u = uhdr_for(hip_ctx, 1, 1, BEST)
    good = sdr_case(w, h, "420")[0]
    _refused(hip_ctx, u, UltraHdr.jpeg_header(w, h, SAMPLINGS["gray"], qts[:1]), w, h, dev, b"4:2:0, 4:2:2 or 4:4:4")
    _refused(hip_ctx, u, UltraHdr.jpeg_header(w, h, SAMPLINGS["440"], qts), w, h, dev, b"4:2:0, 4:2:2 or 4:4:4")
    _refused(hip_ctx, uhdr_for(hip_ctx, 1, 1, BEST, gamma=1.3), good, w, h, dev, b"gamma 1")
    # a 130 x 18 map: not whole 8 x 8 blocks
    _refused(hip_ctx, u, UltraHdr.jpeg_header(130, 18, SAMPLINGS["420"], qts), 130, 18, dev, b"multiples of 8")
    _refused(hip_ctx, uhdr_for(hip_ctx, 2, 1, REALTIME), UltraHdr.jpeg_header(260, 36, SAMPLINGS["422"], qts), 260, 36, dev, b"multiples of 8")


def test_a_progressive_file_never_becomes_a_header():
    """uhdr_hip_jpeg_header_t has no field that could say "progressive": uhdr_hip_jpeg_parse, which fills it, refuses such a file (-8),
    so the one-call form is never reached with one."""
    PILImage = pytest.importorskip("PIL.Image")
    import io

    buf = io.BytesIO()
    PILImage.fromarray(np.full((64, 64, 3), 77, dtype=np.uint8), "RGB").save(buf, "JPEG", progressive=True)
    hdr = A.JpegHeader()
    raw = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    assert A.load().uhdr_hip_jpeg_parse(C.c_void_p(raw.ctypes.data), raw.size, C.byref(hdr)) == -8
