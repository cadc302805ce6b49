"""GPU: the DC terms of write form 3 on a dense side array (csrc/huffman_decode_sync.hip: write_span2<true> stores a block's DC
difference into HuffSyncArgs::dc_dense, dc_partial3_kernel / dc_apply3_kernel predict there and scatter the result to term 0 of the
JBLOCKs) and the fused API-1 decode that leaves the scatter out (csrc/api_jpeg.cpp: decode_api1_scans_impl; csrc/jpeg_decode.hip:
idct_dequant_rgb_kernel<4, true> takes term 0 of a three-channel map's blocks from the side array).

Content: quality 100 (every quantisation step 1), the AC terms of the noise-textured image of tests/mcu_layouts.py (scale 0.3, what
tests/test_gpu_huffman_straggler.py uses at q100), the DC terms written over it:
  "checker"  neighbouring blocks alternate between black (-1024) and white (+1016): DC differences of +-2040, category 11;
  "ramp"     every component's DC climbs and falls in steps of 1024 .. 2047 between -32700 and +32700: category 11 differences whose
             running sums come close to both ends of int16 (the kernels add in int and cast at the end).
Both are checked when a case is built.  The scans are coded on the CPU (oracle.loader, Annex K tables), hold at least 4096 bytes and
must take the parallel route: every decode is held to the entropy_decode_parallel counter, and the library's debug output
(UHDR_HIP_HUFF_DEBUG) has to name the write form that delivered.

  1. stand-alone huffman_decode against the oracle's decoder, every coefficient: three components 1x1 at 264 x 136 (1683 scan blocks:
     six DC chunks of 256 and 147 more), one component at 520 x 264 (2145 blocks) and at 512 x 256 (2048: exactly eight chunks);
  2. the fused decode (decode_api1_scans, 272 x 144, 4:2:0 base image, three-channel map at scale 1 / one-channel map) against
     huffman_decode2 + idct_dequant_rgb / idct_dequant + applyGainMapFromCoefficients, byte for byte;
  3. the same with UHDR_HIP_HUFF_WRITE=2 (form 2) and UHDR_HIP_HUFF_LEVELS=0 (the rounds), then the default again, in one context: the
     IDCT must not take a side array that form 3 did not deliver;
  4. a stand-alone decode into arrays that held 0x5555 everywhere: they come back whole, term 0 included.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from mcu_layouts import photo_coefs
from oracle import loader as L

pytestmark = pytest.mark.gpu

S444, S420, S400 = [(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)], [(1, 1)]
SAMPLINGS = {"444": S444, "400": S400}
CHUNK = 256  # scan positions per DC chunk (csrc/huffman_decode_sync.hip: kPlaceChunk)
FORM_LINE = re.compile(r"hypothesis decode kernels \(write form (\d)\)")
ATTEMPT = "paths handed to the straggler waves"
ROUNDS_LINE = re.compile(r"rounds decode of \d+ bytes, \d+ subsequences of \d+ bits \(write form (\d)\): (\w+)")
DEV = "cuda:0"
F16, RGBA, Y400 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_32bppRGBA8888, A.UHDR_IMG_FMT_8bppYCbCr400


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


# ---- content ----------------------------------------------------------------------------------------------------------------------------
def _dc_checker(rng, bh, bw):
    yy, xx = np.mgrid[0:bh, 0:bw]
    return np.where((yy + xx) % 2 == 0, -1024, 1016) + rng.integers(-3, 4, (bh, bw))


def _dc_ramp(rng, bh, bw):
    steps = rng.integers(1024, 2048, bh * bw)
    out, v, d = np.zeros(bh * bw, dtype=np.int64), 0, 1
    for i, s in enumerate(steps):
        if abs(v + d * int(s)) > 32700:
            d = -d
        v += d * int(s)
        out[i] = v
    return out.reshape(bh, bw)


@functools.lru_cache(maxsize=None)
def _case(name, w, h, kind):
    """(coefficients, the oracle's scan); built once, left unchanged."""
    sampling = SAMPLINGS[name]
    bw, bh = (w + 7) // 8, (h + 7) // 8
    rng = np.random.default_rng(31 * w + h + len(sampling) + (7 if kind == "ramp" else 0))
    coefs = photo_coefs(rng, [(bw, bh)] * len(sampling), 100, 0.3)
    for c in coefs:
        dc = (_dc_checker if kind == "checker" else _dc_ramp)(rng, bh, bw)
        c[..., 0] = dc.astype(np.int16)
        diff = np.diff(np.concatenate([[0], dc.ravel()]))  # 1x1 components: the scan visits a component's blocks in raster order
        assert 1024 <= np.abs(diff).max() <= 2047, "no DC difference of category 11"
        assert (np.abs(diff) >= 1024).mean() > 0.9
        if kind == "ramp":
            assert dc.max() > 31000 and dc.min() < -31000, "the running sums stay away from the ends of int16"
        c.setflags(write=False)
    scan = L.huffman_encode_port(coefs, w, h, sampling, 0)
    assert len(scan) >= 4096, len(scan)  # the parallel route's threshold
    return coefs, scan


def _dev(scan):
    import torch

    return torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to(DEV)


def _parallel(uhdr):
    st = A.Stats()
    uhdr.lib.uhdr_hip_get_stats(uhdr.ctx.handle, C.byref(st))
    return st.entropy_decode_parallel


def _delivered_by(err):
    """The write forms of the hypothesis attempts the debug output names, and the attempts' own lines (lost / resolved)."""
    forms = [int(m.group(1)) for m in FORM_LINE.finditer(err)]
    attempts = [ln for ln in err.splitlines() if ATTEMPT in ln]
    return forms, attempts


# ---- 1. stand-alone decode against the oracle's ------------------------------------------------------------------------------------------
CASES1 = [("444", 264, 136, 1683), ("400", 520, 264, 2145), ("400", 512, 256, 2048)]


@pytest.mark.parametrize("kind", ["checker", "ramp"])
@pytest.mark.parametrize("name,w,h,nblocks", CASES1)
def test_standalone_decode_equals_the_oracle(uhdr, monkeypatch, capfd, name, w, h, nblocks, kind):
    coefs, scan = _case(name, w, h, kind)
    sampling = SAMPLINGS[name]
    shapes = [c.shape[:2] for c in coefs]
    assert sum(a * b for a, b in shapes) == nblocks
    assert (nblocks % CHUNK == 0) == (nblocks == 2048) and nblocks > 6 * CHUNK
    rc, want = L.huffman_decode_port(shapes, w, h, sampling, 0, scan)
    assert rc == 0
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    capfd.readouterr()
    before = _parallel(uhdr)
    got = uhdr.huffman_decode(_dev(scan), shapes, w, h, sampling, 0)
    host = [g.cpu().numpy() for g in got]
    err = capfd.readouterr().err
    forms, attempts = _delivered_by(err)
    with capfd.disabled():
        print(f"\n{name} {w}x{h} {kind}, {len(scan)} bytes, write forms {forms}: " + " | ".join(a[-60:] for a in attempts))
    assert _parallel(uhdr) == before + 1
    assert forms and set(forms) == {3} and not ROUNDS_LINE.search(err), err  # form 3 delivered (a lost attempt is repeated in form 3)
    assert attempts and "true path resolved" in attempts[-1], err
    for c in range(len(coefs)):
        assert np.array_equal(host[c], want[c]), (name, kind, c, int((host[c] != want[c]).sum()))
        assert np.array_equal(want[c], coefs[c])


# ---- 4. arrays that held something else ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("444", 264, 136), ("400", 520, 264)])
def test_stale_arrays_come_back_whole(uhdr, monkeypatch, capfd, name, w, h):
    import torch

    coefs, scan = _case(name, w, h, "checker")
    sampling = SAMPLINGS[name]
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    outs = [torch.full(c.shape, 0x5555, dtype=torch.int16, device=DEV) for c in coefs]
    data = _dev(scan)
    sc = uhdr._scan(outs, w, h, sampling, 0)
    capfd.readouterr()
    before = _parallel(uhdr)
    uhdr._call(True, uhdr.lib.uhdr_hip_huffman_decode_dev, uhdr.ctx.handle, C.byref(sc), None, C.c_void_p(data.data_ptr()), data.numel())
    err = capfd.readouterr().err
    forms, attempts = _delivered_by(err)
    assert _parallel(uhdr) == before + 1
    assert forms and set(forms) == {3} and attempts and "true path resolved" in attempts[-1], err
    for c in range(len(coefs)):
        host = outs[c].cpu().numpy()
        assert np.array_equal(host[..., 0], coefs[c][..., 0]), (c, "term 0")
        assert np.array_equal(host, coefs[c]), c


# ---- 2. / 3. the fused decode against the staged route ------------------------------------------------------------------------------------
FW, FH = 272, 144  # 34 x 18 blocks, 17 x 9 MCUs of the 4:2:0 base image


@functools.lru_cache(maxsize=None)
def _base():
    rng = np.random.default_rng(20272144)
    coefs = photo_coefs(rng, [(34, 18), (17, 9), (17, 9)], 95, 2.0)
    for c in coefs:
        c.setflags(write=False)
    scan = L.huffman_encode_port(coefs, FW, FH, S420, 0)
    assert len(scan) >= 4096, len(scan)
    return coefs, scan


_staged_cache = {}


def _fused_setup(uhdr, nmap):
    """Headers, device scans, tables and -- computed once per map kind, then shared -- the staged route's pixels."""
    u = uhdr
    name = "444" if nmap == 3 else "400"
    base, scan_b = _base()
    mp, scan_m = _case(name, FW, FH, "checker")
    qy, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
    q1, q1c = L.quant_table_port(100, False), L.quant_table_port(100, True)
    hb = u.jpeg_header(FW, FH, S420, [qy, qc, qc])
    hm = u.jpeg_header(FW, FH, SAMPLINGS[name], [q1, q1c, q1c][:nmap])
    db, dm = _dev(scan_b), _dev(scan_m)
    md = synth.default_metadata()
    if nmap not in _staged_cache:
        before = _parallel(u)
        kb, km = u.huffman_decode2(db, [c.shape[:2] for c in base], FW, FH, S420, dm, [c.shape[:2] for c in mp], FW, FH, SAMPLINGS[name])
        assert _parallel(u) == before + 2
        for got, want in zip(kb + km, base + mp):
            assert np.array_equal(got.cpu().numpy(), want)
        if nmap == 3:
            gm = Image(RGBA, FW, FH, A.UHDR_CG_BT_2100, align=64, device=DEV)
            u.idct_dequant_rgb(km, q1, q1c, FW, FH, RGBA, 0, dst=gm)
        else:
            plane = u.idct_dequant(km[0], q1)
            u.ctx.synchronize()
            gm = Image(Y400, FW, FH, A.UHDR_CG_BT_2100)
            gm.valid(0)[:] = plane.cpu().numpy()[:FH, :FW]
            gm = gm.to(DEV)
        d2 = Image(F16, FW, FH, align=64, device=DEV)
        u.applyGainMapFromCoefficients(kb, [qy, qc, qc], FW, FH, A.UHDR_CG_BT_709, gm, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, d2)
        u.ctx.synchronize()
        want = d2.to_host().valid(0).copy()
        want.setflags(write=False)
        assert want.any()
        _staged_cache[nmap] = want
    return hb, db, hm, dm, md, _staged_cache[nmap]


def _fused(uhdr, capfd, hb, db, hm, dm, md):
    """One decode_api1_scans call: (pixels, the debug output); both scans must have taken the parallel route."""
    dst = Image(F16, FW, FH, align=64, device=DEV)
    capfd.readouterr()
    before = _parallel(uhdr)
    uhdr.decodeApi1Scans(hb, db, A.UHDR_CG_BT_709, hm, dm, A.UHDR_CG_BT_2100, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dst)
    uhdr.ctx.synchronize()
    err = capfd.readouterr().err
    assert _parallel(uhdr) == before + 2, err
    return dst.to_host().valid(0), err


@pytest.mark.parametrize("nmap", [3, 1])
def test_fused_decode_equals_the_staged_route(uhdr, monkeypatch, capfd, nmap):
    hb, db, hm, dm, md, want = _fused_setup(uhdr, nmap)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    got, err = _fused(uhdr, capfd, hb, db, hm, dm, md)
    forms, attempts = _delivered_by(err)
    assert sorted(set(forms)) == [2, 3] and not ROUNDS_LINE.search(err), err  # the base image's form 2, the map's form 3
    assert sum("true path resolved" in a for a in attempts) == 2, err  # (the two scans' lines come from two threads, in any order)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("nmap", [3, 1])
def test_other_routes_then_the_default_again(uhdr, monkeypatch, capfd, nmap):
    hb, db, hm, dm, md, want = _fused_setup(uhdr, nmap)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    got, err = _fused(uhdr, capfd, hb, db, hm, dm, md)  # the default first: a side array of this context now holds the map's terms
    assert 3 in _delivered_by(err)[0], err
    assert np.array_equal(got, want)

    monkeypatch.setenv("UHDR_HIP_HUFF_WRITE", "2")
    got, err = _fused(uhdr, capfd, hb, db, hm, dm, md)
    forms, _ = _delivered_by(err)
    assert forms and set(forms) == {2} and not ROUNDS_LINE.search(err), err
    assert np.array_equal(got, want), ("form 2", int((got != want).sum()))
    monkeypatch.delenv("UHDR_HIP_HUFF_WRITE")

    monkeypatch.setenv("UHDR_HIP_HUFF_LEVELS", "0")
    got, err = _fused(uhdr, capfd, hb, db, hm, dm, md)
    rounds = ROUNDS_LINE.findall(err)
    assert len(rounds) == 2 and all(r[1] == "settled" for r in rounds) and not FORM_LINE.search(err), err
    assert np.array_equal(got, want), ("rounds", int((got != want).sum()))
    monkeypatch.delenv("UHDR_HIP_HUFF_LEVELS")

    got, err = _fused(uhdr, capfd, hb, db, hm, dm, md)
    assert 3 in _delivered_by(err)[0] and not ROUNDS_LINE.search(err), err
    assert np.array_equal(got, want), ("default again", int((got != want).sum()))
