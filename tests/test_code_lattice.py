"""The code-lattice images of tests/code_lattice.py, on the CPU: what the builders guarantee, that the C restatement
("port") equals the real reference ("ref") bit for bit on every case tests/test_gpu_code_lattice.py runs on the device,
and that the lattice drives the reference to the ends of its own ranges -- both clamps of the log2 content boost
(jpegr.cpp:969-986), both ends of the 8-bit map, the linear output ceiling 10000/203 (clampPixelFloatLinear).  The tests
that need the real reference are skipped where oracle/_ref is not built."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import code_lattice as CL
from libultrahdr_amd import capi as A
from oracle import loader as L

SDR_FMTS = [CL.S420, CL.S422, CL.S444, CL.SRGBA]
HDR_FMTS = [CL.HP010, CL.H444, CL.H1010102]
SIZES = [CL.SIZE_MAIN, CL.SIZE_PIXEL]


def _build(fmt, size, seed=CL.SEED):
    if fmt in SDR_FMTS:
        return CL.sdr(fmt, *size, seed=seed)
    return CL.hdr(fmt, *size, ct=CL.PQ, seed=seed)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", SDR_FMTS + HDR_FMTS)
def test_every_code_in_every_channel_and_same_bytes_for_same_seed(fmt, size):
    img = _build(fmt, size)
    n = 256 if fmt in SDR_FMTS else 1024
    for c, plane in enumerate(CL.channels(img)):
        assert np.array_equal(np.unique(plane), np.arange(n)), f"channel {c}"
    assert np.array_equal(img.buf, _build(fmt, size).buf)
    assert not np.array_equal(img.buf, _build(fmt, size, seed=CL.SEED + 1).buf)
    # the ramps: every code in all channels at once / luma with neutral chroma, and in each channel against 0 in the others
    c0, c1, c2 = [p.reshape(-1) for p in CL.at_pixels(img)]
    mid = 0 if fmt in (CL.SRGBA, CL.H1010102) else n // 2
    for code in (0, 1, n // 2, n - 2, n - 1):
        if mid:
            assert ((c0 == code) & (c1 == mid) & (c2 == mid)).any(), code
        else:
            assert ((c0 == code) & (c1 == code) & (c2 == code)).any(), code
        for a, b, c in ((c0, c1, c2), (c1, c0, c2), (c2, c0, c1)):
            assert ((a == code) & (b == 0) & (c == 0)).any(), code


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(CL.PAIRS))
def test_corner_pairs_are_present(name, size):
    sdr, hdr = CL.pair(name, size)
    s, h = CL.at_pixels(sdr), CL.at_pixels(hdr)
    rgb = sdr.fmt == CL.SRGBA
    black = (s[0] == 0) & ((s[1] == 0) & (s[2] == 0) if rgb else (s[1] == 128) & (s[2] == 128))
    white = (s[0] == 255) & ((s[1] == 255) & (s[2] == 255) if rgb else (s[1] == 128) & (s[2] == 128))
    peak = (h[0] == 1023) & ((h[1] == 1023) & (h[2] == 1023) if rgb else (h[1] == 512) & (h[2] == 512))
    zero = (h[0] == 0) & ((h[1] == 0) & (h[2] == 0) if rgb else (h[1] == 512) & (h[2] == 512))
    for a in (black, white):
        for b in (peak, zero):
            assert (a & b).any()
    # single channels too: SDR 0 against HDR max and the other way round, in every channel
    for c in range(3):
        assert ((s[c] == 0) & (h[c] == 1023)).any() and ((s[c] == 255) & (h[c] == 0)).any(), c
    if not rgb:
        # limited-range codes below and above the nominal range (luma 64..940, chroma 64..960; 8 bit: 16..235 / 16..240)
        assert (h[0] < 64).any() and (h[0] > 940).any()
        assert all((h[c] < 64).any() and (h[c] > 960).any() for c in (1, 2))
        assert (s[0] < 16).any() and (s[0] > 235).any()
        # YCbCr triples outside the RGB cube: black or white luma with chroma at an end
        for img, lo, hi in ((s, 0, 255), (h, 0, 1023)):
            for y in (lo, hi):
                for c in (1, 2):
                    assert ((img[0] == y) & (img[c] == lo)).any() and ((img[0] == y) & (img[c] == hi)).any()


def _same(a, b):
    return (a.fmt, a.w, a.h, a.raw.cg, a.raw.ct, a.raw.range) == (b.fmt, b.w, b.h, b.raw.cg, b.raw.ct, b.raw.range) and \
        all(np.array_equal(x, y) for x, y in zip(a.planes_valid(), b.planes_valid()))


@pytest.fixture(scope="module")
def pairs():
    return {name: CL.pair(name) for name in CL.PAIRS}


@pytest.mark.parametrize("name,cfg_name", CL.GENERATE_CASES + [c for c in CL.APPLY_MAPS if c not in CL.GENERATE_CASES])
def test_generate_gainmap_port_equals_ref(ref, pairs, name, cfg_name):
    sdr, hdr = pairs[name]
    cfg = CL.cfg(cfg_name)
    md_p, gm_p = L.generate_gainmap("port", sdr, hdr, cfg)
    md_r, gm_r = L.generate_gainmap("ref", sdr, hdr, cfg)
    assert _same(gm_p, gm_r)
    assert bytes(md_p) == bytes(md_r), (md_p.as_dict(), md_r.as_dict())


@pytest.mark.parametrize("key,ct,size", CL.TONEMAP_CASES)
def test_tone_map_port_equals_ref(ref, key, ct, size):
    hdr = CL.tonemap_image(key, ct, size)
    assert _same(L.tone_map("port", hdr), L.tone_map("ref", hdr))


@pytest.mark.parametrize("m,ct,boost", CL.APPLY_CASES)
def test_apply_gainmap_port_equals_ref(ref, pairs, m, ct, boost):
    name, cfg_name = CL.APPLY_MAPS[m]
    sdr, hdr = pairs[name]
    md, gm = L.generate_gainmap("ref", sdr, hdr, CL.cfg(cfg_name))
    assert _same(L.apply_gainmap("port", sdr, gm, md, ct, boost), L.apply_gainmap("ref", sdr, gm, md, ct, boost))


# Why one pair is left out of the upper clamp.  computeGain caps a channel whose SDR value is below 2/255 nits at 2.3
# (gainmapmath.cpp:773-782), so log2(max boost) reaches 15.6 only where hdr / sdr >= 2^15.6 = 49667 with sdr >= 2/255 nits.
# The reference converts the HDR pixel to the SDR gamut, never the SDR pixel (jpegr.cpp:608-622), so an RGBA8888 channel
# is srgbInvOetf(code / 255) * 203 nits exactly: 0 or >= 0.0616 nits (code 1).  That asks for an HDR channel of 3060 nits,
# which PQ has and HLG, with its 1000 nit peak, has not: with RGBA8888 + HLG the largest boost is 1000 / 0.0616 = 2^13.99.
# A YCbCr SDR image has channel values between the sRGB codes (triples outside the cube), so its HLG pairs do get there.
BELOW_UPPER_CLAMP = {"rgba+1010102-hlg-709"}


@pytest.mark.parametrize("name", list(CL.PAIRS))
def test_lattice_drives_the_reference_to_both_clamps_and_both_map_ends(ref, pairs, name):
    sdr, hdr = pairs[name]
    md, gm = L.generate_gainmap("ref", sdr, hdr, CL.cfg("default"))
    assert md.min_content_boost[0] == CL.CLAMP_MIN_BOOST == float(np.float32(4.957594501320273e-05))
    if name in BELOW_UPPER_CLAMP:
        assert 2.0 ** 13.9 < md.max_content_boost[0] < CL.CLAMP_MAX_BOOST
    else:
        assert md.max_content_boost[0] == CL.CLAMP_MAX_BOOST == 49667.01171875
    g = gm.valid(0)
    assert (g == 0).any() and (g == 255).any()


def test_lattice_map_applied_reaches_the_linear_ceiling(ref, pairs):
    name, cfg_name = CL.APPLY_MAPS[0]
    sdr, hdr = pairs[name]
    md, gm = L.generate_gainmap("ref", sdr, hdr, CL.cfg(cfg_name))
    out = L.apply_gainmap("ref", sdr, gm, md, A.UHDR_CT_LINEAR).valid(0).view(np.float16).reshape(sdr.h, sdr.w, 4)
    assert (out[..., :3] == np.float16(10000.0 / 203.0)).any()
    assert out[..., :3].max() == np.float16(10000.0 / 203.0)


def test_the_grey_sample_one_code_off_on_the_device_is_powf_rounding(tmp_path):
    """tests/test_gpu_code_lattice.py measures one tone-map sample where the HIP path is one code below the reference (Cr 127 / 128 of the
    grey pixel Y 276 of the limited-range PQ 4:4:4 image).  tests/probe_lattice_grey_site.c re-runs that pixel on the CPU: the reference's
    code with glibc's powf in srgbOetf, the HIP path's with a correctly rounded pow -- the site of tests/test_tonemap_site.py.  (Skipped
    where the C library's powf rounds this argument differently.)"""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe = str(tmp_path / "grey_site")
    subprocess.check_call(["gcc", "-O2", "-o", exe, "probe_lattice_grey_site.c", "-lm"], cwd=os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {v: int(re.search(r"V (\d+)", line).group(1)) for v, line in re.findall(r"variant (glibc powf|correctly rounded pow): (.*)", out)}
    if got["glibc powf"] != 128:
        pytest.skip(f"this C library's powf rounds the sample differently ({got})")
    assert got["correctly rounded pow"] == 127, got
