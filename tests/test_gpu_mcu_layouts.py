"""GPU: the entropy codec on every MCU layout check_scan (csrc/api_entropy.cpp) accepts -- the 63 three-component layouts of
tests/mcu_layouts.py, 3 .. 10 blocks per MCU -- where the rest of the suite runs four (4:4:4, 4:2:0, 4:2:2, one component).  The layout
decides the encoder's lane map (huffman_encode.hip: MCU and component of a lane, the DC prediction's lane, dummy blocks, live lanes per
wavefront, restart intervals per wavefront), the decoder's hypothesis geometry (64 x blocks-per-MCU threads, slot rows of levels x
blocks-per-MCU, the ladder's level count) and the per-block tables of the placing and DC kernels (huffman_decode_sync.hip).  The facade
sends only the four layouts above to the device: what is tested here is the public C / Python API.

The reference of every assertion is the coefficients that were coded, or the oracle's bytes (L.huffman_encode_port);
tests/test_mcu_layouts.py holds the oracle to libjpeg on all 63 layouts and shows that the cases are what they claim (dummy blocks, scan
and interval lengths, size classes, where the DC swing sits).  Equality is exact everywhere.  Shapes: 136 x 104 (17 x 13 blocks, odd both
ways), 16 x 16, and one MCU row whose last encoder segment is a single MCU; nothing above 256 x 256.

Encoder, all 63: marker-less on both routes ("sparse" and "dense", real and MCU-padded grids), the restart-interval kernel at ri = 1,
one ri that packs two or more intervals into a wavefront and the largest one, the refusals' text.
Decoder, all 63, default route: photo-like q95 (noise x 2: tests/mcu_layouts.py PHOTO_NOISE), coefficients, route counters moved by
(1, 0, 0, 0), and the first debug line names the level count of M.DEFAULT_LEVELS ("rounds decode" at 10 blocks per MCU).
Decoder, REPRESENTATIVES, routes pinned by the environment switches: stragglers forced (one attempt, "true path resolved", paths handed
over) at 512 and 1024 bits with one lockstep level (hyp_pass01_kernel) and two (hyp_pass0 + hyp_pass1q), the rounds alone, write form
1, the serial kernel, the interval kernel, the parallel restart route, and the largest DC swing across an MCU border per component.
Whole files, REPRESENTATIVES: jpeg_decode, jpeg_encode, jpeg_to_coefficients.  uhdr_hip_jpeg_encode_image (partial edge blocks) stays
with the layouts it has today: the reference helper that defines its padding rules never sees the others, so there is nothing to compare
with.  12 blocks per MCU: refused by the four scan entry points, code and text.

What the library's debug lines said on the MI355X (UHDR_HIP_HUFF_DEBUG; the numbers are a property of the scans):
Default ladder (all 63 decoded by the parallel route):
    blocks per MCU  layouts  first attempt       which attempt held
    3               1        512 bits x 15       the first (4 paths handed to the straggler waves)
    4               6        512 x 11            the first, all six (0 .. 17 handed)
    5               12       512 x 7             the first, all (0 .. 11)
    6               11       512 x 7             the first, all (1 .. 19)
    7               12       512 x 4             the first for eleven; 21-11-22: "3 paths unmerged after 4 levels (2 in lockstep, 16 paths
                                                 handed to the straggler waves), true path LOST (next attempt)", held at 1024 x 4.  The context
                                                 remembers that size for scans of the same blocks-per-MCU and density: the seven layouts
                                                 that run after it start at 1024 bits (and hold there).
    8               12       512 x 4             the first, all (2 .. 28; 22-12-21 with "1 paths unmerged", resolved)
    9               3        512 x 4             the first, all (9 .. 21)
    10              6        rounds, 1024 bits   "settled", all six
Paths handed to the straggler waves by the pinned cases ("true path resolved", one attempt; noise x 2 unless a swap is named):
    layout    blocks  levels  512 bits, 1 lockstep  1024, 1  512, 2      1024, 2
    12-11-11  4       7       50                    4        6           20 (x 4)
    11-21-11  4       7       52                    19       14          8 (x 3)
    21-12-11  5       7       38                    5        5           5
    11-12-12  5       7       79                    21       1           8 (x 4)
    11-11-22  6       7       57                    16       5           4 (x 3)
    22-21-11  7       4       93                    14       10          7 (x 3)
    22-11-12  7       4       75                    9        17          7
    22-21-21  8       4       97                    27       3           6 (x 4)
    21-22-12  8       4       103                   20       28          10 (x 4)
    22-22-11  9       4       151                   24       9           4
    11-22-22  9       4       137                   28       15          8 (x 3)
    22-22-21  10      3       62 (x 1)              48       5 (x 0.6)   2
    22-12-22  10      3       121                   23       7           17 (x 3)
Cases that were swapped (tests/mcu_layouts.py STRAGGLER_NOISE; no layout is dropped, the coefficients are compared as everywhere):
  - 1024 bits with two lockstep levels, nine layouts at noise x 2: nothing is left for the stragglers, e.g. 12-11-11 "merges per level 264 4 0
    0 0 0+, 0 paths unmerged after 7 levels (2 in lockstep, 0 paths handed to the straggler waves), true path resolved" -> the busier x 3, or
    x 4 where x 3 still hands over 0 .. 3.  (x 6 is too busy for 7 .. 10 blocks per MCU: "7 paths unmerged after 4 levels ... true path LOST".)
  - 22-22-21 at 512 bits: "3 paths unmerged after 3 levels (1 in lockstep, 207 paths handed to the straggler waves), true path LOST (next
    attempt)" at x 2, the same with two lockstep levels (30 handed), and lost at x 1.5 (4 unmerged) and x 3 (11) as well: three levels of 512
    bits are a short window -> the calmer x 1 for one lockstep level, x 0.6 for two (x 1 hands over 1 path, x 0.6 5).
All 26 scans of the parallel restart route (8 intervals, photo-like and DC swing) moved the counters by (1, 0, 0, 0).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcu_layouts as M
from libultrahdr_amd import capi as A
from oracle import loader as L

pytestmark = pytest.mark.gpu

ROUTES = ["one_walk", "two_pass"]
OUT_OF_RANGE = "coefficients outside the baseline range (DC difference beyond 11 bits / AC beyond 10 bits)"


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


@pytest.fixture(scope="module")
def routes(hip_ctx):
    """{route: UltraHdr}: the session's context (the default route) and one created with the two-pass switch set (the pattern of
    tests/test_gpu_huffman_encode_one_walk.py)."""
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    assert "UHDR_HIP_HUFF_TWO_PASS" not in os.environ, "the session's context must be on the default route"
    os.environ["UHDR_HIP_HUFF_TWO_PASS"] = "1"
    try:
        ctx2 = Context(0)
    finally:
        del os.environ["UHDR_HIP_HUFF_TWO_PASS"]
    yield {"one_walk": UltraHdr(ctx=hip_ctx), "two_pass": UltraHdr(ctx=ctx2)}
    ctx2.close()


def _encode(u, coefs, w, h, sampling, ri=0):
    import torch

    dev = [torch.from_numpy(np.array(c)).to("cuda:0") for c in coefs]  # (a copy: the cases' arrays are read-only)
    return u.huffman_encode(dev, w, h, sampling, ri).cpu().numpy().tobytes()


def _dev(scan):
    import torch

    return torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to("cuda:0")


def _stats(uhdr):
    st = A.Stats()
    uhdr.lib.uhdr_hip_get_stats(uhdr.ctx.handle, C.byref(st))
    return np.array([st.entropy_decode_parallel, st.entropy_decode_declined, st.entropy_decode_single_lane, st.entropy_decode_intervals])


def _decode(uhdr, coefs, scan, sampling, ri=0, w=M.W, h=M.H, what=""):
    """Decodes the scan; asserts the coefficients; returns the moves of the route counters (parallel, declined, single lane, intervals)."""
    before = _stats(uhdr)
    got = uhdr.huffman_decode(_dev(scan), [c.shape[:2] for c in coefs], w, h, sampling, ri)
    host = [g.cpu().numpy() for g in got]
    moved = tuple(int(v) for v in _stats(uhdr) - before)
    for c in range(len(coefs)):
        bad = np.argwhere((host[c] != coefs[c]).any(axis=-1))
        assert bad.size == 0, (M.layout_id(sampling), what, ri, f"component {c}: {len(bad)} blocks differ, the first at {bad[0].tolist()}", moved)
    return moved


def _attempts(err):
    """The debug lines that name an attempt of the ladder, in order."""
    return [ln for ln in err.splitlines() if "uhdr_hip: hypothesis decode of " in ln or "uhdr_hip: rounds decode of " in ln]


HYP = re.compile(r"subsequences of (\d+) bits x (\d+): .* (\d+) paths unmerged after (\d+) levels \((\d+) in lockstep, (\d+) paths handed to the straggler waves\), true path (\w+)")


# ---- encoder, all 63 layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_marker_less_encoder_equals_the_oracle(routes, sampling):
    shapes = [(M.W, M.H, False), (M.W, M.H, True), (16, 16, False), (*M.last_segment_of_one_mcu(sampling), False)]
    for route in ROUTES:
        for kind in ("sparse", "dense"):
            for w, h, padded in shapes:
                coefs, want = M.random_case(sampling, kind, 0, w, h, padded)
                got = _encode(routes[route], coefs, w, h, sampling)
                assert len(got) == len(want), (route, kind, w, h, padded, len(got), len(want))
                assert got == want, (route, kind, w, h, padded)


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_restart_interval_encoder_equals_the_oracle(uhdr, sampling):
    for ri in M.restart_intervals(sampling):
        for kind in ("sparse", "dense"):
            for w, h, padded in [(M.W, M.H, False), (M.W, M.H, True), (16, 16, False)]:
                coefs, want = M.random_case(sampling, kind, ri, w, h, padded)
                got = _encode(uhdr, coefs, w, h, sampling, ri)
                assert len(got) == len(want), (ri, kind, w, h, padded, len(got), len(want))
                assert got == want, (ri, kind, w, h, padded)


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_an_interval_beyond_one_wavefront_is_refused(uhdr, sampling):
    bpm = M.blocks_per_mcu(sampling)
    top = 64 // bpm
    coefs, _ = M.random_case(sampling, "sparse", 0, 16, 16)
    with pytest.raises(A.UhdrError) as e:
        _encode(uhdr, coefs, 16, 16, sampling, top + 1)
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE
    assert f"restart_interval must be 0 (no markers) or in 1..{top} for {bpm} blocks per MCU" in e.value.detail and f"received {top + 1}" in e.value.detail


def test_coefficients_outside_the_baseline_range_are_refused(routes):
    sampling = [(2, 1), (2, 2), (1, 2)]
    for what in ("ac", "dc"):
        coefs = [c.copy() for c in M.random_case(sampling, "sparse")[0]]
        c = coefs[1]
        if what == "ac":
            c[c.shape[0] // 2, c.shape[1] // 2, 17] = 1024  # 11 bits
        else:
            c[3, 2, 0], c[3, 3, 0] = 1023, -1025            # blocks (1, 0) and (1, 1) of one MCU: a DC difference of 12 bits
        for u, ri in ((routes["one_walk"], 0), (routes["two_pass"], 0), (routes["one_walk"], 4)):
            with pytest.raises(A.UhdrError) as e:
                _encode(u, coefs, M.W, M.H, sampling, ri)
            assert e.value.code == A.UHDR_CODEC_INVALID_PARAM and e.value.detail == OUT_OF_RANGE, (what, ri, e.value.detail)
    coefs, want = M.random_case(sampling, "sparse")  # ... and the contexts code the next scan as before
    for route in ROUTES:
        assert _encode(routes[route], coefs, M.W, M.H, sampling) == want


# ---- decoder, all 63 layouts, the default route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_default_route(uhdr, monkeypatch, capfd, sampling):
    bpm = M.blocks_per_mcu(sampling)
    coefs, scan = M.photo_case(sampling, 95, M.PHOTO_NOISE)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    capfd.readouterr()
    moved = _decode(uhdr, coefs, scan, sampling, what="default route")
    lines = _attempts(capfd.readouterr().err)
    with capfd.disabled():
        print(f"\n{M.layout_id(sampling)} ({bpm} blocks per MCU), {len(scan)} bytes, counters moved by {moved}: " + " | ".join(ln[len("uhdr_hip: "):] for ln in lines))
    assert moved == (1, 0, 0, 0), moved
    assert lines, "no debug line"
    if M.DEFAULT_LEVELS[bpm] == "rounds":
        assert len(lines) == 1 and "rounds decode of" in lines[0] and lines[0].endswith(": settled"), lines
    else:
        m = HYP.search(lines[0])
        assert m, lines[0]
        assert (int(m.group(2)), int(m.group(4))) == (bpm, M.DEFAULT_LEVELS[bpm]), lines[0]


# ---- decoder, the representatives, routes pinned ------------------------------------------------------------------------------------
reps = pytest.mark.parametrize("sampling", M.REPRESENTATIVES, ids=M.REP_IDS)


@reps
@pytest.mark.parametrize("sub_bits", [512, 1024])  # whole subsequences / four pieces with notes at the cuts
@pytest.mark.parametrize("main_levels", [1, 2])    # hyp_pass01_kernel / hyp_pass0_kernel + hyp_pass1q_kernel
def test_stragglers_forced(uhdr, monkeypatch, capfd, sampling, sub_bits, main_levels):
    """The protocol of tests/test_gpu_huffman_straggler.py (decode_with_stragglers), with the level count pinned as well so that
    blocks-per-MCU x (levels + 1) stays within the 48 slots and the pin does not silently fall to the rounds."""
    lid, bpm = M.layout_id(sampling), M.blocks_per_mcu(sampling)
    levels = M.PINNED_LEVELS[bpm]
    noise = M.STRAGGLER_NOISE.get((lid, sub_bits, main_levels), M.PHOTO_NOISE)
    coefs, scan = M.photo_case(sampling, 95, noise)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    monkeypatch.setenv("UHDR_HIP_HUFF_SUB_BITS", str(sub_bits))
    monkeypatch.setenv("UHDR_HIP_HUFF_LEVELS", str(levels))
    monkeypatch.setenv("UHDR_HIP_HUFF_MAIN_LEVELS", str(main_levels))
    capfd.readouterr()
    moved = _decode(uhdr, coefs, scan, sampling, what=f"stragglers {sub_bits} bits, {main_levels} lockstep")
    err = capfd.readouterr().err
    lines = _attempts(err)
    with capfd.disabled():
        print(f"\n{lid} ({bpm} blocks per MCU) noise x {noise}, {len(scan)} bytes: " + " | ".join(ln[len("uhdr_hip: "):] for ln in lines))
    assert moved == (1, 0, 0, 0), moved
    assert len(lines) == 1, lines  # one attempt: the first one held
    m = HYP.search(lines[0])
    assert m, lines[0]
    assert (int(m.group(1)), int(m.group(2)), int(m.group(4)), int(m.group(5))) == (sub_bits, bpm, levels, main_levels), lines[0]
    assert m.group(7) == "resolved", lines[0]
    assert int(m.group(6)) > 0, "no path reached the straggler waves: the case tests nothing"


def _photo(sampling, ri=0):
    return M.photo_case(sampling, 95, M.PHOTO_NOISE, ri)


@reps
def test_the_rounds_alone(uhdr, monkeypatch, capfd, sampling):
    coefs, scan = _photo(sampling)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    monkeypatch.setenv("UHDR_HIP_HUFF_LEVELS", "0")
    capfd.readouterr()
    moved = _decode(uhdr, coefs, scan, sampling, what="rounds")
    lines = _attempts(capfd.readouterr().err)
    assert moved == (1, 0, 0, 0), moved
    assert len(lines) == 1 and "rounds decode of" in lines[0] and lines[0].endswith(": settled"), lines


@reps
def test_write_form_1(uhdr, monkeypatch, capfd, sampling):
    """UHDR_HIP_HUFF_WRITE=1: sync_write_kernel, dc_partial_kernel and dc_apply_kernel in place of the scan-order scratch and coef_place_kernel."""
    coefs, scan = _photo(sampling)
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    monkeypatch.setenv("UHDR_HIP_HUFF_WRITE", "1")
    capfd.readouterr()
    moved = _decode(uhdr, coefs, scan, sampling, what="write form 1")
    err = capfd.readouterr().err
    assert moved == (1, 0, 0, 0), moved
    assert "(write form 1)" in err and "(write form 2)" not in err and "(write form 3)" not in err, err


@reps
def test_serial_kernel(uhdr, monkeypatch, sampling):
    coefs, scan = _photo(sampling)
    monkeypatch.setenv("UHDR_HIP_HUFF_SERIAL", "1")
    assert _decode(uhdr, coefs, scan, sampling, what="serial") == (0, 0, 1, 0)


@reps
def test_interval_kernel(uhdr, monkeypatch, sampling):
    """Short intervals (one MCU each), one lane per interval; and the 8 long intervals through the same kernel."""
    monkeypatch.setenv("UHDR_HIP_HUFF_RST_INTERVALS", "1")
    for ri in (1, M.eight_intervals(M.W, M.H, sampling)):
        coefs, scan = _photo(sampling, ri)
        assert _decode(uhdr, coefs, scan, sampling, ri, what="interval kernel") == (0, 0, 0, 1), ri


@reps
def test_parallel_restart_route(uhdr, capfd, sampling):
    """8 intervals of 320 bytes and more: restart_jump and dc_restart_kernel.  The counters as
    tests/test_gpu_huff_tables.py::test_restart_intervals_long_enough_for_the_parallel_route asserts them."""
    ri = M.eight_intervals(M.W, M.H, sampling)
    for coefs, scan in (_photo(sampling, ri), M.dc_swing_case(sampling, ri)):
        moved = _decode(uhdr, coefs, scan, sampling, ri, what="parallel restart route")
        with capfd.disabled():
            print(f"\n{M.layout_id(sampling)} ri {ri}, {len(scan)} bytes: counters moved by {moved}")
        assert moved[0] + moved[3] == 1 and moved[1] == moved[2] == 0, moved


@reps
def test_largest_dc_swing_across_an_mcu_border(uhdr, routes, monkeypatch, sampling):
    """Per component, -1024 in its last block of one MCU and +1023 in its first block of the next: a prediction taken from the wrong lane
    or the wrong component's sum shows.  Decoder: the default route (coef_place_kernel) and write form 1 (dc_apply_kernel); encoder: both
    marker-less routes and the interval kernel."""
    coefs, scan = M.dc_swing_case(sampling)
    assert _decode(uhdr, coefs, scan, sampling, what="dc swing") == (1, 0, 0, 0)
    monkeypatch.setenv("UHDR_HIP_HUFF_WRITE", "1")
    assert _decode(uhdr, coefs, scan, sampling, what="dc swing, write form 1") == (1, 0, 0, 0)
    monkeypatch.delenv("UHDR_HIP_HUFF_WRITE")
    for route in ROUTES:
        assert _encode(routes[route], coefs, M.W, M.H, sampling) == scan, route
    for ri in M.restart_intervals(sampling):
        assert _encode(uhdr, coefs, M.W, M.H, sampling, ri) == M.dc_swing_case(sampling, ri)[1], ri


# ---- whole files, the representatives -------------------------------------------------------------------------------------------
@reps
@pytest.mark.parametrize("ri", [0, 3])
def test_file_decode(uhdr, sampling, ri):
    """uhdr.jpeg_decode: planes of the real grids, equal to the oracle's IDCT of the coded coefficients; uhdr.jpeg_to_coefficients."""
    coefs, scan = _photo(sampling, ri)
    (ql, qc), jpeg = M.assemble(coefs, M.W, M.H, sampling, ri, scan)
    got = uhdr.jpeg_decode(jpeg)
    assert len(got) == 3
    for c, (bh, bw) in enumerate(M.real_grids(M.W, M.H, sampling)):
        want = L.idct_dequant_port(coefs[c], ql if c == 0 else qc)
        assert got[c].shape == want.shape == (bh * 8, bw * 8), c
        assert np.array_equal(got[c], want), (c, int((got[c] != want).sum()))
    hdr, dev = uhdr.jpeg_to_coefficients(jpeg)
    assert [(hdr.scan.h_samp[c], hdr.scan.v_samp[c]) for c in range(3)] == sampling and hdr.scan.restart_interval == ri
    for c in range(3):
        assert np.array_equal(dev[c].cpu().numpy(), coefs[c]), c


def _planes(sampling):
    rng = np.random.default_rng(500 + int(M.layout_id(sampling).replace("-", "")))
    out = []
    for c, (bh, bw) in enumerate(M.real_grids(M.W, M.H, sampling)):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
        base = 128 + 90 * np.sin(xx / (37.0 - 5 * c)) * np.cos(yy / 23.0) + rng.normal(0, 6, (bh * 8, bw * 8))
        out.append(np.clip(base, 0, 255).astype(np.uint8))
    return out


def _encoded_file(uhdr, sampling):
    planes = _planes(sampling)
    ql, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
    jpeg = uhdr.jpeg_encode(planes, M.W, M.H, sampling, ql, qc)
    want = [L.fdct_quant_port(p, p.shape[1], p.shape[1] // 8, p.shape[0] // 8, ql if c == 0 else qc) for c, p in enumerate(planes)]
    return jpeg, want, (ql, qc)


@reps
def test_file_encode(uhdr, sampling):
    """uhdr.jpeg_encode on block-padded planes: the file's coefficients (the oracle's entropy decoder) are the oracle's FDCT of the planes,
    and the device decodes its own file to the oracle's IDCT of them."""
    jpeg, want, (ql, qc) = _encoded_file(uhdr, sampling)
    hdr = uhdr.jpeg_parse(jpeg)
    ri = 64 // M.blocks_per_mcu(sampling)
    assert hdr.scan.restart_interval == ri and [(hdr.scan.h_samp[c], hdr.scan.v_samp[c]) for c in range(3)] == sampling
    shapes = [(hdr.scan.blocks_h[c], hdr.scan.blocks_w[c]) for c in range(3)]
    assert shapes == M.real_grids(M.W, M.H, sampling)
    rc, got = L.huffman_decode_port(shapes, M.W, M.H, sampling, ri, jpeg[hdr.scan_offset: hdr.scan_offset + hdr.scan_bytes])
    assert rc == 0
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c
    back = uhdr.jpeg_decode(jpeg)
    for c in range(3):
        assert np.array_equal(back[c], L.idct_dequant_port(want[c], ql if c == 0 else qc)), c


@reps
def test_libjpeg_reads_the_encoded_file(uhdr, ref, sampling):
    from test_oracle_vs_ref import _read_coefficients

    jpeg, want, (ql, qc) = _encoded_file(uhdr, sampling)
    got, qt = _read_coefficients(ref, jpeg)
    assert len(got) == 3 and np.array_equal(qt[0], ql) and np.array_equal(qt[1], qc) and np.array_equal(qt[2], qc)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c


# ---- more than 10 blocks per MCU ----------------------------------------------------------------------------------------------------
def _refused(e):
    assert e.value.code == A.UHDR_CODEC_INVALID_PARAM, e.value
    assert e.value.detail == "an MCU holds at most 10 blocks (T.81 B.2.3), received 12", e.value.detail


def test_12_blocks_per_mcu_are_refused_by_the_scan_entry_points(uhdr):
    w = h = 16
    coefs = M.random_coefs(np.random.default_rng(12), M.real_grids(w, h, M.ILLEGAL), "sparse")
    scan = L.huffman_encode_port(coefs, w, h, M.ILLEGAL, 0)  # (the oracle codes it: no decoder takes it)
    before = _stats(uhdr)
    for ri in (0, 1):
        with pytest.raises(A.UhdrError) as e:  # uhdr_hip_huffman_encode_dev
            _encode(uhdr, coefs, w, h, M.ILLEGAL, ri)
        _refused(e)
    with pytest.raises(A.UhdrError) as e:  # uhdr_hip_huffman_decode_dev
        uhdr.huffman_decode(_dev(scan), [c.shape[:2] for c in coefs], w, h, M.ILLEGAL, 0)
    _refused(e)
    planes = [np.full((16, 16), 100 + c, np.uint8) for c in range(3)]
    ql, qc = L.quant_table_port(95, False), L.quant_table_port(95, True)
    with pytest.raises(A.UhdrError) as e:  # uhdr_hip_jpeg_encode_scan
        uhdr.jpeg_encode(planes, w, h, M.ILLEGAL, ql, qc)
    _refused(e)
    # uhdr_hip_jpeg_decode_scan: the parser refuses the file, so the header is that of the 10-block layout next to it with the last
    # component's factors raised
    legal = [(2, 2), (2, 2), (2, 1)]
    lc, ls = M.random_case(legal, "sparse", 0, w, h)
    _, jpeg = M.assemble(lc, w, h, legal, 0, ls)
    hdr = uhdr.jpeg_parse(jpeg)
    hdr.scan.h_samp[2], hdr.scan.v_samp[2], hdr.scan.blocks_h[2] = 2, 2, 2
    buf = np.frombuffer(jpeg, dtype=np.uint8)
    outs = [np.zeros((16, 16), np.uint8) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
    with pytest.raises(A.UhdrError) as e:
        uhdr._call(False, uhdr.lib.uhdr_hip_jpeg_decode_scan, uhdr.ctx.handle, C.byref(hdr), C.c_void_p(buf.ctypes.data + hdr.scan_offset),
                   buf.size - hdr.scan_offset, 0, 0, ptrs, (C.c_uint * 3)(16, 16, 16), (C.c_uint * 3)(16, 16, 16))
    _refused(e)
    assert all(not o.any() for o in outs) and tuple(_stats(uhdr) - before) == (0, 0, 0, 0)
    got = uhdr.jpeg_decode(jpeg)  # ... and the context decodes the legal file as before
    (ql, qc), _ = M.assemble(lc, w, h, legal, 0, ls)
    for c in range(3):
        assert np.array_equal(got[c], L.idct_dequant_port(lc[c], ql if c == 0 else qc)), c
