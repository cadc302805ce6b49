"""CPU: the 63 MCU layouts of tests/mcu_layouts.py against the oracle's own decoder and libjpeg, the parser on files of every layout,
the refusal of 12 blocks per MCU, and the cases of tests/test_gpu_mcu_layouts.py being what they claim to be.  Equality is exact.

This widens the pin of the oracle's Huffman restatements to libjpeg (tests/test_oracle_vs_ref.py:
test_huffman_restatements_randomised_against_libjpeg, 5 layouts) to every layout libjpeg takes."""
import ctypes as C

import numpy as np
import pytest

import mcu_layouts as M
from libultrahdr_amd import capi as A
from oracle import loader as L

RIS = [0, 1, 3]


def _cases(sampling):
    for (w, h) in M.SIZES:
        for ri in RIS:
            yield w, h, ri, M.random_case(sampling, "sparse", ri, w, h)


def _read_coefficients(ref, jpeg):
    from test_oracle_vs_ref import _read_coefficients as read

    return read(ref, jpeg)


def _parse(jpeg):
    hdr = A.JpegHeader()
    buf = np.frombuffer(jpeg, dtype=np.uint8)
    return A.load().uhdr_hip_jpeg_parse(buf.ctypes.data, buf.size, C.byref(hdr)), hdr


def _illegal_file():
    w, h = 16, 16
    rng = np.random.default_rng(12)
    coefs = M.random_coefs(rng, M.real_grids(w, h, M.ILLEGAL), "sparse")
    scan = L.huffman_encode_port(coefs, w, h, M.ILLEGAL, 0)
    return coefs, scan, M.assemble(coefs, w, h, M.ILLEGAL, 0, scan)[1]


def test_the_layouts_are_the_63_legal_ones():
    assert len(M.LAYOUTS) == 63 and len(set(M.IDS)) == 63 and M.ILLEGAL not in M.LAYOUTS
    assert all(hs in (1, 2) and vs in (1, 2) for s in M.LAYOUTS for hs, vs in s)
    hist = {}
    for s in M.LAYOUTS:
        hist[M.blocks_per_mcu(s)] = hist.get(M.blocks_per_mcu(s), 0) + 1
    assert hist == {3: 1, 4: 6, 5: 12, 6: 11, 7: 12, 8: 12, 9: 3, 10: 6}
    assert M.blocks_per_mcu(M.ILLEGAL) == 12
    assert M.layout_id([(2, 1), (1, 2), (1, 1)]) == "21-12-11"
    assert sorted(M.DEFAULT_LEVELS) == sorted(M.PINNED_LEVELS) == sorted(hist)


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_the_oracle_decodes_its_own_scan(sampling):
    for w, h, ri, (coefs, scan) in _cases(sampling):
        rc, back = L.huffman_decode_port([c.shape[:2] for c in coefs], w, h, sampling, ri, scan)
        assert rc == 0 and all(np.array_equal(b, c) for b, c in zip(back, coefs)), (w, h, ri)


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_libjpeg_reads_the_oracles_file(ref, sampling):
    for w, h, ri, (coefs, scan) in _cases(sampling):
        _, jpeg = M.assemble(coefs, w, h, sampling, ri, scan)
        back, _ = _read_coefficients(ref, jpeg)
        assert len(back) == 3 and all(np.array_equal(b, c) for b, c in zip(back, coefs)), (w, h, ri)


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_the_parser_reads_the_file(sampling):
    """uhdr_hip_jpeg_parse gives back the layout, the real grids, the restart interval and the scan bytes."""
    for w, h, ri, (coefs, scan) in _cases(sampling):
        _, jpeg = M.assemble(coefs, w, h, sampling, ri, scan)
        rc, hdr = _parse(jpeg)
        assert rc == 0, (w, h, ri, rc)
        sc = hdr.scan
        assert (sc.num_components, sc.w, sc.h, sc.restart_interval) == (3, w, h, ri)
        assert [(sc.h_samp[c], sc.v_samp[c]) for c in range(3)] == sampling
        assert [(sc.blocks_h[c], sc.blocks_w[c]) for c in range(3)] == M.real_grids(w, h, sampling) == [c.shape[:2] for c in coefs]
        assert jpeg[hdr.scan_offset: hdr.scan_offset + hdr.scan_bytes] == scan


def test_the_parser_refuses_12_blocks_per_mcu():
    """All three components at 2x2: T.81 B.2.3 allows 10 blocks per MCU.  The oracle codes and decodes such a scan all the same, which
    is what makes the file; the parser answers -7 with the other SOF refusals."""
    coefs, scan, jpeg = _illegal_file()
    rc, back = L.huffman_decode_port([c.shape[:2] for c in coefs], 16, 16, M.ILLEGAL, 0, scan)
    assert rc == 0 and all(np.array_equal(b, c) for b, c in zip(back, coefs))
    assert _parse(jpeg)[0] == -7
    legal = bytearray(jpeg)  # the same file with the last component at 2x1 parses (the refusal is the MCU size, nothing else in the file)
    sof = jpeg.find(b"\xff\xc0")
    assert legal[sof + 11 + 6] == 0x22
    legal[sof + 11 + 6] = 0x21
    assert _parse(bytes(legal))[0] == 0


def test_libjpeg_refuses_12_blocks_per_mcu(ref):
    _, _, jpeg = _illegal_file()
    qt = np.zeros((3, 64), dtype=np.uint16)
    bw, bh, nc = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    none = (C.c_void_p * 3)(None, None, None)
    buf = np.frombuffer(jpeg, dtype=np.uint8)
    assert ref.ref_jpeg_read_coefficients(buf.ctypes.data, buf.size, none, qt.ctypes.data, bw, bh, C.byref(nc)) != 0
    assert _parse(jpeg)[0] == -7


# ---- the cases are what they claim ------------------------------------------------------------------------------------------------
def test_representatives_hold_what_the_pinned_tests_need():
    reps = M.REPRESENTATIVES
    assert all(s in M.LAYOUTS for s in reps) and len({M.layout_id(s) for s in reps}) == len(reps)
    assert {M.blocks_per_mcu(s) for s in reps} >= set(range(4, 11))
    assert [(1, 2), (1, 1), (1, 1)] in reps                                                         # 4:4:0
    area = lambda f: f[0] * f[1]
    assert any(area(s[1]) > area(s[0]) or area(s[2]) > area(s[0]) for s in reps)                    # chroma finer than luma
    def from_different_components(s):
        hmax, vmax = max(f[0] for f in s), max(f[1] for f in s)
        return not any(f == (hmax, vmax) for f in s)
    assert any(from_different_components(s) for s in reps)                                          # hmax and vmax
    assert any(area(s[1]) > area(s[2]) for s in reps) and any(area(s[2]) > area(s[1]) for s in reps)  # Cb / Cr differ, both orders
    assert any(s[2] == (2, 2) for s in reps)
    assert any(s[0][1] > s[0][0] for s in reps)                                                     # vs > hs: jj / hs with hs = 1, vs = 2


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_dummy_blocks_at_the_main_shape(sampling):
    col, row = M.has_dummy_blocks(M.W, M.H, sampling)
    if sampling == [(1, 1)] * 3:
        assert not col and not row
    else:
        assert col or row
        hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
        assert col == (hmax == 2) and row == (vmax == 2)  # 17 x 13 blocks: odd both ways, a dummy column / row wherever a factor is 2
    real, pad = M.real_grids(M.W, M.H, sampling), M.padded_grids(M.W, M.H, sampling)
    assert all(r[0] <= p[0] and r[1] <= p[1] for r, p in zip(real, pad))


def test_every_layout_with_a_2_has_a_dummy_column_or_row_and_most_have_both():
    both = sum(1 for s in M.LAYOUTS if all(M.has_dummy_blocks(M.W, M.H, s)))
    some = sum(1 for s in M.LAYOUTS if any(M.has_dummy_blocks(M.W, M.H, s)))
    assert some == 62 and both == 62 - 2 * 7  # hmax == 1 or vmax == 1: 8 layouts each, 4:4:4 among both


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_decode_cases_reach_the_parallel_decoder(sampling):
    """The marker-less scans of the GPU decode tests hold the 4096 bytes the parallel decoder asks for, the 8-interval scans average the
    320 bytes per interval its restart route asks for, and the short-interval scans (ri = 1) stay below that."""
    for coefs, scan in (M.photo_case(sampling, 95, M.PHOTO_NOISE), M.dc_swing_case(sampling)):
        assert len(scan) >= 4096, len(scan)
    ri = M.eight_intervals(M.W, M.H, sampling)
    mpr, mrows = M.mcu_grid(M.W, M.H, sampling)
    assert -(-mpr * mrows // ri) == 8
    for scan in (M.photo_case(sampling, 95, M.PHOTO_NOISE, ri=ri)[1], M.dc_swing_case(sampling, ri)[1]):
        assert len(scan) >= 4096 and len(scan) // 8 >= 320, len(scan)
        assert len(re_split_markers(scan)) == 8
    short = M.photo_case(sampling, 95, M.PHOTO_NOISE, ri=1)[1]
    assert len(short) // (mpr * mrows) < 320


def re_split_markers(scan):
    import re

    return re.split(rb"\xff[\xd0-\xd7]", scan)


@pytest.mark.parametrize("sampling", M.REPRESENTATIVES, ids=M.REP_IDS)
def test_pinned_cases_reach_the_parallel_decoder(sampling):
    for key, noise in M.STRAGGLER_NOISE.items():
        if key[0] == M.layout_id(sampling):
            assert len(M.photo_case(sampling, 95, noise)[1]) >= 4096, key


@pytest.mark.parametrize("sampling", M.REPRESENTATIVES, ids=M.REP_IDS)
def test_the_dc_swing_is_where_it_is_meant_to_be(sampling):
    coefs, scan = M.dc_swing_case(sampling)
    rc, back = L.huffman_decode_port([c.shape[:2] for c in coefs], M.W, M.H, sampling, 0, scan)
    assert rc == 0 and all(np.array_equal(b, c) for b, c in zip(back, coefs))
    mpr, _ = M.mcu_grid(M.W, M.H, sampling)
    for c, lo, hi in M.swing_blocks(sampling):
        hs, vs = sampling[c]
        assert coefs[c][lo][0] == -1024 and coefs[c][hi][0] == 1023
        # hi is block (0, 0) of the component in its MCU, lo the component's last block in the MCU in front of it, same MCU row
        assert hi[0] % vs == 0 and hi[1] % hs == 0 and lo[0] % vs == vs - 1 and lo[1] % hs == hs - 1
        assert lo[0] // vs == hi[0] // vs and lo[1] // hs + 1 == hi[1] // hs < mpr


@pytest.mark.parametrize("sampling", M.LAYOUTS, ids=M.IDS)
def test_encoder_cases(sampling):
    """"dense" scans at the main shape hold a segment above the encoder's small size class, "sparse" ones none; the last-segment shape ends
    in a segment of one MCU; 16 x 16 is one segment; the three restart intervals are 1, one that packs two or more intervals into a
    wavefront, and the largest the encoder takes."""
    bpm, seg = M.blocks_per_mcu(sampling), M.segment_mcus(sampling)
    for padded in (False, True):
        dense = M.segment_bits(M.random_case(sampling, "dense", padded=padded)[0], M.W, M.H, sampling)
        sparse = M.segment_bits(M.random_case(sampling, "sparse", padded=padded)[0], M.W, M.H, sampling)
        mpr, mrows = M.mcu_grid(M.W, M.H, sampling)
        assert len(dense) == len(sparse) == -(-mpr * mrows // seg) > 1
        assert max(dense) > M.SMALL_MAX_BITS + 64 and max(sparse) < M.SMALL_MAX_BITS - 64, (max(dense), max(sparse))
    w, h = M.last_segment_of_one_mcu(sampling)
    mpr, mrows = M.mcu_grid(w, h, sampling)
    assert w <= 256 and h <= 256 and (mpr * mrows) % seg == 1 and mpr * mrows > 1
    mpr, mrows = M.mcu_grid(16, 16, sampling)
    assert mpr * mrows <= seg
    lo, mid, top = M.restart_intervals(sampling)
    assert lo == 1 < mid < top == 64 // bpm and 2 * mid * bpm <= 64 < (top + 1) * bpm
    assert bpm * (M.PINNED_LEVELS[bpm] + 1) <= 48
