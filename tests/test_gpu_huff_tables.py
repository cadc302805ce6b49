"""GPU: the device forms of a file's Huffman tables (csrc/api_entropy.cpp: make_dec_table, make_fast_table, make_track_table,
make_value_table, make_pair_table, make_pair_value_table and the packed sub-table array) on tables other than Annex K, through every
kernel that reads them: the self-synchronising decoder with its straggler waves, the serial kernel, the interval kernel, the restart
route of the parallel decoder, and the file entry points behind csrc/jpeg_parse.cpp.

The table families, the encoder that takes them and the 256 x 256 cases are tests/huff_tables.py; tests/test_huff_tables.py shows that
the oracle's decoder and libjpeg read the coded coefficients from the same bytes, so the reference of every assertion here is the
coefficients that were coded.  Equality is exact.  Apart from the env-pinned straggler group no assertion depends on which attempt of
the ladder succeeded: only the route counters (uhdr_hip_get_stats) and the coefficients count.

Routes of the default ladder, as measured (counters of uhdr_hip_get_stats; scan bytes in brackets).  inverted and flat may take either
route; both took the parallel one on every sampling -- the reversed Annex K tables do fall in step within what the ladder gives their
density, and the flat eight-bit code, which has no short code to fall in step on, does too:
    family    4:4:4 q95          4:2:0 q100         4:2:2 q95          one comp q100
    inverted  parallel (155587)  parallel (169300)  parallel (113864)  parallel (114106)
    flat      parallel (61622)   parallel (65705)   parallel (45054)   parallel (44199)
On a fresh context each of these held at the ladder's first attempt: inverted (405 .. 891 bits per block) at 4096 bits with 0 paths unmerged
(0 .. 39 handed to the stragglers), flat at 512 bits (q95: 160 / 175 bits per block, 285 / 244 handed) and at 2048 bits (q100: 72 / 5 handed).
annexk, deep16, dc_long, short_first and shallow: parallel on every sampling; deep33 and deep17: one lane on every sampling.

Paths handed to the straggler waves (one lockstep level, "true path resolved", one attempt), 512 bits / 1024 bits:
    family       4:2:0                         4:4:4
    inverted     q95, noise x 0.5: 2381 / 701  q95, noise x 0.5: 1968 / 550
    deep16       q95:  816 / 162               q95:  714 /  87
    dc_long      q95:  791 / 211               q95:  592 /  90
    short_first  q100: 666 /  96               q100: 690 / 135
Cases that were swapped out, with what the library's debug line said of them (none of a family is dropped, inverted at 512 bits included):
  - 4:2:0 q100 for inverted, deep16 and dc_long: the first attempt is lost at both sizes ("602 / 341", "36 / 18" and "14 / 12 paths unmerged
    after 7 / 4 levels ... true path LOST (next attempt)"; the decode is then repeated and right) -> the calmer 4:2:0 q95.
  - inverted at the cases' full noise, 4:2:0 q95 and 4:4:4 q95: "93 / 34" and "51 / 30 paths unmerged ... true path LOST" (a symbol
    of 16 bits and more leaves 512 x 7 or 1024 x 4 bits too few symbols to fall in step on) -> the same image with half the noise.
  - short_first 4:4:4 q95 at 1024 bits: "0 paths handed to the straggler waves" (one-bit codes fall in step within the first level)
    -> the busier 4:4:4 q100, used for both sizes.
"""
import ctypes as C

import numpy as np
import pytest

import huff_tables as T
from libultrahdr_amd import capi as A
from oracle import loader as L
from test_gpu_huffman_straggler import decode_with_stragglers

pytestmark = pytest.mark.gpu

NAMES = list(T.FAMILIES)
QUALITY = {"444": 95, "420": 100, "422": 95, "400": 100}  # as tests/test_huff_tables.py
PARALLEL = ("annexk", "deep16", "dc_long", "short_first", "shallow")  # must take the parallel route
HANDED_OVER = ("deep33", "deep17")  # more sub-tables than the packed array / one table holds: one lane
EITHER = ("inverted", "flat")


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def _dev(scan):
    import torch

    return torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to("cuda:0")


def _stats(uhdr):
    st = A.Stats()
    uhdr.lib.uhdr_hip_get_stats(uhdr.ctx.handle, C.byref(st))
    return np.array([st.entropy_decode_parallel, st.entropy_decode_declined, st.entropy_decode_single_lane, st.entropy_decode_intervals])


def _decode(uhdr, name, sampling, quality, ri=0):
    """Decodes the family's scan of the case; asserts the coefficients; returns the moves of the four route counters (parallel,
    declined, single lane, intervals) and the scan's length."""
    coefs, scan, tables = T.coded(name, sampling, quality, ri)
    before = _stats(uhdr)
    got = uhdr.huffman_decode(_dev(scan), [c.shape[:2] for c in coefs], T.W, T.H, T.SAMPLINGS[sampling], ri, tables=tables)
    host = [g.cpu().numpy() for g in got]
    moved = tuple(int(v) for v in _stats(uhdr) - before)
    for c in range(len(coefs)):
        assert np.array_equal(host[c], coefs[c]), (name, sampling, quality, ri, c, moved)
    return moved, len(scan)


# ---- a. the default route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", list(T.SAMPLINGS))
@pytest.mark.parametrize("name", NAMES)
def test_default_route(uhdr, capfd, name, sampling):
    moved, nbytes = _decode(uhdr, name, sampling, QUALITY[sampling])
    with capfd.disabled():
        print(f"\n{name} {sampling} q{QUALITY[sampling]}, {nbytes} bytes: parallel / declined / single lane / intervals moved by {moved}")
    if name in PARALLEL:
        assert moved == (1, 0, 0, 0), (name, sampling, moved)
    elif name in HANDED_OVER:
        assert moved == (0, 0, 1, 0), (name, sampling, moved)
    else:
        assert moved in ((1, 0, 0, 0), (0, 0, 1, 0)), (name, sampling, moved)


def test_inverted_takes_the_parallel_route_somewhere(uhdr):
    """A family that never took the parallel route would test the one-lane kernel four times over."""
    took = [s for s in T.SAMPLINGS if _decode(uhdr, "inverted", s, QUALITY[s])[0] == (1, 0, 0, 0)]
    assert took, "inverted scans: no sampling decoded by the parallel route"


# ---- b. stragglers forced -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub_bits", [512, 1024])
@pytest.mark.parametrize("name,sampling,quality,noise", T.STRAGGLER_CASES)
def test_straggler_walk_on_other_tables(uhdr, monkeypatch, capfd, name, sampling, quality, noise, sub_bits):
    """One lockstep level, the subsequence size pinned: exactly one attempt, "true path resolved", a non-zero number of paths handed
    to the straggler waves (the protocol of tests/test_gpu_huffman_straggler.py), and the coefficients that were coded."""
    coefs, scan, tables = T.coded(name, sampling, quality, 0, noise)
    decode_with_stragglers(uhdr, monkeypatch, capfd, sampling, quality, sub_bits, 1, tables=tables, coded=(coefs, scan))


# ---- c. the kernels that read make_dec_table's form -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_serial_kernel(uhdr, monkeypatch, name):
    monkeypatch.setenv("UHDR_HIP_HUFF_SERIAL", "1")
    moved, _ = _decode(uhdr, name, "420", 100)
    assert moved == (0, 0, 1, 0), (name, moved)


@pytest.mark.parametrize("name", NAMES)
def test_interval_kernel(uhdr, monkeypatch, name):
    """restart_interval 4: 64 intervals, one lane each.  Every family's intervals of this case average 320 bytes or more (Annex K: 552),
    which the library sends to the parallel decoder first; UHDR_HIP_HUFF_RST_INTERVALS pins the interval kernel, as in
    tests/test_gpu_huffman_sync.py.  Without the pin, either route -- one of them, and the same coefficients."""
    monkeypatch.setenv("UHDR_HIP_HUFF_RST_INTERVALS", "1")
    moved, nbytes = _decode(uhdr, name, "420", 100, ri=4)
    assert moved == (0, 0, 0, 1), (name, moved)
    monkeypatch.delenv("UHDR_HIP_HUFF_RST_INTERVALS")
    assert nbytes // 64 >= 320
    moved, _ = _decode(uhdr, name, "420", 100, ri=4)
    assert moved in ((1, 0, 0, 0), (0, 0, 0, 1)), (name, moved)


@pytest.mark.parametrize("name", ["inverted", "dc_long"])
def test_restart_intervals_long_enough_for_the_parallel_route(uhdr, name):
    ri = 16  # 256 MCUs: 16 intervals
    scan = T.coded(name, "420", 100, ri)[1]
    assert len(scan) >= 4096 and len(scan) // 16 >= 320, len(scan)
    moved, _ = _decode(uhdr, name, "420", 100, ri=ri)
    assert moved[0] + moved[3] == 1 and moved[1] == moved[2] == 0, (name, moved)


# ---- d. files -------------------------------------------------------------------------------------------------------------------
def _file(name, layout, ri=0):
    coefs, scan, tables = T.coded(name, "420", 100, ri)
    ql, qc = L.quant_table_port(100, False), L.quant_table_port(100, True)
    return coefs, (ql, qc), T.assemble_file(coefs, T.W, T.H, T.SAMPLINGS["420"], ri, ql, qc, scan, tables, layout)


@pytest.mark.parametrize("layout", ["one-per-segment", "all-in-one", "redefined"])
def test_files_with_the_dht_segments_laid_out_otherwise(uhdr, layout):
    coefs, _, jpeg = _file("dc_long", layout)
    hdr, dev = uhdr.jpeg_to_coefficients(jpeg)
    bits, vals = T.family("dc_long")
    assert np.array_equal(np.frombuffer(hdr.tables.bits, dtype=np.uint8).reshape(4, 17), bits)
    assert np.array_equal(np.frombuffer(hdr.tables.vals, dtype=np.uint8).reshape(4, 256), vals)
    for c in range(3):
        assert np.array_equal(dev[c].cpu().numpy(), coefs[c]), (layout, c)


def test_file_whose_tables_do_not_fit_the_packed_array(uhdr):
    """deep33 through the one-call file decode: the planes of the oracle's IDCT of the coded coefficients, or the documented decline
    (UHDR_CODEC_UNSUPPORTED_FEATURE, entropy_decode_declined + 1) that test_files_with_optimised_huffman_tables accepts."""
    coefs, (ql, qc), jpeg = _file("deep33", "one-per-segment")
    before = _stats(uhdr)
    try:
        planes = uhdr.jpeg_decode(jpeg)
    except A.UhdrError as err:
        assert err.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE, err
        assert tuple(_stats(uhdr) - before) == (0, 1, 0, 0)
        return
    assert (_stats(uhdr) - before)[0] == 0
    for c in range(3):
        assert np.array_equal(planes[c], L.idct_dequant_port(coefs[c], qc if c else ql)), c


# ---- e. the table cache ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dc_long", "short_first"])
def test_table_cache_is_keyed_by_the_table_bytes(uhdr, name):
    """The same scan bytes with the tables they were coded with, then with Annex K (garbage, or the one error a corrupt scan gives), then
    with the right tables again: the third decode equals the first -- the context's device tables are rebuilt whenever the DHT bytes change."""
    coefs, scan, tables = T.coded(name, "420", 100)
    shapes, samp = [c.shape[:2] for c in coefs], T.SAMPLINGS["420"]
    first = [g.cpu().numpy() for g in uhdr.huffman_decode(_dev(scan), shapes, T.W, T.H, samp, 0, tables=tables)]
    for c in range(3):
        assert np.array_equal(first[c], coefs[c]), c
    try:
        wrong = [g.cpu().numpy() for g in uhdr.huffman_decode(_dev(scan), shapes, T.W, T.H, samp, 0, tables=T.family("annexk"))]
        assert not all(np.array_equal(wrong[c], coefs[c]) for c in range(3))
    except A.UhdrError as err:
        assert err.code == A.UHDR_CODEC_INVALID_PARAM, err
    third = [g.cpu().numpy() for g in uhdr.huffman_decode(_dev(scan), shapes, T.W, T.H, samp, 0, tables=tables)]
    for c in range(3):
        assert np.array_equal(third[c], first[c]), c
