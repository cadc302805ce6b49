"""CPU: the table families and the table-taking encoder of tests/huff_tables.py, held to the oracle's encoder and decoder and to
libjpeg itself -- what tests/test_gpu_huff_tables.py compares the device decoder with is the coefficients that were coded, and here is
why that is the same as the oracle's and libjpeg's reading of the same bytes."""
import ctypes as C

import numpy as np
import pytest

import huff_tables as T
from oracle import loader as L

NAMES = list(T.FAMILIES)
QUALITY = {"444": 95, "420": 100, "422": 95, "400": 100}  # the case each sampling is checked on (the other quality: the length test below)


@pytest.mark.parametrize("name", NAMES)
def test_every_family_is_four_valid_dht_tables(name):
    for sampling, quality in QUALITY.items():
        bits, vals = T.family(name, sampling, quality)
        for t in range(4):
            n = T.check_dht(bits[t], vals[t], t % 2 == 0)
            if name == "shallow":
                assert (t % 2 == 0 and n == 12) or n < 162
            else:
                want = T.DC_SYMBOLS if t % 2 == 0 else T.AC_SYMBOLS
                assert sorted(vals[t, :n].tolist()) == sorted(want), (name, t)
        counts = tuple(T.long_prefixes(bits[t]) for t in range(4))
        if name in T.PREFIXES:
            assert counts == T.PREFIXES[name], (name, counts)
        if name in ("shallow", "flat"):
            assert counts == (0, 0, 0, 0)
            assert int(np.flatnonzero(bits[1])[-1]) <= 9 and int(np.flatnonzero(bits[3])[-1]) <= 9
    assert sum(T.PREFIXES["deep16"]) == 32 and sum(T.PREFIXES["deep33"]) == 33 and T.PREFIXES["deep17"][1] == 17
    assert len(set(T.PREFIXES["dc_long"])) == 4 and min(T.PREFIXES["dc_long"]) > 0


def test_the_families_put_the_codes_where_they_say():
    code, length = T.codes_of(*[a[1] for a in T.family("inverted")])
    assert all(length[s] == 16 for s in (T.EOB, 0x01, 0x11, 0x02, T.ZRL, 0x0A))
    _, dlen = T.codes_of(*[a[0] for a in T.family("inverted")])
    assert sorted(dlen[:4].tolist()) == [15, 15, 16, 16]
    for t in (1, 3):
        code, length = T.codes_of(*[a[t] for a in T.family("short_first")])
        assert (length[T.EOB], length[0x01], length[0x11]) == (1, 2, 3) and code[T.EOB] == 0
        _, length = T.codes_of(*[a[t] for a in T.family("flat")])
        assert set(length[T.AC_SYMBOLS].tolist()) == {8}
        _, length = T.codes_of(*[a[t] for a in T.family("deep16")])
        assert length[T.EOB] <= 9 < length[0x01] and length[0x11] <= 9 < length[0x02]  # both levels in every block
    _, dlen = T.codes_of(*[a[0] for a in T.family("short_first")])
    assert dlen[0] == 1
    _, dlen = T.codes_of(*[a[0] for a in T.family("dc_long")])
    assert dlen[11] == 16  # 16 + 11 bits in one step


def test_the_cases_hold_what_the_families_are_for():
    for sampling, quality in QUALITY.items():
        tk = T._tokens(sampling, quality, 0)
        dc, ac = tk["tab"] % 2 == 0, tk["tab"] % 2 == 1
        assert (tk["sym"][dc] == 11).any() and (tk["sym"][dc] == 0).any(), "DC categories 0 and 11"
        assert ((tk["sym"][ac] & 15) == 10).any(), "AC size 10"
        assert (tk["sym"][ac] == T.ZRL).any() and (tk["sym"][ac] == T.EOB).any()
        if quality == 100:
            assert any((c[..., 63] != 0).any() for c in T.case(sampling, quality)), "no block is coded up to its last term"


@pytest.mark.parametrize("ri", [0, 7])
@pytest.mark.parametrize("sampling", list(T.SAMPLINGS))
def test_annexk_bytes_equal_the_oracles_encoder(sampling, ri):
    for quality in (95, 100):
        coefs = T.case(sampling, quality)
        assert T.encode_scan(coefs, T.W, T.H, T.SAMPLINGS[sampling], ri, T.family("annexk")) == L.huffman_encode_port(coefs, T.W, T.H, T.SAMPLINGS[sampling], ri)


@pytest.mark.parametrize("w,h,sampling,ri", [(100, 60, "420", 0), (57, 33, "422", 3), (41, 23, "444", 0), (19, 50, "400", 5)])
def test_annexk_bytes_equal_the_oracles_encoder_with_dummy_blocks(w, h, sampling, ri):
    """Sizes that are no multiple of the MCU: dummy blocks at the right and bottom edges."""
    rng = np.random.default_rng(w * h)
    samp = T.SAMPLINGS[sampling]
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    coefs = []
    for hs, vs in samp:
        bw, bh = (-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8
        a = (rng.integers(-200, 201, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.2)).astype(np.int16)
        a[..., 0] = rng.integers(-1000, 1001, (bh, bw))
        coefs.append(a)
    assert T.encode_scan(coefs, w, h, samp, ri, T.family("annexk")) == L.huffman_encode_port(coefs, w, h, samp, ri)


@pytest.mark.parametrize("sampling", list(T.SAMPLINGS))
@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_decodes_what_was_coded(name, sampling):
    quality = QUALITY[sampling]
    for ri in (0, 5):
        coefs, scan, tables = T.coded(name, sampling, quality, ri)
        rc, got = L.huffman_decode_port([c.shape[:2] for c in coefs], T.W, T.H, T.SAMPLINGS[sampling], ri, scan, tables=tables)
        assert rc == 0, (name, sampling, ri)
        for c in range(len(coefs)):
            assert np.array_equal(got[c], coefs[c]), (name, sampling, ri, c)


@pytest.mark.parametrize("name,sampling,quality,noise", T.STRAGGLER_CASES)
def test_the_oracle_decodes_the_straggler_groups_variants(name, sampling, quality, noise):
    coefs, scan, tables = T.coded(name, sampling, quality, 0, noise)
    rc, got = L.huffman_decode_port([c.shape[:2] for c in coefs], T.W, T.H, T.SAMPLINGS[sampling], 0, scan, tables=tables)
    assert rc == 0
    for c in range(len(coefs)):
        assert np.array_equal(got[c], coefs[c]), (name, sampling, c)


def _libjpeg_reads(jpeg, coefs):
    ref = L.ref()
    buf = np.frombuffer(jpeg, dtype=np.uint8)
    want = [np.zeros(c.shape, dtype=np.int16) for c in coefs]
    ptrs = (C.c_void_p * 3)(*[b.ctypes.data for b in want] + [None] * (3 - len(want)))
    qt = np.zeros((3, 64), dtype=np.uint16)
    bw, bh, nc = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    assert ref.ref_jpeg_read_coefficients(buf.ctypes.data, buf.size, ptrs, qt.ctypes.data, bw, bh, C.byref(nc)) == 0
    assert nc.value == len(coefs) and [(bh[c], bw[c]) for c in range(nc.value)] == [c.shape[:2] for c in coefs]
    return want, qt


@pytest.mark.parametrize("layout", ["one-per-segment", "all-in-one", "redefined"])
@pytest.mark.parametrize("name", NAMES)
def test_libjpeg_reads_the_coefficients_from_the_assembled_file(name, layout):
    """The helper pinned to the reference itself: jpeg_read_coefficients() on assemble_file(...) gives the coefficients that went in,
    for every family and every DHT layout (the sampling changes with the family, the restart interval with the layout)."""
    if L.ref() is None:
        pytest.skip("oracle/_ref not built")
    sampling = list(T.SAMPLINGS)[NAMES.index(name) % 4]
    quality = QUALITY[sampling]
    ri = {"one-per-segment": 0, "all-in-one": 5, "redefined": 0}[layout]
    coefs, scan, tables = T.coded(name, sampling, quality, ri)
    ql, qc = L.quant_table_port(quality, False), L.quant_table_port(quality, True)
    jpeg = T.assemble_file(coefs, T.W, T.H, T.SAMPLINGS[sampling], ri, ql, qc, scan, tables, layout)
    got, qt = _libjpeg_reads(jpeg, coefs)
    for c in range(len(coefs)):
        assert np.array_equal(got[c], coefs[c]), (name, layout, c)
        assert np.array_equal(qt[c], qc if c else ql)


def test_annexk_file_equals_the_oracles_assembler():
    coefs, scan, tables = T.coded("annexk", "420", 100, 0)
    ql, qc = L.quant_table_port(100, False), L.quant_table_port(100, True)
    assert T.assemble_file(coefs, T.W, T.H, T.SAMPLINGS["420"], 0, ql, qc, scan, tables) == L.jpeg_assemble_port(coefs, T.W, T.H, T.SAMPLINGS["420"], 0, ql, qc, scan)


@pytest.mark.parametrize("sampling", list(T.SAMPLINGS))
def test_inverted_scans_are_three_times_as_long(sampling):
    for quality in (95, 100):
        assert len(T.coded("inverted", sampling, quality)[1]) >= 3 * len(T.coded("annexk", sampling, quality)[1])
