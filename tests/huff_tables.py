"""Huffman table families other than Annex K, and a baseline encoder that takes the tables (plain Python and numpy, no GPU).

The device decoder rebuilds every file's DHT tables into five forms (csrc/api_entropy.cpp: make_dec_table, make_fast_table,
make_track_table / make_value_table, make_pair_table / make_pair_value_table); the oracle's encoder knows Annex K only.  Here:
build_dht / long_prefixes / check_dht for tables, FAMILIES for complete sets of four (DC luma, AC luma, DC chroma, AC chroma),
encode_scan for the entropy-coded data of a scan under any such set (T.81 F.1.2, the oracle's encoder restated for numpy: bytes equal
for Annex K), assemble_file for a JFIF file around it with the DHT segments laid out in three ways, and case() for the coefficients
(the builder of tests/test_gpu_huffman_straggler.py, plus a few extreme blocks).  tests/test_huff_tables.py holds all of it to the
oracle's decoder and to libjpeg; tests/test_gpu_huff_tables.py runs the device decoder on it."""
import functools

import numpy as np

from oracle import loader as L

W = H = 256
SAMPLINGS = {"444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "400": [(1, 1)]}
EOB, ZRL = 0x00, 0xF0
AC_SYMBOLS = [(r << 4) | s for r in range(16) for s in range(1, 11)] + [EOB, ZRL]  # the 162 symbols of a baseline AC table
DC_SYMBOLS = list(range(12))
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8)))


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def build_dht(symbols, lengths):
    """(bits[17], vals[256]) uint8: the canonical DHT content for symbols and their code lengths; symbols of one length keep the
    order they are given in (code order)."""
    assert len(symbols) == len(lengths) and len(set(symbols)) == len(symbols)
    bits, vals = np.zeros(17, np.uint8), np.zeros(256, np.uint8)
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])  # (stable)
    for k, i in enumerate(order):
        assert 1 <= lengths[i] <= 16
        bits[lengths[i]] += 1
        vals[k] = symbols[i]
    return bits, vals


def codes_of(bits, vals):
    """T.81 Annex C: (code[256], length[256]) per symbol value; length 0 = the table does not define the symbol."""
    code, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    c = k = 0
    for l in range(1, 17):
        for _ in range(int(bits[l])):
            code[vals[k]], length[vals[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, length


def long_prefixes(bits) -> int:
    """The number of distinct nine-bit prefixes that carry codes longer than nine bits: the sub-tables make_fast_table needs."""
    seen = set()
    c = 0
    for l in range(1, 17):
        for _ in range(int(bits[l])):
            if l > 9:
                seen.add(c >> (l - 9))
            c += 1
        c <<= 1
    return len(seen)


def check_dht(bits, vals, is_dc):
    """A valid DHT table: lengths 1 .. 16, at most 256 distinct symbols, Kraft sum below 1 (the all-ones code of the longest length
    stays unused), DC symbols no larger than 15."""
    n = int(np.sum(bits[1:].astype(int)))
    assert bits[0] == 0 and 1 <= n <= 256
    assert sum(int(bits[l]) << (16 - l) for l in range(1, 17)) < 1 << 16, "Kraft sum"
    assert len(set(vals[:n].tolist())) == n, "a symbol twice"
    assert not vals[n:].any()
    if is_dc:
        assert int(vals[:n].max()) <= 15
    return n


def _tables(*four):
    bits, vals = np.zeros((4, 17), np.uint8), np.zeros((4, 256), np.uint8)
    for t, (b, v) in enumerate(four):
        bits[t], vals[t] = b, v
    return bits, vals


def _hot_first(symbols, hot):
    return list(hot) + [s for s in symbols if s not in hot]


# what a photographic scan uses most, most frequent first (the head of Annex K's AC tables, ZRL added)
HOT_AC = [EOB, 0x01, 0x11, 0x02, 0x21, 0x03, 0x12, 0x31, 0x41, 0x04, ZRL, 0x51, 0x13, 0x22, 0x05, 0x61]


def _annexk():
    return L.std_dht_tables()


def _inverted():
    """Annex K's lengths with the symbols in reverse order: the rare symbols get the short codes; EOB, 0x01, 0x11, 0x02 and ZRL sit among
    the 16-bit codes.  Annex K's DC lengths end at 9 and 11 bits, so the DC tables also stretch their four longest codes (categories
    3 .. 0) to 15, 15, 16 and 16 bits."""
    bits, vals = L.std_dht_tables()
    out = []
    for t in range(4):
        n = int(bits[t, 1:].sum())
        lengths = [l for l in range(1, 17) for _ in range(int(bits[t, l]))]
        if t % 2 == 0:
            lengths[-4:] = [15, 15, 16, 16]
        out.append(build_dht(vals[t, :n][::-1].tolist(), lengths))
    return _tables(*out)


# 162 lengths whose long codes fill exactly sixteen nine-bit prefixes: 74 codes of nine bits or fewer, then 16 / 16 / 16 / 16 codes of
# 10 .. 13 bits (8 + 4 + 2 + 1 prefixes) and 8 / 8 / 8 of 14 .. 16 bits (one more).  The symbols alternate between the short and the
# long half in order of frequency, so that every block reads both levels.
_DEEP_SHORT = [2, 3, 4, 4, 5, 5, 6, 6] + [7] * 6 + [8] * 24 + [9] * 36
_DEEP_LONG = [10] * 16 + [11] * 16 + [12] * 16 + [13] * 16 + [14] * 8 + [15] * 8 + [16] * 8
# ... and seventeen: 24 nine-bit codes fewer, 32 codes of 14 bits (a prefix of their own), the 15- and 16-bit codes in a seventeenth
_DEEP17_SHORT = _DEEP_SHORT[:-24]
_DEEP17_LONG = [10] * 16 + [11] * 16 + [12] * 16 + [13] * 16 + [14] * 32 + [15] * 8 + [16] * 8


def _deep_ac(short, long_, hot=HOT_AC):
    syms = _hot_first(AC_SYMBOLS, hot)
    assert len(short) + len(long_) == len(syms)
    lengths = {}
    s, l = list(short), list(long_)
    for i, sym in enumerate(syms):
        take_long = (i % 2 == 1 and l) or not s
        lengths[sym] = l.pop(0) if take_long else s.pop(0)
    return build_dht(syms, [lengths[x] for x in syms])


def _flat_dc():
    return build_dht(DC_SYMBOLS, [4] * 12)


def _deep16():
    ac = _deep_ac(_DEEP_SHORT, _DEEP_LONG)
    return _tables(_flat_dc(), ac, _flat_dc(), ac)


def _deep33():
    """deep16, except that DC luma has one code longer than nine bits (category 11 on ten bits)."""
    ac = _deep_ac(_DEEP_SHORT, _DEEP_LONG)
    return _tables(build_dht(DC_SYMBOLS, [4] * 11 + [10]), ac, _flat_dc(), ac)


def _deep17():
    """AC luma with seventeen prefixes, the other three tables as deep16."""
    ac = _deep_ac(_DEEP_SHORT, _DEEP_LONG)
    ac17 = _deep_ac(_DEEP17_SHORT, _DEEP17_LONG)
    return _tables(_flat_dc(), ac17, _flat_dc(), ac)


def _dc_long():
    """All four tables with sub-tables, 3, 6, 2 and 4 of them: DC luma on lengths 1 .. 7, four times 10 and 16 (category 11: 16 + 11
    bits), DC chroma on 2, 2, 3 .. 8, three times 10 and 11, the AC tables with fewer prefixes than deep16."""
    dc_l = build_dht(DC_SYMBOLS, list(range(1, 8)) + [10] * 4 + [16])
    dc_c = build_dht(DC_SYMBOLS, [2, 2, 3, 4, 5, 6, 7, 8, 10, 10, 10, 11])
    ac_l = _deep_ac([2, 3, 4, 5, 5, 6, 6] + [7] * 7 + [8] * 24 + [9] * 96, [10] * 6 + [11] * 6 + [12] * 4 + [13] * 4 + [14] * 4 + [16] * 4)
    ac_c = _deep_ac([2, 3, 4, 4, 5, 5, 6, 6] + [7] * 6 + [8] * 24 + [9] * 100, [10] * 4 + [11] * 4 + [12] * 4 + [14] * 4 + [15] * 4 + [16] * 4)
    return _tables(dc_l, ac_l, dc_c, ac_c)


def _short_first():
    """EOB and DC category 0 on one-bit codes, the next most frequent symbols on two and three bits."""
    syms = _hot_first(AC_SYMBOLS, HOT_AC)
    ac = build_dht(syms, [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 11] + [12] * 4 + [16] * 147)
    dc = build_dht(DC_SYMBOLS, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    return _tables(dc, ac, dc, ac)


def _flat():
    """Every AC symbol on an eight-bit code (162 < 255), every DC symbol on four bits."""
    ac = build_dht(AC_SYMBOLS, [8] * 162)
    return _tables(_flat_dc(), ac, _flat_dc(), ac)


def shallow_tables(used):
    """AC tables that hold only the symbols in `used` ([luma set, chroma set]; EOB and ZRL always), all on nine bits or fewer; DC
    tables on four bits flat.  Most of both first levels stays undefined."""
    out = []
    for t in range(2):
        syms = _hot_first(sorted(set(used[t]) | {EOB, ZRL}), [s for s in HOT_AC if s in used[t] or s in (EOB, ZRL)])
        n = len(syms)
        assert n <= 162
        # 3, 4, 5, 6 bits for the first eight, then as many seven- and eight-bit codes as leave the rest on nine bits with room to spare
        lengths = ([3, 4, 4, 5, 5, 6, 6, 6] + [7] * 8 + [8] * 24 + [9] * 122)[:n]
        out.append(build_dht(syms, lengths))
    return _tables(_flat_dc(), out[0], _flat_dc(), out[1])


FAMILIES = {"annexk": _annexk, "inverted": _inverted, "deep16": _deep16, "deep33": _deep33, "deep17": _deep17, "dc_long": _dc_long,
            "short_first": _short_first, "shallow": None, "flat": _flat}
# sub-tables per table (long_prefixes) that each family is built to have; shallow: none, whatever the case uses
PREFIXES = {"deep16": (0, 16, 0, 16), "deep33": (1, 16, 0, 16), "deep17": (0, 17, 0, 16), "dc_long": (3, 6, 2, 4)}


@functools.lru_cache(maxsize=None)
def family(name, sampling="420", quality=95, noise=None):
    """(bits[4][17], vals[4][256]) of a family; `shallow` is cut to the symbols the case (sampling, quality, noise) uses."""
    if name == "shallow":
        tk = _tokens(sampling, quality, 0, noise)
        ac = tk["tab"] % 2 == 1
        return shallow_tables([set(tk["sym"][ac & (tk["tab"] == 1)].tolist()), set(tk["sym"][ac & (tk["tab"] == 3)].tolist())])
    return FAMILIES[name]()


# ---- coefficients ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(sampling, quality, noise=None):
    """Coefficients of the 256 x 256 noise-textured image of tests/test_gpu_huffman_straggler.py (q95, or q100 with the noise scaled by
    0.3), left unchanged once built -- plus, in one block of 37, a DC term at the end of its range with alternating sign and one AC term of
    ten magnitude bits: DC differences of category 11 and AC size 10, the symbols with the most bits behind a code."""
    from test_gpu_huffman_straggler import _case

    coefs = [c.copy() for c in _case(sampling, quality, False, noise)[0]]
    rng = np.random.default_rng(77 + quality + len(sampling) + int(sampling))
    for c in coefs:
        flat = c.reshape(-1, 64)
        idx = np.arange(rng.integers(0, 37), flat.shape[0], 37)
        flat[idx, 0] = np.where(np.arange(idx.size) % 2 == 0, 1016, -1024)
        flat[idx, rng.integers(1, 64, idx.size)] = (rng.integers(512, 1024, idx.size) * rng.choice([-1, 1], idx.size)).astype(np.int16)
    for c in coefs:
        c.setflags(write=False)
    return coefs


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def _scan_blocks(coefs, w, h, sampling):
    """Blocks in scan order: (zig-zag coefficients [n, 64], component [n], blocks per MCU).  Dummy blocks at the right and bottom edges
    of an interleaved scan: AC zero, DC equal to the previous block of the MCU (0 in front of its first)."""
    nc = len(coefs)
    if nc == 1:
        return coefs[0].reshape(-1, 64)[:, ZIGZAG].astype(np.int32), np.zeros(coefs[0].shape[0] * coefs[0].shape[1], np.int32), 1
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    mpr, mrows = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    bpm = sum(hs * vs for hs, vs in sampling)
    out = np.zeros((mrows, mpr, bpm, 64), np.int32)
    real = np.zeros((mrows, mpr, bpm), bool)
    comp = np.zeros(bpm, np.int32)
    j = 0
    for c, (hs, vs) in enumerate(sampling):
        bh, bw = coefs[c].shape[:2]
        padded = np.zeros((mrows * vs, mpr * hs, 64), np.int32)
        padded[:bh, :bw] = coefs[c][..., ZIGZAG]
        ok = np.zeros((mrows * vs, mpr * hs), bool)
        ok[:bh, :bw] = True
        for yi in range(vs):
            for xi in range(hs):
                out[:, :, j] = padded[yi::vs, xi::hs]
                real[:, :, j] = ok[yi::vs, xi::hs]
                comp[j] = c
                j += 1
    for j in range(bpm):  # the dummy rule, in MCU order
        prev = out[:, :, j - 1, 0] if j else np.zeros((mrows, mpr), np.int32)
        out[:, :, j, 0] = np.where(real[:, :, j], out[:, :, j, 0], prev)
    return out.reshape(-1, 64), np.tile(comp, mrows * mpr), bpm


def _bit_length(a):
    return np.frexp(a.astype(np.float64))[1].astype(np.int64) * (a > 0)


def scan_tokens(coefs, w, h, sampling, restart_interval):
    """The scan as symbols, before any table is chosen: per token the table (0 .. 3), the symbol, the magnitude bits and their number,
    and the token index every restart interval starts at."""
    zz, comp, bpm = _scan_blocks(coefs, w, h, sampling)
    n = zz.shape[0]
    per = restart_interval * bpm if restart_interval > 0 else n  # blocks per interval
    # DC differences per component, the prediction starting over with every interval
    diff = np.zeros(n, np.int64)
    for c in range(len(coefs)):
        sel = np.flatnonzero(comp == c)
        dc = zz[sel, 0].astype(np.int64)
        prev = np.concatenate([[0], dc[:-1]])
        first = np.concatenate([[True], (sel[1:] // per) != (sel[:-1] // per)])
        prev[first] = 0
        diff[sel] = dc - prev
    blk = np.arange(n, dtype=np.int64)
    toks = [(blk * 260, 2 * (comp != 0), _bit_length(np.abs(diff)), diff)]  # (sort key, table, symbol, value)
    b, k = np.nonzero(zz[:, 1:])
    k = k + 1
    v = zz[b, k].astype(np.int64)
    newblk = np.concatenate([[True], b[1:] != b[:-1]]) if b.size else np.zeros(0, bool)
    prevk = np.where(newblk, 0, np.concatenate([[0], k[:-1]]))
    run = k - prevk - 1
    size = _bit_length(np.abs(v))
    assert size.size == 0 or size.max() <= 10, "AC term beyond ten bits"
    tab_ac = 1 + 2 * (comp[b] != 0)
    toks.append((b * 260 + k * 4 + 3, tab_ac, ((run % 16) << 4) | size, v))
    for j in range(1, 4):
        m = run // 16 >= j
        toks.append((b[m] * 260 + k[m] * 4 + j - 1, tab_ac[m], np.full(int(m.sum()), ZRL), np.zeros(int(m.sum()), np.int64)))
    last = np.zeros(n, np.int64)
    last[b] = k  # (ascending within a block: the last one stays)
    e = np.flatnonzero(last < 63)
    toks.append((e * 260 + 259, 1 + 2 * (comp[e] != 0), np.full(e.size, EOB), np.zeros(e.size, np.int64)))
    key = np.concatenate([t[0] for t in toks])
    order = np.argsort(key, kind="stable")
    tab = np.concatenate([t[1] for t in toks])[order]
    sym = np.concatenate([t[2] for t in toks])[order]
    val = np.concatenate([t[3] for t in toks])[order]
    nbits = np.where(sym == ZRL, 0, np.where(tab % 2 == 0, sym, sym & 15))
    assert nbits.max() <= 11, "DC difference beyond eleven bits"
    extra = np.where(val < 0, val + (1 << nbits) - 1, val)  # F.1.2.1: a negative value is coded as value - 1, its low bits
    starts = np.searchsorted(key[order], np.arange(0, n, per) * 260)
    return {"tab": tab.astype(np.int64), "sym": sym.astype(np.int64), "extra": extra.astype(np.uint64), "nbits": nbits.astype(np.int64), "starts": starts}


def pack_tokens(tk, tables) -> bytes:
    """Codes and magnitude bits MSB first, every interval padded with ones to a byte, 0xFF followed by a stuffed zero, RSTn between
    the intervals."""
    bits, vals = tables
    code, length = np.zeros((4, 256), np.uint64), np.zeros((4, 256), np.int64)
    for t in range(4):
        code[t], length[t] = codes_of(bits[t], vals[t])
    ln = length[tk["tab"], tk["sym"]]
    assert ln.min() > 0, "a symbol of the scan has no code in these tables"
    value = (code[tk["tab"], tk["sym"]] << tk["nbits"].astype(np.uint64)) | tk["extra"]
    ln = ln + tk["nbits"]
    # the padding of every interval as one more token behind it
    starts = tk["starts"]
    total = np.add.reduceat(ln, starts)
    pad = (-total) % 8
    at = np.concatenate([starts[1:], [ln.size]])
    ln = np.insert(ln, at, pad)
    value = np.insert(value, at, ((1 << pad) - 1).astype(np.uint64))
    end_bytes = np.cumsum(total + pad) // 8  # where the intervals end, in unstuffed bytes
    pos = np.concatenate([[0], np.cumsum(ln)[:-1]])
    stream = np.zeros(int(ln.sum()), np.uint8)
    for b in range(int(ln.max())):  # bit b of every token that has one, counted from its low end
        m = ln > b
        stream[pos[m] + ln[m] - 1 - b] = ((value[m] >> np.uint64(b)) & np.uint64(1)).astype(np.uint8)
    raw = np.packbits(stream)
    ff = np.flatnonzero(raw == 0xFF)
    out = np.insert(raw, ff + 1, 0)
    if starts.size > 1:
        cuts = end_bytes[:-1]
        cuts = cuts + np.searchsorted(ff, cuts)  # stuffed zeros in front of each cut
        marks = np.stack([np.full(cuts.size, 0xFF), 0xD0 + np.arange(cuts.size) % 8], axis=1).astype(np.uint8)
        out = np.insert(out, np.repeat(cuts, 2), marks.reshape(-1))
    return out.tobytes()


def encode_scan(coefs, w, h, sampling, restart_interval, tables) -> bytes:
    """Baseline sequential entropy coding (everything between the SOS header and EOI) under `tables` = (bits[4][17], vals[4][256]):
    DC luma, AC luma, DC chroma, AC chroma."""
    return pack_tokens(scan_tokens(coefs, w, h, sampling, restart_interval), tables)


@functools.lru_cache(maxsize=None)
def _tokens(sampling, quality, restart_interval, noise=None):
    return scan_tokens(case(sampling, quality, noise), W, H, SAMPLINGS[sampling], restart_interval)


@functools.lru_cache(maxsize=None)
def coded(name, sampling, quality, restart_interval=0, noise=None):
    """(coefficients, scan bytes, tables) of a family on a case; built once.  Every scan has the 4096 bytes the parallel route asks for."""
    tables = family(name, sampling, quality, noise)
    scan = pack_tokens(_tokens(sampling, quality, restart_interval, noise), tables)
    assert len(scan) >= 4096, (name, sampling, quality, noise, len(scan))
    return case(sampling, quality, noise), scan, tables


# The cases of the forced-straggler group of tests/test_gpu_huff_tables.py: (family, sampling, quality, noise scale; None = the case's
# own).  That file's docstring says which variants were swapped in and why.
STRAGGLER_CASES = [("inverted", "420", 95, 0.5), ("inverted", "444", 95, 0.5), ("deep16", "420", 95, None), ("deep16", "444", 95, None),
                   ("dc_long", "420", 95, None), ("dc_long", "444", 95, None), ("short_first", "420", 100, None), ("short_first", "444", 100, None)]


# ---- files ----------------------------------------------------------------------------------------------------------------------
def _segment(marker, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _dht_payload(tc, th, bits, vals) -> bytes:
    n = int(np.sum(bits[1:].astype(int)))
    return bytes([(tc << 4) | th]) + bytes(bits[1:].tolist()) + bytes(vals[:n].tolist())


def assemble_file(coefs, w, h, sampling, ri, qt_luma, qt_chroma, scan, tables, dht_layout="one-per-segment") -> bytes:
    """A complete baseline JFIF file around the scan (T.81 B.2: SOI, APP0, DQT, SOF0, DHT, DRI, SOS, data, EOI).  dht_layout:
    "one-per-segment"; "all-in-one" (one DHT segment holds every table); "redefined" (an Annex K table of the same class and id in
    front of the frame header, the real one behind it: the later definition holds)."""
    nc = len(coefs)
    ntab = 2 if nc > 1 else 1
    out = bytes([0xFF, 0xD8]) + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t, qt in enumerate((qt_luma, qt_chroma)[:ntab]):
        out += _segment(0xDB, bytes([t]) + bytes(int(qt[ZIGZAG[i]]) for i in range(64)))
    ids = [(t % 2, t // 2, t) for t in range(2 * ntab)]  # (class, id, index into the four tables)
    if dht_layout == "redefined":
        std = L.std_dht_tables()
        for tc, th, t in ids:
            out += _segment(0xC4, _dht_payload(tc, th, std[0][t], std[1][t]))
    frame = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        hs, vs = sampling[c] if nc > 1 else (1, 1)
        frame += bytes([c + 1, (hs << 4) | vs, 1 if c else 0])
    out += _segment(0xC0, frame)
    payloads = [_dht_payload(tc, th, tables[0][t], tables[1][t]) for tc, th, t in ids]
    if dht_layout == "all-in-one":
        out += _segment(0xC4, b"".join(payloads))
    else:
        assert dht_layout in ("one-per-segment", "redefined"), dht_layout
        for p in payloads:
            out += _segment(0xC4, p)
    if ri:
        out += _segment(0xDD, ri.to_bytes(2, "big"))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([c + 1, 0x11 if c else 0x00])
    out += _segment(0xDA, sos + bytes([0, 63, 0]))
    return out + scan + bytes([0xFF, 0xD9])
