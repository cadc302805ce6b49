"""The MCU layouts the entropy codec accepts, and scans of every one of them (plain Python and numpy, no GPU).

check_scan (csrc/api_entropy.cpp) admits one-component scans and three-component scans with every sampling factor in {1, 2} and at
most 10 blocks per MCU (T.81 B.2.3): 63 layouts of 3 .. 10 blocks per MCU; all three components at 2x2 (12 blocks) is refused, as
libjpeg refuses the file.  Here: LAYOUTS / REPRESENTATIVES, the grids of a layout (real blocks, MCU-padded), the random "sparse" and
"dense" coefficients of tests/test_gpu_parity.py on any grids, a photo-like generator (the one of tests/test_gpu_huffman_straggler.py,
which imports it from here), a file with the largest DC swing in front of the first block of every component of an MCU, and the level
count the decoder's default ladder starts with per blocks-per-MCU value.  tests/test_mcu_layouts.py holds all of it to the oracle's
decoder and to libjpeg; tests/test_gpu_mcu_layouts.py runs the device on it."""
import functools
import itertools
import re

import numpy as np

from oracle import loader as L

_FACTORS = [(1, 1), (2, 1), (1, 2), (2, 2)]
ILLEGAL = [(2, 2)] * 3  # 12 blocks per MCU
LAYOUTS = [list(t) for t in itertools.product(_FACTORS, repeat=3) if list(t) != ILLEGAL]


def layout_id(sampling) -> str:
    return "-".join(f"{hs}{vs}" for hs, vs in sampling)


IDS = [layout_id(s) for s in LAYOUTS]

# the layouts that carry the route-pinned tests (tests/test_mcu_layouts.py checks what they hold together)
REPRESENTATIVES = [
    [(1, 2), (1, 1), (1, 1)],  # 4:4:0 -- a losslessly rotated 4:2:2 file; 4 blocks per MCU
    [(1, 1), (2, 1), (1, 1)],  # a chroma component finer than luma; 4
    [(2, 1), (1, 2), (1, 1)],  # hmax and vmax from different components; 5
    [(1, 1), (1, 2), (1, 2)],  # 5
    [(1, 1), (1, 1), (2, 2)],  # a last component of 2x2; 6
    [(2, 2), (2, 1), (1, 1)],  # Cb finer than Cr; 7
    [(2, 2), (1, 1), (1, 2)],  # Cr finer than Cb; 7
    [(2, 2), (2, 1), (2, 1)],  # 8
    [(2, 1), (2, 2), (1, 2)],  # 8
    [(2, 2), (2, 2), (1, 1)],  # 9
    [(1, 1), (2, 2), (2, 2)],  # 9
    [(2, 2), (2, 2), (2, 1)],  # 10
    [(2, 2), (1, 2), (2, 2)],  # 10
]
REP_IDS = [layout_id(s) for s in REPRESENTATIVES]

# Overflow levels of the first attempt of the decoder's default ladder per blocks-per-MCU value: a path's slot row is levels x
# blocks-per-MCU of the 48 slots, the ladder takes the largest of 15 / 11 / 7 / 4 that leaves one row free, and at 10 blocks per
# MCU not even 4 fit: the rounds alone.  Written out, not computed: the table is what the library's debug line is held to.
DEFAULT_LEVELS = {3: 15, 4: 11, 5: 7, 6: 7, 7: 4, 8: 4, 9: 4, 10: "rounds"}
# ... and the most levels a pinned attempt (UHDR_HIP_HUFF_LEVELS) may ask for before it silently falls to the rounds:
# blocks-per-MCU x (levels + 1) <= 48, at the level counts the pins use
PINNED_LEVELS = {3: 7, 4: 7, 5: 7, 6: 7, 7: 4, 8: 4, 9: 4, 10: 3}

W, H = 136, 104  # 17 x 13 full-resolution blocks, odd both ways: the smallest shape that keeps every route reachable for every layout
SIZES = [(W, H), (16, 16), (130, 9)]
# The photo-like content's noise scale.  tests/test_gpu_huffman_straggler.py uses 1.0 at 256 x 256; at W x H that leaves 20 layouts under
# the 4096 bytes the parallel decoder asks for (3338 at the least), 2.0 gives 5126 .. 11 K bytes at 120 .. 147 bits per block.
PHOTO_NOISE = 2.0
# The pinned straggler cases whose content was swapped: {(layout id, subsequence bits, lockstep levels): noise scale}; the docstring of
# tests/test_gpu_mcu_layouts.py says why, with the library's debug line.
STRAGGLER_NOISE = {
    ("22-22-21", 512, 1): 1.0, ("22-22-21", 512, 2): 0.6,  # calmer: three levels of 512 bits lose the true path from x 1.5 up
    # busier: at x 2 nothing is left for the stragglers after two lockstep levels of 1024 bits
    ("12-11-11", 1024, 2): 4.0, ("11-21-11", 1024, 2): 3.0, ("11-12-12", 1024, 2): 4.0, ("11-11-22", 1024, 2): 3.0, ("22-21-11", 1024, 2): 3.0,
    ("22-21-21", 1024, 2): 4.0, ("21-22-12", 1024, 2): 4.0, ("11-22-22", 1024, 2): 3.0, ("22-12-22", 1024, 2): 3.0,
}
SMALL_MAX_BITS = 32736  # tests/test_gpu_huffman_encode_one_walk.py: a segment leaves the encoder's small size class above this


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def blocks_per_mcu(sampling) -> int:
    return sum(hs * vs for hs, vs in sampling)


def mcu_grid(w, h, sampling):
    """(MCUs per row, MCU rows) of an interleaved scan."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return -(-w // (8 * hmax)), -(-h // (8 * vmax))


def real_grids(w, h, sampling):
    """[(blocks_h, blocks_w)] per component: jpeg_component_info::height_in_blocks / width_in_blocks."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [(-(-(-(-h * vs // vmax)) // 8), -(-(-(-w * hs // hmax)) // 8)) for hs, vs in sampling]


def padded_grids(w, h, sampling):
    """[(blocks_h, blocks_w)] per component, padded to whole MCUs (what check_scan takes as well: no dummy blocks)."""
    mpr, mrows = mcu_grid(w, h, sampling)
    return [(mrows * vs, mpr * hs) for hs, vs in sampling]


def segment_mcus(sampling) -> int:
    """MCUs per segment of the marker-less encoder: one wavefront, the first MCU's lanes carry the MCU in front of the segment."""
    return 64 // blocks_per_mcu(sampling) - 1


def last_segment_of_one_mcu(sampling):
    """(w, h) of one MCU row of segment_mcus + 1 MCUs, a few pixels short of whole MCUs where that leaves the grid alone."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return 8 * hmax * (segment_mcus(sampling) + 1) - 3, 8 * vmax - 3


def restart_intervals(sampling):
    """The restart intervals the encoder's interval kernel is run at: 1, one that packs more than one interval into a wavefront
    (2 * ri * blocks-per-MCU <= 64), and the largest the encoder takes."""
    top = 64 // blocks_per_mcu(sampling)
    return [1, top // 2, top]


def eight_intervals(w, h, sampling) -> int:
    """The restart interval that cuts the scan into 8 intervals."""
    mpr, mrows = mcu_grid(w, h, sampling)
    return -(-mpr * mrows // 8)


def has_dummy_blocks(w, h, sampling):
    """(a dummy column, a dummy row): some component's real grid is narrower / lower than its MCU-padded grid."""
    real, pad = real_grids(w, h, sampling), padded_grids(w, h, sampling)
    return any(r[1] < p[1] for r, p in zip(real, pad)), any(r[0] < p[0] for r, p in zip(real, pad))


# ---- content --------------------------------------------------------------------------------------------------------------------
def random_coefs(rng, grids, kind):
    """tests/test_gpu_parity.py's _random_coefs on any grids.  "sparse": what a q ~ 90 photo looks like -- few non-zero terms, long zero
    runs (ZRL), many EOBs; "dense": every term non-zero, all size categories."""
    coefs = []
    for bh, bw in grids:
        if kind == "sparse":
            a = (rng.normal(0, 25, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.12)).astype(np.int16)
            a[..., 0] = rng.integers(-1000, 1000, (bh, bw))
            a[..., 63] = np.where(rng.random((bh, bw)) < 0.3, 1, a[..., 63])
        else:
            assert kind == "dense", kind
            a = rng.integers(-1023, 1024, (bh, bw, 64)).astype(np.int16)
            a[a == 0] = 1
        coefs.append(np.ascontiguousarray(a))
    return coefs


def photo_coefs(rng, grids_wh, quality, noise):
    """Coefficients of a noise-textured image: per component ((blocks_w, blocks_h) in grids_wh) a smooth field under noise whose
    amplitude varies over the picture -- calm regions (end-of-block codes, zero runs) next to busy ones (blocks coded up to the last
    term) -- through the oracle's FDCT and quantisation at `quality`.  noise: the scale of the noise."""
    coefs = []
    for c, (bw, bh) in enumerate(grids_wh):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
        amp = 0.3 + 7.0 * (0.5 + 0.5 * np.sin(xx / 23.0 + c) * np.cos(yy / 17.0)) ** 2
        pl = 128 + 70 * np.sin(xx / (29.0 + 5 * c)) * np.cos(yy / (21.0 + 3 * c)) + rng.normal(0, 1, (bh * 8, bw * 8)) * amp * noise
        qt = L.quant_table_port(quality, c > 0)
        coefs.append(L.fdct_quant_port(np.ascontiguousarray(np.clip(np.rint(pl), 0, 255).astype(np.uint8)), bw * 8, bw, bh, qt))
    return coefs


def _seed(sampling) -> int:
    return int(layout_id(sampling).replace("-", ""))


def _frozen(coefs):
    for c in coefs:
        c.setflags(write=False)
    return coefs


@functools.lru_cache(maxsize=None)
def _photo(lid, w, h, quality, noise):
    sampling = LAYOUTS[IDS.index(lid)]
    rng = np.random.default_rng(1000 * _seed(sampling) + quality)
    return _frozen(photo_coefs(rng, [(bw, bh) for bh, bw in real_grids(w, h, sampling)], quality, noise))


def photo_case(sampling, quality=95, noise=1.0, ri=0, w=W, h=H):
    """(coefficients, the oracle's scan) of the photo-like image of a layout; built once, left unchanged."""
    return _coded("photo", layout_id(sampling), w, h, quality, noise, ri)


def random_case(sampling, kind, ri=0, w=W, h=H, padded=False):
    """(coefficients, the oracle's scan) of "sparse" / "dense" random coefficients on the real or the MCU-padded grids."""
    return _coded(kind, layout_id(sampling), w, h, 0, 0.0, ri, padded)


def dc_swing_case(sampling, ri=0, w=W, h=H):
    """The "sparse" case with, for every component, the last block of the component in one MCU at DC -1024 and its first block in the
    next MCU at +1023: the largest DC difference there is (2047, category 11), right where the prediction crosses from one MCU into the
    next.  The MCU pairs are (1, 1 + c) -> (1, 2 + c) for component c: real blocks of every layout at W x H."""
    return _coded("swing", layout_id(sampling), w, h, 0, 0.0, ri)


def swing_blocks(sampling):
    """[(component, (by, bx) of the -1024 block, (by, bx) of the +1023 block)] of dc_swing_case."""
    out = []
    for c, (hs, vs) in enumerate(sampling):
        my, mx = 1, 2 + c
        out.append((c, (my * vs + vs - 1, (mx - 1) * hs + hs - 1), (my * vs, mx * hs)))
    return out


@functools.lru_cache(maxsize=None)
def _coded(kind, lid, w, h, quality, noise, ri, padded=False):
    sampling = LAYOUTS[IDS.index(lid)]
    if kind == "photo":
        coefs = _photo(lid, w, h, quality, noise)
    else:
        rng = np.random.default_rng(7000 + _seed(sampling) + w * 3 + h + (1 if kind == "dense" else 0))
        grids = padded_grids(w, h, sampling) if padded else real_grids(w, h, sampling)
        coefs = random_coefs(rng, grids, "sparse" if kind == "swing" else kind)
        if kind == "swing":
            for c, lo, hi in swing_blocks(sampling):
                assert hi[0] < coefs[c].shape[0] and hi[1] < coefs[c].shape[1], (lid, c)
                coefs[c][lo[0], lo[1], 0], coefs[c][hi[0], hi[1], 0] = -1024, 1023
        _frozen(coefs)
    return coefs, L.huffman_encode_port(coefs, w, h, sampling, ri)


def segment_bits(coefs, w, h, sampling):
    """Coded bits of every segment of the marker-less encoder (segment_mcus MCUs each, the last one shorter), counted by the oracle:
    the scan with the segment length as its restart interval has one byte-padded interval per segment, so a segment's bits lie within
    7 of 8 x its unstuffed bytes (the DC prediction starts over at each cut, which moves a segment by a few bits -- far less than the
    distance the cases keep from the size-class threshold)."""
    scan = L.huffman_encode_port(coefs, w, h, sampling, segment_mcus(sampling))
    # (inside entropy-coded data a 0xFF is followed by a stuffed zero or is an RSTn marker)
    return [8 * (len(p) - p.count(b"\xff\x00")) for p in re.split(rb"\xff[\xd0-\xd7]", scan)]


def assemble(coefs, w, h, sampling, ri, scan, quality=95):
    """(quantisation tables, a complete baseline JFIF file around the scan)."""
    ql, qc = L.quant_table_port(quality, False), L.quant_table_port(quality, True)
    return (ql, qc), L.jpeg_assemble_port(coefs, w, h, sampling, ri, ql, qc, scan)
