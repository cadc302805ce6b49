"""GPU: the straggler waves of the self-synchronising Huffman decoder (csrc/huffman_decode_sync.hip: hyp_straggler_kernel) --
the scalar walk that follows one path per wave, its lane index and zig-zag index packed in one register.

Small scans (256 x 256 noise-textured images through the oracle's FDCT and quantisation at q95 and q100, coded by the oracle's
Huffman encoder) decoded with the subsequence size pinned and ONE lockstep level, so that every path still alive after it goes to
the straggler waves.  The decode must give back the coefficients that were coded (what tests/test_gpu_huffman_sync.py compares
with), and every case must really have used the stragglers: the library's debug line (UHDR_HIP_HUFF_DEBUG) has to report a
non-zero number of "paths handed to the straggler waves" and "true path resolved" -- a case that hands over nothing, or whose
first attempt is lost and repeated by another route, would test nothing and fails.

q100 blocks reach the zig-zag index 64 without an end-of-block code and carry ZRL runs (checked when the case is built);
UHDR_HIP_HUFF_SUB_BITS=512 walks whole subsequences, =1024 walks four pieces and leaves the notes at the cuts; one scan ends
in a last subsequence shorter than 64 bits (rounds of fewer than 64 bit positions up to the end of the stream, zeros beyond it);
one 4:2:0 scan takes two lockstep levels, the base image's route.

Paths handed to the straggler waves, as reported by the library before the packed step was introduced (the counts are a
property of the scans, not of the walk; "true path resolved" in every case):
    sampling  quality  512 bits  1024 bits
    4:4:4     q95            33          3
    4:4:4     q100          599        150
    4:2:0     q95            91         13
    4:2:0     q100          478        118
    4:2:2     q95            61          8
    4:2:2     q100          519         89
    one comp  q95            11          1
    one comp  q100           88         11
    4:4:4 q95 with the short last subsequence, 512 bits: 35;  4:2:0 q95, 512 bits, two lockstep levels: 11
At q100 the noise is scaled by 0.3: with the full scale the busy blocks (a code for nearly every term) keep 2 .. 52 paths from
falling in step within the 7 / 4 levels these sizes get, the first attempt is lost and the decode is repeated by another route.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from oracle import loader as L

from mcu_layouts import photo_coefs

pytestmark = pytest.mark.gpu

W = H = 256
S444, S420, S422, S400 = [(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 1)]
SAMPLINGS = {"444": S444, "420": S420, "422": S422, "400": S400}
SEED = {("444", 95): 11, ("420", 95): 12, ("422", 95): 13, ("400", 95): 14, ("444", 100): 11, ("420", 100): 12, ("422", 100): 13, ("400", 100): 14}
AMP = {95: 1.0, 100: 0.3}  # the noise's scale: at q100 (every step 1) busy blocks of full-scale noise never fall in step within the levels


def _grids(sampling):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-W * hs // hmax) + 7) // 8, (-(-H * vs // vmax) + 7) // 8) for hs, vs in sampling]


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    assert order[:6] == [0, 1, 8, 16, 9, 2] and order[-1] == 63
    return np.array(order)


def _has_zrl(c):
    """A run of 16 or more zeros in front of a non-zero AC term, in zig-zag order, somewhere."""
    nz = c[..., _zigzag()][..., 1:] != 0
    idx = np.where(nz, np.arange(1, 64), 0)
    prev = np.maximum.accumulate(idx, axis=-1)
    prev = np.concatenate([np.zeros_like(prev[..., :1]), prev[..., :-1]], axis=-1)
    return bool((nz & (np.arange(1, 64) - prev > 16)).any())


@functools.lru_cache(maxsize=None)
def _case(name, quality, short_tail=False, noise=None):
    """(coefficients, scan) of a noise-textured image: a smooth field under noise whose amplitude varies over the picture -- calm
    regions (end-of-block codes, zero runs) next to busy ones (blocks coded up to the last term).  Built once, left unchanged.
    noise: the noise's scale, None = AMP[quality] (tests/huff_tables.py asks for calmer and busier variants)."""
    sampling = SAMPLINGS[name]
    rng = np.random.default_rng(1000 * SEED[name, quality] + quality)
    coefs = photo_coefs(rng, _grids(sampling), quality, AMP[quality] if noise is None else noise)  # (shared with the layouts of tests/mcu_layouts.py)
    scan = L.huffman_encode_port(coefs, W, H, sampling, 0)
    if short_tail:
        # clean length (stuffed zero bytes dropped) = 1 .. 7 bytes beyond a multiple of 64: the last 512-bit subsequence is shorter than
        # 64 bits and the length no multiple of 8 bytes.  The last block's AC terms are redrawn until the coded length fits.
        for _ in range(400):
            nclean = len(scan) - scan.count(b"\xff\x00")
            if 1 <= nclean % 64 <= 7:
                break
            coefs[-1][-1, -1, 1:] = (rng.integers(-300, 301, 63) * (rng.random(63) < rng.random())).astype(np.int16)
            scan = L.huffman_encode_port(coefs, W, H, sampling, 0)
        nclean = len(scan) - scan.count(b"\xff\x00")
        assert 1 <= nclean % 64 <= 7, nclean
    if quality == 100 and noise is None:
        assert any((c[..., 63] != 0).any() for c in coefs), "no block is coded up to its last term"
        assert any(_has_zrl(c) for c in coefs), "no ZRL run"
    assert len(scan) >= 4096 or noise is not None
    return coefs, scan


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def _dev(scan):
    import torch

    return torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to("cuda:0")


def _parallel(uhdr):
    st = A.Stats()
    uhdr.lib.uhdr_hip_get_stats(uhdr.ctx.handle, C.byref(st))
    return st.entropy_decode_parallel


def decode_with_stragglers(uhdr, monkeypatch, capfd, name, quality, sub_bits, main_levels, short_tail=False, tables=None, coded=None):
    """Decodes the case with the stragglers forced; returns the number of paths they were handed.  Asserts everything else.
    tables / coded: the DHT tables (None: Annex K) and the (coefficients, scan) coded with them, in place of the case's own
    (tests/test_gpu_huff_tables.py)."""
    coefs, scan = coded if coded is not None else _case(name, quality, short_tail)
    sampling = SAMPLINGS[name]
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    monkeypatch.setenv("UHDR_HIP_HUFF_SUB_BITS", str(sub_bits))
    monkeypatch.setenv("UHDR_HIP_HUFF_MAIN_LEVELS", str(main_levels))
    capfd.readouterr()
    before = _parallel(uhdr)
    got = uhdr.huffman_decode(_dev(scan), [c.shape[:2] for c in coefs], W, H, sampling, 0, tables=tables)
    host = [g.cpu().numpy() for g in got]
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if "paths handed to the straggler waves" in ln]
    with capfd.disabled():
        print(f"\n{name} q{quality} {sub_bits} bits, {main_levels} lockstep, {len(scan)} bytes: " + " | ".join(lines))
    assert _parallel(uhdr) == before + 1
    assert len(lines) == 1, err  # one attempt: the first one held
    m = re.search(r"subsequences of (\d+) bits .*\((\d+) in lockstep, (\d+) paths handed to the straggler waves\), true path (\w+)", lines[0])
    assert m, lines[0]
    assert (int(m.group(1)), int(m.group(2))) == (sub_bits, main_levels), lines[0]
    assert m.group(4) == "resolved", lines[0]
    handed = int(m.group(3))
    assert handed > 0, "no path reached the straggler waves: the case tests nothing"
    for c in range(len(coefs)):
        assert np.array_equal(host[c], coefs[c]), (name, quality, sub_bits, c)
    return handed


@pytest.mark.parametrize("sub_bits", [512, 1024])  # one piece / four pieces with notes at the cuts
@pytest.mark.parametrize("quality", [95, 100])
@pytest.mark.parametrize("name", ["444", "420", "422", "400"])  # 3, 6, 4 and 1 blocks per MCU
def test_straggler_walk_gives_back_the_coefficients(uhdr, monkeypatch, capfd, name, quality, sub_bits):
    decode_with_stragglers(uhdr, monkeypatch, capfd, name, quality, sub_bits, 1)


def test_last_subsequence_shorter_than_a_window(uhdr, monkeypatch, capfd):
    """4:4:4, clean length 1 .. 7 bytes beyond a multiple of 64: rounds of fewer than 64 bit positions, the last of them against
    the end of the stream, and symbols that reach into the zeros beyond it."""
    decode_with_stragglers(uhdr, monkeypatch, capfd, "444", 95, 512, 1, short_tail=True)


def test_two_lockstep_levels_then_stragglers(uhdr, monkeypatch, capfd):
    """The base image's route: 4:2:0, two levels in lockstep, the stragglers' merge candidates include the in-flight slots."""
    decode_with_stragglers(uhdr, monkeypatch, capfd, "420", 95, 512, 2)
