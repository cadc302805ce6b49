"""The Huffman encoder's block walk (libultrahdr_amd/csrc/huffman_encode.hip: walk_block, shared by the one-walk kernel, the two-pass /
large-class kernel and the restart-interval kernel) stages every row in zig-zag order and runs software-pipelined, two stages deep: the
coefficient of the term after next and the code of the next term are in flight while the current term is coded.  The cases here are the
ones at which such a pipeline goes wrong -- blocks with fewer terms than the pipeline is deep, terms at the ends of the row, runs around
the ZRL thresholds, values at every size boundary, refused values in the prologue's and the epilogue's terms -- each compared byte for
byte with the oracle's sequential restatement of jchuff.c, on all three kernels:
  one_walk   the default route of a marker-less scan;
  two_pass   a context created with UHDR_HIP_HUFF_TWO_PASS=1;
  restart    the same coefficients with a restart interval (RESTART_MCUS per sampling).
The cases themselves are checked on the CPU (no `gpu` mark), and so is the zig-zag order the kernels compile in."""
import functools
import os
import subprocess

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from oracle import loader as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S420, S444, S1 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3, [(1, 1)]
ROUTES = ["one_walk", "two_pass", "restart"]
RESTART_MCUS = {1: 5, 3: 4, 6: 3}  # by blocks per MCU: 5, 12 and 18 blocks per interval, several intervals per wavefront
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
          50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
ALL63 = tuple(range(1, 64))
# zig-zag positions of a block's AC terms: 0, 1, 2, 3, 4 and 63 terms, cycling
POSITION_SETS = [(), (1,), (1, 2), (1, 2, 3), (1, 2, 3, 4), ALL63,
                 (), (63,), (1, 63), (2, 33, 63), (1, 17, 33, 49), ALL63,
                 (), (62,), (62, 63), (61, 62, 63), (3, 19, 35, 51), ALL63]
RUNS = [0, 14, 15, 16, 17, 31, 32, 33, 47, 48, 61]
BOUNDARY_VALUES = sorted({s * v for n in range(1, 11) for v in (1 << (n - 1), (1 << n) - 1) for s in (1, -1)})  # +-1, +-2, +-3, +-4, ... +-512, +-1023


def _bpm(sampling):
    return 1 if len(sampling) == 1 else sum(hs * vs for hs, vs in sampling)


def _shapes(w, h, sampling):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    out = []
    for hs, vs in sampling:
        cw, chh = -(-w * hs // hmax), -(-h * vs // vmax)
        out.append((-(-chh // 8), -(-cw // 8)))
    return out


def _mcus(w, h, sampling):
    hmax, vmax = (1, 1) if len(sampling) == 1 else (max(s[0] for s in sampling), max(s[1] for s in sampling))
    return -(-w // (8 * hmax)) * -(-h // (8 * vmax))


def _row_scan(blocks):
    """A single-component scan, one row of blocks: blocks = [(dc, {zig-zag position: value})] -> (coefs, w, h, sampling)."""
    a = np.zeros((1, len(blocks), 64), dtype=np.int16)
    for i, (dc, terms) in enumerate(blocks):
        a[0, i, 0] = dc
        for k, v in terms.items():
            assert 1 <= k <= 63 and v != 0
            a[0, i, ZIGZAG[k]] = v
    return [a], 8 * len(blocks), 8, S1


def _terms_of(block):
    """[(run, value)] of a natural-order block's AC terms in zig-zag order, and the trailing zero count."""
    out, run = [], 0
    for k in range(1, 64):
        v = int(block[ZIGZAG[k]])
        if v == 0:
            run += 1
        else:
            out.append((run, v))
            run = 0
    return out, run


@functools.lru_cache(maxsize=None)
def _depth_case():
    rng = np.random.default_rng(41)
    blocks = []
    for i in range(65):
        ps = POSITION_SETS[i % len(POSITION_SETS)]
        vals = rng.integers(1, 1024, len(ps)) * rng.choice([-1, 1], len(ps))
        blocks.append((int(rng.integers(-1000, 1000)), {k: int(v) for k, v in zip(ps, vals)}))
    return _row_scan(blocks)


@functools.lru_cache(maxsize=None)
def _runs_case():
    """Per run R: R zeros in front of the first term; R zeros between two terms; R zeros in front of the last of three terms."""
    rng = np.random.default_rng(43)
    v = lambda: int(rng.integers(1, 1024) * rng.choice([-1, 1]))
    blocks = []
    for r in RUNS:
        blocks.append((v(), {r + 1: v(), **({r + 2: v()} if r + 2 <= 63 else {})}))
        blocks.append((v(), {1: v(), r + 2: v()}))
        blocks.append((v(), {1: v(), 2: v(), r + 3: v()} if r + 3 <= 63 else {1: v(), r + 2: v()}))
    return _row_scan(blocks)


@functools.lru_cache(maxsize=None)
def _values_case():
    """Every boundary value as the first, a middle and the last term of a block (runs 0, 3 and 20), and as a block's only term; the DC
    values give differences of 0, +-1 and +-2047."""
    blocks = []
    dcs = [0, 0, 1, 0, -1, 0, -1024, 1023, -1024, -1024]
    for i, b in enumerate(BOUNDARY_VALUES):
        o = BOUNDARY_VALUES[(i * 7 + 3) % len(BOUNDARY_VALUES)]
        blocks.append((dcs[(2 * i) % len(dcs)], {1: b, 5: o, 26: -b, 63: o}))
        blocks.append((dcs[(2 * i + 1) % len(dcs)], {1 + i % 63: b}))
    return _row_scan(blocks)


def _refusal_cases():
    """(name, coefs, w, h, sampling): one value outside the baseline range each -- an AC term of +-1024 as the first, the last and the only
    term of a block, and in blocks of two terms (the prologue reads a clamped position there); a DC difference of +-2048.  The block sits
    behind the first segment's end (block 64 of 65) or inside it (block 11); neither starts a restart interval of RESTART_MCUS[1] blocks."""
    out = []
    for sign in (1, -1):
        bad = 1024 * sign
        shapes = {"first": {1: bad, 2: 5, 9: -3, 40: 7}, "last": {1: 5, 2: -3, 9: 7, 40: bad}, "last63": {3: 5, 62: -3, 63: bad}, "only": {17: bad},
                  "only63": {63: bad}, "two_first": {4: bad, 30: 2}, "two_second": {4: 2, 30: bad}}
        for where, terms in shapes.items():
            for at in (11, 64):
                coefs, w, h, s = _depth_case()
                a = coefs[0].copy()
                a[0, at, 1:] = 0
                for k, v in terms.items():
                    a[0, at, ZIGZAG[k]] = v
                out.append((f"ac{bad}_{where}_block{at}", [a], w, h, s))
        for at in (11, 64):
            coefs, w, h, s = _depth_case()
            a = coefs[0].copy()
            a[0, at - 1, 0], a[0, at, 0] = -1024 * sign, 1024 * sign  # (a DC term of 1024 is no baseline value either; the difference is what is coded)
            out.append((f"dc{2048 * sign}_block{at}", [a], w, h, s))
    return out


def _random_coefs(rng, w, h, sampling, kind):
    coefs = []
    for bh, bw in _shapes(w, h, sampling):
        if kind == "sparse":
            a = (rng.normal(0, 25, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.12)).astype(np.int16)
            a[..., 0] = rng.integers(-1000, 1000, (bh, bw))
            a[..., 63] = np.where(rng.random((bh, bw)) < 0.3, 1, a[..., 63])
        else:  # "dense": every term non-zero, all size categories
            a = rng.integers(-1023, 1024, (bh, bw, 64)).astype(np.int16)
            a[a == 0] = 1
        coefs.append(np.ascontiguousarray(a))
    return coefs


def _dense_block_case(pos):
    """Single component, 4 * 63 + 1 blocks = 5 segments (4k + 1: the second workgroup of four waves has one live wave): every block empty
    but the one at wave position `pos` of each segment, which holds 63 terms.  Wave position p of segment s is block 63 s + p - 1; position 0
    is the lane that carries the block in front of the segment (only its DC term is read): dense in front of segments 1 and 3 there."""
    nblocks = 63 * 4 + 1
    rng = np.random.default_rng(47 + pos)
    blocks = [(int(rng.integers(-50, 50)), {}) for _ in range(nblocks)]
    for s in ((1, 3) if pos == 0 else range(5)):
        i = 63 * s + pos - 1
        if 0 <= i < nblocks:
            blocks[i] = (blocks[i][0], {k: int(v) for k, v in zip(ALL63, rng.integers(1, 1024, 63) * rng.choice([-1, 1], 63))})
    return _row_scan(blocks)


LAYOUTS = [(24, 24, S420), (40, 24, S420), (8, 8, S444)]  # 4:2:0 edge MCUs with dummy blocks; one MCU, three lanes busy
RANDOM_SIZES = [(200, 40), (333, 77)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------

def test_the_compiled_in_zigzag_order_is_the_librarys_table(tmp_path):
    """huff_zigzag.h (what the kernels stage rows by) against host::jpeg_zigzag_to_natural() (what the library uploads), in a host-only
    program over the library's own sources; and both against the order this file builds its cases with."""
    src = tmp_path / "zigzag.cpp"
    src.write_text('#include "host_tables.h"\n#include "huff_zigzag.h"\n#include <cstdio>\n'
                   "int main() {\n  const uint8_t* t = uhdr::host::jpeg_zigzag_to_natural();\n"
                   '  for (int k = 0; k < 64; k++) printf("%d %d\\n", (int)uhdr::kHuffZigzag[k], (int)t[k]);\n  return 0;\n}\n')
    exe = tmp_path / "zigzag"
    csrc = os.path.join(ROOT, "libultrahdr_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-x", "hip", str(src),
                    os.path.join(csrc, "host_tables.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60)
    pairs = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(pairs) == 64
    assert [p[0] for p in pairs] == [p[1] for p in pairs] == ZIGZAG
    assert sorted(ZIGZAG) == list(range(64))


def test_the_depth_case_holds_the_term_counts_and_position_sets_it_claims():
    coefs, w, h, s = _depth_case()
    a = coefs[0][0]
    assert a.shape == (65, 64) and _mcus(w, h, s) == 65  # 63 blocks per segment: two segments, the second one led by block 62's lane
    counts = [len(_terms_of(b)[0]) for b in a]
    assert counts == [[0, 1, 2, 3, 4, 63][i % 6] for i in range(65)]
    sets = {tuple(k for k in range(1, 64) if b[ZIGZAG[k]] != 0) for b in a}
    for want in [(1,), (63,), (62,), (1, 2), (1, 63), (62, 63)]:
        assert want in sets, want
    assert (np.abs(a[:, 1:].astype(int)) <= 1023).all()


def test_the_runs_case_holds_every_run_in_every_place():
    coefs, _, _, _ = _runs_case()
    front, between, before_last = set(), set(), set()
    for b in coefs[0][0]:
        terms, _trail = _terms_of(b)
        front.add(terms[0][0])
        if len(terms) >= 2:
            between.add(terms[1][0])
            before_last.add(terms[-1][0])
        if len(terms) >= 3:
            before_last.add(terms[-1][0])
    assert front >= set(RUNS) and between >= set(RUNS) and before_last >= set(RUNS)
    three = {_terms_of(b)[0][-1][0] for b in coefs[0][0] if len(_terms_of(b)[0]) == 3}
    assert three >= set(RUNS) - {61}  # (61 zeros fit between two terms only)


def test_the_values_case_holds_both_signs_at_every_size_boundary():
    coefs, _, _, _ = _values_case()
    a = coefs[0][0].astype(int)
    assert BOUNDARY_VALUES[:3] == [-1023, -512, -511] and {1, -1, 2, -2, 3, -3, 4, -4, 511, -511, 512, -512, 1023, -1023} <= set(BOUNDARY_VALUES)
    for b in BOUNDARY_VALUES:
        first = sum(1 for blk in a if _terms_of(blk)[0][0][1] == b)
        last = sum(1 for blk in a if _terms_of(blk)[0][-1][1] == b)
        only = sum(1 for blk in a if [t[1] for t in _terms_of(blk)[0]] == [b])
        assert first >= 1 and last >= 1 and only >= 1, b
    sizes = {int(abs(v)).bit_length() for v in a[:, 1:].ravel() if v}
    assert sizes == set(range(1, 11))
    diffs = set(np.diff(np.concatenate([[0], a[:, 0]])).tolist())
    assert {0, 1, -1, 2047, -2047} <= diffs and max(abs(d) for d in diffs) <= 2047


def test_the_refusal_cases_hold_one_value_outside_the_range_each():
    cases = _refusal_cases()
    assert len(cases) == 2 * (7 * 2 + 2)
    for name, coefs, w, h, s in cases:
        a = coefs[0][0].astype(int)
        big_ac = np.argwhere(np.abs(a[:, 1:]) > 1023)
        diffs = np.diff(np.concatenate([[0], a[:, 0]]))
        big_dc = np.flatnonzero(np.abs(diffs) > 2047)
        if name.startswith("ac"):
            assert len(big_ac) == 1 and len(big_dc) == 0 and abs(a[big_ac[0][0], 1 + big_ac[0][1]]) == 1024, name
            terms = [t[1] for t in _terms_of(coefs[0][0][big_ac[0][0]])[0]]
            where = name.split("_", 1)[1].rsplit("_", 1)[0]
            want = {"first": (4, 0), "last": (4, 3), "last63": (3, 2), "only": (1, 0), "only63": (1, 0), "two_first": (2, 0), "two_second": (2, 1)}[where]
            assert (len(terms), [abs(t) for t in terms].index(1024)) == want, name
        else:
            assert len(big_ac) == 0 and len(big_dc) == 1 and abs(diffs[big_dc[0]]) == 2048, name


def test_the_layout_cases_are_what_they_claim():
    for w, h, s in LAYOUTS[:2]:
        (bh, bw), (ch, cw) = _shapes(w, h, s)[0], _shapes(w, h, s)[1]
        assert bw % 2 == 1 and (bw + 1) // 2 == cw  # an odd luma block width: the right column of MCUs holds dummy blocks
    assert _mcus(*LAYOUTS[2]) == 1
    for pos in (0, 1, 62, 63):
        coefs, w, h, s = _dense_block_case(pos)
        nseg = -(-_mcus(w, h, s) // 63)
        assert nseg % 4 == 1 and nseg > 1
        dense = [i for i, b in enumerate(coefs[0][0]) if len(_terms_of(b)[0]) == 63]
        empty = [i for i, b in enumerate(coefs[0][0]) if len(_terms_of(b)[0]) == 0]
        assert len(dense) + len(empty) == coefs[0].shape[1]
        assert dense == [63 * s_ + pos - 1 for s_ in ((1, 3) if pos == 0 else range(5)) if 63 * s_ + pos - 1 < coefs[0].shape[1]], pos


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def routes(hip_ctx):
    """{route: UltraHdr}: the session's context (the default route; also the restart-interval kernel's) and one created with the two-pass switch set."""
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    assert "UHDR_HIP_HUFF_TWO_PASS" not in os.environ, "the session's context must be on the default route"
    os.environ["UHDR_HIP_HUFF_TWO_PASS"] = "1"
    try:
        ctx2 = Context(0)
    finally:
        del os.environ["UHDR_HIP_HUFF_TWO_PASS"]
    u = UltraHdr(ctx=hip_ctx)
    yield {"one_walk": u, "two_pass": UltraHdr(ctx=ctx2), "restart": u}
    ctx2.close()
    # The many small scans of this module leave torch's caching allocator full of small free blocks.  Give them back (tensors that only
    # wait for the garbage collector included): a module that runs behind this one (test_gpu_huffman_jblock_write.py::
    # test_three_separate_allocations) asserts where torch places its tensors, which depends on the free blocks it finds.
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


def _ri(route, sampling):
    return RESTART_MCUS[_bpm(sampling)] if route == "restart" else 0


@functools.lru_cache(maxsize=None)
def _want(key, ri):
    coefs, w, h, s = _CASES[key]()
    return L.huffman_encode_port(coefs, w, h, s, ri)


_CASES = {"depth": _depth_case, "runs": _runs_case, "values": _values_case,
          **{f"dense{p}": functools.partial(_dense_block_case, p) for p in (0, 1, 62, 63)}}


def _encode(u, coefs, w, h, sampling, ri):
    import torch

    return u.huffman_encode([torch.from_numpy(c).to("cuda:0") for c in coefs], w, h, sampling, ri).cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", sorted(_CASES))
def test_enumerated_cases_equal_the_oracle(routes, route, case):
    coefs, w, h, s = _CASES[case]()
    ri = _ri(route, s)
    got = _encode(routes[route], coefs, w, h, s, ri)
    want = _want(case, ri)
    assert len(got) == len(want), (route, case, len(got), len(want))
    assert got == want, (route, case)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_refused_values_in_every_place_of_the_pipeline(routes, route):
    good, w, h, s = _depth_case()
    ri = _ri(route, s)
    for name, coefs, w, h, s in _refusal_cases():
        with pytest.raises(A.UhdrError) as e:
            _encode(routes[route], coefs, w, h, s, ri)
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM, (route, name)
    assert _encode(routes[route], good, w, h, s, ri) == _want("depth", ri)  # ... and the context codes a valid scan as before


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_refused_values_in_a_three_component_scan(routes, route):
    rng = np.random.default_rng(53)
    w, h, s = 40, 24, S420
    ri = _ri(route, s)
    for comp, val in ((0, 1024), (1, -1024), (2, 1024)):
        coefs = _random_coefs(rng, w, h, s, "sparse")
        c = coefs[comp]
        c[-1, -1, 1:] = 0
        c[-1, -1, ZIGZAG[63]] = val  # the only term of the scan's last real block of that component, at the row's end
        with pytest.raises(A.UhdrError) as e:
            _encode(routes[route], coefs, w, h, s, ri)
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM, (route, comp)
    good = _random_coefs(rng, w, h, s, "sparse")
    assert _encode(routes[route], good, w, h, s, ri) == L.huffman_encode_port(good, w, h, s, ri)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_layouts_with_dummy_blocks_and_single_mcus_equal_the_oracle(routes, route):
    rng = np.random.default_rng(59)
    for w, h, s in LAYOUTS:
        for kind in ("sparse", "dense"):
            coefs = _random_coefs(rng, w, h, s, kind)
            ri = _ri(route, s)
            assert _encode(routes[route], coefs, w, h, s, ri) == L.huffman_encode_port(coefs, w, h, s, ri), (route, w, h, kind)


@functools.lru_cache(maxsize=None)
def _random_case(w, h, nsamp, kind, ri):
    s = {1: S1, 3: S444, 6: S420}[nsamp]
    coefs = _random_coefs(np.random.default_rng(61 + w + nsamp), w, h, s, kind)
    return coefs, s, L.huffman_encode_port(coefs, w, h, s, ri)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_random_scans_equal_the_oracle(routes, route, kind):
    for w, h in RANDOM_SIZES:
        for nsamp in (1, 3, 6):
            ri = RESTART_MCUS[nsamp] if route == "restart" else 0
            coefs, s, want = _random_case(w, h, nsamp, kind, ri)
            got = _encode(routes[route], coefs, w, h, s, ri)
            assert len(got) == len(want), (route, kind, w, h, nsamp, len(got), len(want))
            assert got == want, (route, kind, w, h, nsamp)
