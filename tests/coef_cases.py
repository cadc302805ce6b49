"""Coefficient planes for the tests of the operators that take an image in JPEG coefficient form (test_gpu_coef422.py,
test_gpu_coef444.py, test_gpu_coef_tile_trips.py): libjpeg's block grids and the two generators."""
import numpy as np

from oracle import loader as L

S420, S422, S444 = [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 1)] * 3


def grids(w, h, sampling):
    """[(blocks_w, blocks_h)] per component: libjpeg's width_in_blocks / height_in_blocks."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8) for hs, vs in sampling]


def quality_tables(quality):
    """Three different quantization tables: luma, chroma, and a coarser chroma."""
    return [L.quant_table_port(quality, False), L.quant_table_port(quality, True), L.quant_table_port(max(quality - 10, 1), True)]


def smooth_coefs(dims, qts, rng):
    """tests/test_gpu_parity.py::_coef_case's planes: a smooth field + noise, so that the decoded image is not just clipped garbage."""
    coefs = []
    for c, (bw, bh) in enumerate(dims):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8]
        pl = 128 + 90 * np.sin(xx / (13.0 + 5 * c)) * np.cos(yy / (9.0 + 3 * c)) + rng.normal(0, 12, (bh * 8, bw * 8))
        coefs.append(L.fdct_quant_port(np.ascontiguousarray(np.clip(pl, 0, 255).astype(np.uint8)), bw * 8, bw, bh, qts[c]))
    return coefs


def wild_coefs(dims, rng):
    """The full int16 range (with all-255 tables: the 32-bit multiply path and the modulo-1024 range limit)."""
    return [rng.integers(-32768, 32768, (bh, bw, 64), dtype=np.int16) for bw, bh in dims]
