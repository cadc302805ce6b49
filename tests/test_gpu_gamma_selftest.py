"""GPU: the two device sweeps behind UHDR_HIP_GENERATE_GAMMA_TABLE (uhdr_hip_selftest 6 and 7, csrc/selftest.hip).

which 6: for a gamma and a form, the code gamma_code (csrc/gamma_code.h) gives EVERY float from eight ulps below zero to eight ulps past
the last threshold lies between its thresholds, T[code] <= v < T[code + 1] -- about 1.07e9 floats, a second each.  The thresholds
themselves are held to the reference's expressions on the CPU (tests/test_gamma_code_table.py); this is the device's search over them.
which 7: the ratio -> byte table minmax_table_kernel builds from a gamma's two-pass thresholds against the per-sample evaluation that ends
in the search, over the table's whole domain and 2^20 bit patterns beyond either end, for ranges the 256 x 128 parity images do not have.
Zero violations are required everywhere.  Measured on an MI355X: which 6, 0 violations over 1 065 287 504 to 1 065 353 234 floats in each
of the five cases; which 7, 0 mismatches in each of the fifteen ranges (2.1e6 to 2.5e8 ratios, 641 to 1003 table entries); every case
prints its counts."""
import ctypes as C

import numpy as np
import pytest

from libultrahdr_amd import capi as A

pytestmark = pytest.mark.gpu


def _run(hip_ctx, which, arg0=0, arg1=0, seed=1, mm=None):
    out = (C.c_ulonglong * 8)()
    mmv = (C.c_float * 6)(*(mm if mm is not None else [0.0] * 6))
    A.check(hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, which, arg0, arg1, seed, mmv, out))
    return [int(v) for v in out]


def _bits(gamma):
    return int(np.float32(gamma).view(np.uint32))


def _last_threshold_bits(gamma, form):
    thr = np.zeros(256, dtype=np.float32)
    info = (C.c_uint32 * 4)()
    assert A.load().uhdr_hip_gamma_code_eval(C.c_float(gamma), form, None, None, 0, info, thr.ctypes.data) == 0
    return int(thr[255:256].view(np.uint32)[0])


# gamma 4.0: an even integer, whose negative arguments take the byte of their magnitude (the sign bit of T[0])
@pytest.mark.parametrize("gamma,form", [(1.571, 0), (1.571, 1), (0.5, 1), (4.0, 1), (4.0, 0)])
def test_every_float_lies_between_the_thresholds_of_its_code(hip_ctx, gamma, form):
    bad, n, searched, no_table = _run(hip_ctx, 6, form, 0, 1, [gamma, 0, 0, 0, 0, 0])[:4]
    print(f"gamma {gamma} form {form}: {bad} violations over {n} floats")
    assert no_table == 0
    assert n == _last_threshold_bits(gamma, form) + 8 + 1 + 9 and searched == n  # 0 .. last + 8, and -0 with the eight floats below it
    assert bad == 0


@pytest.mark.parametrize("gamma", [0.0, -1.0, float("nan")])
def test_a_gamma_without_thresholds_is_flagged(hip_ctx, gamma):
    o = _run(hip_ctx, 6, 1, 0, 1, [gamma, 0, 0, 0, 0, 0])
    assert o[3] == 1 and o[0] == 0 and o[1] == 0
    assert _run(hip_ctx, 7, 0, 1, _bits(gamma), [0.0, 0, 0, 2.0, 0, 0])[3] == 1


def test_bad_sweep_arguments_are_refused(hip_ctx):
    out = (C.c_ulonglong * 8)()
    mm = (C.c_float * 6)(1.571, 0, 0, 0, 0, 0)
    assert hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, 6, 2, 0, 1, mm, out).error_code == A.UHDR_CODEC_INVALID_PARAM  # no such form
    assert hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, 7, 3, 3, _bits(1.571), mm, out).error_code == A.UHDR_CODEC_INVALID_PARAM
    assert hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, 8, 0, 0, 1, mm, out).error_code == A.UHDR_CODEC_INVALID_PARAM


# at gamma 1.571 the byte thresholds are 1 / (1.571 x 255) apart at their closest: 607 / range buckets per binade, rounded up to a power
# of two, times the range must fit 1024 entries -- ranges up to 4 binades (256 per binade), 4.74 .. 8 (128), 9.5 .. 16 (64), 19 .. 29.9 (32)
TABLED = [
    [-2.0, -1.5, -1.0, 4.0, 5.0, 6.0],          # ordinary content: 6, 6.5 and 7 binades
    [-1.0, -0.5, 0.0, 2.5, 3.0, 3.8],           # 3.5 to 3.8 binades, 256 buckets per binade
    [-14.3, -14.3, -14.3, 15.6, 15.6, 15.6],    # the clamp's whole range
    [-0.3333, 0.25, 1.0, 0.5667, 2.15, 1.0035], # narrow ranges: 0.9, 1.9 and 0.0035 binades (1024, 512 and 2^18 buckets per binade)
    [-0.3219281, -3.0, 0.5, 2.5849626, 10.0, 16.0],  # the hint case 0.8 .. 6.0, and 13 and 15.5 binades
]


@pytest.mark.parametrize("mm", TABLED)
def test_the_table_built_from_the_thresholds_equals_the_per_sample_search(hip_ctx, mm):
    for ch in range(3):
        bad, n, entries, no_table = _run(hip_ctx, 7, ch, 3, _bits(1.571), mm)[:4]
        print(f"range {mm[ch]} .. {mm[3 + ch]}: {bad} mismatches over {n} ratios, {entries} entries")
        assert no_table == 0, f"channel {ch}: no table"
        assert 0 < entries <= 1024 and n > 2 ** 21 and bad == 0, (ch, bad, n, entries)


@pytest.mark.parametrize("gamma,mm", [
    (1.571, [1.0, 0, 0, 1.0 + 1e-4, 0, 0]),   # too dense for any bucket width
    (1.571, [-2.0, 0, 0, 2.5, 0, 0]),         # 4.5 binades: between two bucket widths (128 per binade too wide, 256 too many)
    (0.5, [-2.0, 0, 0, 4.0, 0, 0]),           # thresholds 2 / 255^2 apart at the dark end: no range fits
    (4.0, [-2.0, 0, 0, 4.0, 0, 0]),           # an even integer: the byte is not saturated below the range
    (2.0, [-2.0, 0, 0, 4.0, 0, 0]),
])
def test_a_declined_table_is_flagged(hip_ctx, gamma, mm):
    o = _run(hip_ctx, 7, 0, 1, _bits(gamma), mm)
    assert o[3] == 1 and o[0] == 0
