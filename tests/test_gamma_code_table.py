"""CPU: the threshold tables behind UHDR_HIP_GENERATE_GAMMA_TABLE (host_tables.cpp: gamma_code_table) and the lookup the kernels run on
them (csrc/gamma_code.h; uhdr_hip_gamma_code_eval restates it on the host) against the two byte expressions of the reference's encode side:

    form 0, one pass (encodeGain, gainmapmath.cpp:769-770):     (uint8_t)(powf(n, gamma) * 255.0f)
    form 1, two pass (affineMapGain, gainmapmath.cpp:784-789):  m = (float)pow((double)m, (double)gamma); clip(m * 255 + 0.5, 0, 255)

Form 1's direct expression is the oracle's own affine_map_gain (uo_generate_gainmap_pass2 with the range {0, 1}: (g - 0) / (1 - 0) is g
itself).  The oracle exports encodeGain only behind its log2, so form 0's direct expression is restated here from the C library's powf,
called per value, with float32 arithmetic around it; a NaN (powf of a negative) converts to byte 0, as it does in the oracle's build.
(For the even-integer gamma 4.0 pow of a negative is no NaN but the power of the magnitude; the lookup has to follow that too.)
Zero differences are required on 2^20 random floats of [0, 1], on the 16 floats around every threshold and at the ends of the domain.
Gammas that have no table must say so."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from oracle import loader as O

GAMMAS = [0.25, 0.5, 0.8, 1.3, 1.571, 1.7, 2.2, 4.0]
FORMS = [0, 1]
ONE = int(np.float32(1.0).view(np.uint32))

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def direct(x: np.ndarray, gamma: float, form: int) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    if form == 1:
        out = np.zeros(x.size, dtype=np.uint8)
        mm = (C.c_float * 6)(0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
        O.port().uo_generate_gainmap_pass2(x.ctypes.data, mm, C.c_float(gamma), 1, x.size, 1, out.ctypes.data, x.size)
        return out.astype(np.uint32)
    powf, g = _libm.powf, float(np.float32(gamma))
    ng = np.array([powf(v, g) for v in x.tolist()], dtype=np.float32)
    prod = ng * np.float32(255.0)  # float32 product
    assert not np.any(prod >= 256.0)  # the domain ends before the narrowing wraps
    return np.where(np.isnan(prod), 0, np.nan_to_num(prod, nan=0.0).astype(np.int64)).astype(np.uint32)  # truncation; NaN -> 0


def table(gamma: float, form: int):
    info = (C.c_uint32 * 4)()
    thr = np.full(256, -1.0, dtype=np.float32)
    rc = A.load().uhdr_hip_gamma_code_eval(C.c_float(gamma), form, None, None, 0, info, thr.ctypes.data)
    return rc, list(info), thr


def lookup(gamma: float, form: int, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.full(x.size, 0xFFFFFFFF, dtype=np.uint32)
    info = (C.c_uint32 * 4)()
    rc = A.load().uhdr_hip_gamma_code_eval(C.c_float(gamma), form, x.ctypes.data, out.ctypes.data, x.size, info, None)
    assert rc == 0 and info[0] == 1
    return out


@pytest.fixture(scope="module")
def random_unit():
    rng = np.random.default_rng(20261021)
    # uniform over the bit patterns of [0, 1] (every binade as dense as the next) and uniform over the interval, half each
    bits = rng.integers(0, ONE + 1, size=1 << 19, dtype=np.uint32)
    return np.concatenate([bits.view(np.float32), rng.random(1 << 19, dtype=np.float32)])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_thresholds_are_the_steps_of_the_reference_expression(gamma, form):
    rc, info, thr = table(gamma, form)
    assert rc == 0 and info[0] == 1 and info[1] == 256, "no verified table"
    assert thr[0] == 0.0 and bool(np.signbit(thr[0])) == (gamma % 2 == 0) and np.all(np.isfinite(thr)) and np.all(np.diff(thr) > 0) and thr[255] <= 1.0
    steps = thr[1:]
    assert np.array_equal(direct(steps, gamma, form), np.arange(1, 256)), "the byte at T[k] is not k"
    below = (steps.view(np.uint32) - 1).view(np.float32)
    assert np.array_equal(direct(below, gamma, form), np.arange(0, 255)), "T[k] is not the smallest float whose byte is >= k"
    assert info[3] == int(np.diff(steps.view(np.uint32).astype(np.int64)).min())  # the recorded smallest gap, in ulps
    assert info[3] > 16  # the 16 floats around a threshold below hold no second one


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_lookup_equals_the_reference_expression(gamma, form, random_unit):
    _, _, thr = table(gamma, form)
    around = (thr[1:].view(np.uint32)[:, None].astype(np.int64) + np.arange(-8, 8)[None, :]).astype(np.uint32).reshape(-1).view(np.float32)
    ends = np.concatenate([np.array([0.0, -0.0, -1e-9], dtype=np.float32),
                           np.arange(ONE - 4, ONE + 5, dtype=np.uint32).view(np.float32)])  # 1.0 +- 4 ulps
    if form == 1:
        ends = np.concatenate([ends, np.array([-3.0, 7.0], dtype=np.float32)])
    probes = np.concatenate([around, ends, random_unit])
    got = lookup(gamma, form, probes)
    want = direct(probes, gamma, form)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(probes[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    e = got[around.size:around.size + ends.size]
    assert list(e[:3]) == [0, 0, 0] and e[3 + 4] == 255 and e[3 + 8] == 255  # 0, -0, -1e-9; 1.0; 1.0 + 4 ulps
    if form == 1:
        # -3.0 and 7.0: what a min / max content-boost hint inside the content's range produces
        assert e[-2] == (255 if gamma % 2 == 0 else 0) and e[-1] == 255


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gamma", [0.0, -1.0, float("nan"), float("inf")])
def test_a_gamma_without_a_table_says_so(gamma, form):
    x = np.array([0.25], dtype=np.float32)
    out = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    thr = np.full(256, -1.0, dtype=np.float32)
    info = (C.c_uint32 * 4)()
    rc = A.load().uhdr_hip_gamma_code_eval(C.c_float(gamma), form, x.ctypes.data, out.ctypes.data, 1, info, thr.ctypes.data)
    assert rc == 1 and info[0] == 0
    assert out[0] == 0xFFFFFFFF and np.all(thr == -1.0)  # nothing was guessed


def test_an_unknown_form_is_refused():
    assert A.load().uhdr_hip_gamma_code_eval(C.c_float(1.571), 2, None, None, 0, None, None) == -1


def test_the_table_of_a_gamma_is_built_once():
    _, info_a, thr_a = table(1.571, 1)
    _, info_b, thr_b = table(1.571, 1)
    assert info_a[2] == info_b[2]  # the recorded construction time is the first call's: the second call built nothing
    assert np.array_equal(thr_a, thr_b)

