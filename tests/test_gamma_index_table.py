"""CPU: the threshold table behind UHDR_HIP_APPLY_GAMMA_TABLE (host_tables.cpp: gamma_index_table) and the lookup the kernels run on
it (uhdr_hip_gamma_index_eval restates it on the host) against GainLUT::getGainFactor's own expression (gainmapmath.h:483-489):

    gain = pow(gain, 1 / gamma)   -- the double pow, stored to a float
    idx  = int(gain * 1023 + 0.5) clipped to 0..1023

The reference expression is computed here with Python's math.pow (the C library's) and numpy float32 casts; zero differences are
required at every threshold and its predecessor, at the ends of the domain and on 2^20 random floats of [0, 1].  Gammas that have
no such table must say so."""
import ctypes as C
import math

import numpy as np
import pytest

from libultrahdr_amd import capi as A

GAMMAS = [0.25, 0.8, 1.3, 1.571, 1.7, 2.2, 4.0]


def reference_index(x: np.ndarray, gamma: float) -> np.ndarray:
    gamma_inv = float(np.float32(1.0) / np.float32(gamma))  # mGammaInv = 1.0f / gamma, a float
    if gamma_inv != 1.0:
        g = np.array([math.pow(v, gamma_inv) for v in x.astype(np.float64).tolist()], dtype=np.float64).astype(np.float32)
    else:
        g = x.astype(np.float32)
    prod = (g * np.float32(1023.0)).astype(np.float32)  # the float product, then + 0.5 in double
    idx = np.floor(prod.astype(np.float64) + 0.5).astype(np.int64)  # the argument is never negative: int() == floor()
    return np.clip(idx, 0, 1023).astype(np.uint32)


def table(gamma: float):
    lib = A.load()
    info = (C.c_uint32 * 4)()
    thr = np.zeros(1025, dtype=np.float32)
    rc = lib.uhdr_hip_gamma_index_eval(C.c_float(gamma), None, None, 0, info, thr.ctypes.data)
    return rc, list(info), thr


def lookup(gamma: float, x: np.ndarray) -> np.ndarray:
    lib = A.load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.full(x.size, 0xFFFFFFFF, dtype=np.uint32)
    info = (C.c_uint32 * 4)()
    rc = lib.uhdr_hip_gamma_index_eval(C.c_float(gamma), x.ctypes.data, out.ctypes.data, x.size, info, None)
    assert rc == 0 and info[0] == 1
    return out


@pytest.fixture(scope="module")
def random_gains():
    rng = np.random.default_rng(20261020)
    # uniform over the bit patterns of [0, 1] (every binade as dense as the next) and uniform over the interval, half each
    bits = rng.integers(0, 0x3F800000 + 1, size=1 << 19, dtype=np.uint32)
    return np.concatenate([bits.view(np.float32), rng.random(1 << 19, dtype=np.float32)])


@pytest.mark.parametrize("gamma", GAMMAS)
def test_thresholds_are_the_steps_of_the_reference_expression(gamma):
    rc, info, thr = table(gamma)
    assert rc == 0 and info[0] == 1 and info[1] == 1024
    assert thr[0] == 0.0 and np.isinf(thr[1024]) and thr[1024] > 0
    steps = thr[1:1024]
    assert np.all(np.isfinite(steps)) and np.all(steps > 0) and np.all(np.diff(thr[:1024]) >= 0)
    assert steps[-1] <= 1.0  # everything from the last threshold up has index 1023
    at = reference_index(steps, gamma)
    assert np.all(at >= np.arange(1, 1024)), "the index at T[i] is below i"
    below = (steps.view(np.uint32) - 1).view(np.float32)  # the predecessor of every threshold
    strict = np.diff(thr[:1024]) > 0  # where T[i] == T[i - 1] the predecessor belongs to an earlier step
    assert np.all(reference_index(below, gamma)[strict] < np.arange(1, 1024)[strict]), "T[i] is not the smallest float with an index >= i"


@pytest.mark.parametrize("gamma", GAMMAS)
def test_lookup_equals_the_reference_expression(gamma, random_gains):
    _, _, thr = table(gamma)
    steps = thr[1:1024]
    one = np.float32(1.0).view(np.uint32)
    ends = np.array([0, 1, one, one + 1, one + 2], dtype=np.uint32).view(np.float32)  # 0, the smallest denormal, 1.0 and the next two floats
    probes = np.concatenate([steps, (steps.view(np.uint32) - 1).view(np.float32), ends, random_gains])
    got = lookup(gamma, probes)
    want = reference_index(probes, gamma)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(probes[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert got[2 * 1023] == 0 and got[2 * 1023 + 2] == 1023 and got[2 * 1023 + 4] == 1023


@pytest.mark.parametrize("gamma", [0.0, -1.0, float("nan"), float("inf")])
def test_a_gamma_without_a_table_says_so(gamma):
    lib = A.load()
    x = np.array([0.25], dtype=np.float32)
    out = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    info = (C.c_uint32 * 4)()
    rc = lib.uhdr_hip_gamma_index_eval(C.c_float(gamma), x.ctypes.data, out.ctypes.data, 1, info, None)
    assert rc == 1 and info[0] == 0
    assert out[0] == 0xFFFFFFFF  # nothing was guessed


def test_the_table_of_a_gamma_is_built_once():
    rc, info_a, thr_a = table(1.571)
    rc, info_b, thr_b = table(1.571)
    assert info_a[2] == info_b[2]  # the recorded construction time is the first call's: the second call built nothing
    assert np.array_equal(thr_a, thr_b)
