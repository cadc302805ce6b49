"""The three entry points of the fused API-1 encode that also takes RGBA8888 SDR intents, through every layer that names them, without
a GPU: exported by the library, declared in include/uhdr_hip.h with their siblings' parameter lists, bound in capi.py with their
siblings' argtypes, mirrored by the Python and the C++ class."""
import os
import re
import subprocess

import pytest

from libultrahdr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# new entry point -> the sibling whose parameter list it takes
NEW = {"uhdr_hip_encode_api1_fused_any_dev": "uhdr_hip_encode_api1_fused_dev",
       "uhdr_hip_encode_api1_scans_any": "uhdr_hip_encode_api1_scans",
       "uhdr_hip_encode_api1_scans_any_dev": "uhdr_hip_encode_api1_scans_dev"}


def _header():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """The parameter list of a declaration in uhdr_hip.h, whitespace normalised."""
    m = re.search(r"uhdr_error_info_t\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in uhdr_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_the_three_entry_points_are_exported():
    A.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


@pytest.mark.parametrize("name", sorted(NEW))
def test_each_is_declared_with_its_siblings_parameter_list(name):
    assert _params(name) == _params(NEW[name])
    assert len(_params(name)) == (10 if "fused" in name else 15)


@pytest.mark.parametrize("name", sorted(NEW))
def test_each_is_bound_in_capi_with_its_siblings_argtypes(name):
    lib = A.load()
    assert name in A.ABI_SYMBOLS
    fn, sib = getattr(lib, name), getattr(lib, NEW[name])
    assert fn.restype is sib.restype is A.ErrorInfo and list(fn.argtypes) == list(sib.argtypes)
    # without a device it fails loudly on a null context instead of computing anything on the CPU
    args = [None] * len(fn.argtypes)
    for i, t in enumerate(fn.argtypes):
        if t in (A.C.c_int, A.C.c_size_t):
            args[i] = 0
    st = fn(*args)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM


def test_the_entry_points_are_mirrored_in_python_and_cpp():
    from libultrahdr_amd.ultrahdr import UltraHdr

    assert callable(UltraHdr.encodeApi1FusedAny) and callable(UltraHdr.encodeApi1ScansAny)
    py = open(os.path.join(ROOT, "libultrahdr_amd", "ultrahdr.py")).read()
    hpp = open(os.path.join(ROOT, "include", "uhdr_hip.hpp")).read()
    for name in NEW:
        assert name in py and name in hpp, name
    assert re.search(r"uhdr_error_info_t\s+encodeApi1FusedAny\s*\(", hpp) and re.search(r"uhdr_error_info_t\s+encodeApi1ScansAny\s*\(", hpp)
