"""The entry points for gain maps of another aspect ratio -- uhdr_hip_apply_gainmap_any / _any_dev and uhdr_hip_resize_image / _dev --
through every layer that names them, without a GPU: exported by the library, declared in include/uhdr_hip.h (the _any pair with its
siblings' parameter lists), bound in capi.py, mirrored by the Python and the C++ class."""
import os
import re
import subprocess

import pytest

from libultrahdr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# new entry point -> the sibling whose parameter list it takes (None: a parameter list of its own)
NEW = {"uhdr_hip_apply_gainmap_any": "uhdr_hip_apply_gainmap",
       "uhdr_hip_apply_gainmap_any_dev": "uhdr_hip_apply_gainmap_dev",
       "uhdr_hip_resize_image": None,
       "uhdr_hip_resize_image_dev": None}
OWN = {"uhdr_hip_resize_image": ["uhdr_hip_ctx_t* ctx", "const uhdr_raw_image_t* src", "uhdr_raw_image_t* dst"],
       "uhdr_hip_resize_image_dev": ["uhdr_hip_ctx_t* ctx", "const uhdr_raw_image_t* src", "uhdr_raw_image_t* dst", "unsigned int y0",
                                     "unsigned int full_height"]}


def _header():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """The parameter list of a declaration in uhdr_hip.h, whitespace normalised."""
    m = re.search(r"uhdr_error_info_t\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in uhdr_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_the_entry_points_are_exported():
    A.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


@pytest.mark.parametrize("name", sorted(NEW))
def test_each_is_declared(name):
    if NEW[name]:
        assert _params(name) == _params(NEW[name])
    else:
        assert _params(name) == OWN[name]


def test_the_declarations_cite_the_reference():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    assert "jpegr.cpp:1651-1671" in src and "editorhelper.cpp:88-146" in src


@pytest.mark.parametrize("name", sorted(NEW))
def test_each_is_bound_in_capi(name):
    lib = A.load()
    assert name in A.ABI_SYMBOLS
    fn = getattr(lib, name)
    assert fn.restype is A.ErrorInfo
    if NEW[name]:
        assert list(fn.argtypes) == list(getattr(lib, NEW[name]).argtypes)
    else:
        assert len(fn.argtypes) == len(OWN[name]) and fn.argtypes[0] is A.C.c_void_p
        assert all(t is A.C.c_uint for t in fn.argtypes[3:])
    # without a device it fails loudly on a null context instead of computing anything on the CPU
    args = [None] * len(fn.argtypes)
    for i, t in enumerate(fn.argtypes):
        if t in (A.C.c_int, A.C.c_uint, A.C.c_size_t, A.C.c_float):
            args[i] = 0
    st = fn(*args)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM


def test_the_entry_points_are_mirrored_in_python_and_cpp():
    from libultrahdr_amd.ultrahdr import UltraHdr

    assert callable(UltraHdr.applyGainMapAny) and callable(UltraHdr.resizeImage)
    py = open(os.path.join(ROOT, "libultrahdr_amd", "ultrahdr.py")).read()
    hpp = open(os.path.join(ROOT, "include", "uhdr_hip.hpp")).read()
    for name in ("uhdr_hip_apply_gainmap_any", "uhdr_hip_apply_gainmap_any_dev", "uhdr_hip_resize_image", "uhdr_hip_resize_image_dev"):
        assert name in py, name
    for name in ("uhdr_hip_apply_gainmap_any", "uhdr_hip_resize_image"):
        assert name in hpp, name
    assert re.search(r"uhdr_error_info_t\s+applyGainMapAny\s*\(", hpp) and re.search(r"uhdr_error_info_t\s+resizeImage\s*\(", hpp)
