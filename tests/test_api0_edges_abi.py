"""The two entry points of the fused API-0 encode for frames that are not whole MCUs and maps that are not whole blocks through every
layer that names them, without a GPU: exported by the library, declared in include/uhdr_hip.h with uhdr_hip_encode_api0_scans_scaled's
parameter list, bound in capi.py with its argtypes, mirrored by the Python and the C++ class."""
import os
import re
import subprocess

from libultrahdr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLING = "uhdr_hip_encode_api0_scans_scaled"
MIRRORS = {"uhdr_hip_encode_api0_scans_edges": "encodeApi0ScansEdges", "uhdr_hip_encode_api0_scans_edges_dev": "encodeApi0ScansEdgesDev"}


def _header():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """The parameter list of a declaration in uhdr_hip.h, whitespace normalised."""
    m = re.search(r"uhdr_error_info_t\s+" + name + r"\s*\((.*?)\)\s*;", _header()[1], flags=re.S)
    assert m, f"{name} is not declared in uhdr_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_both_entry_points_are_exported():
    A.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(MIRRORS) <= exported, sorted(set(MIRRORS) - exported)


def test_both_entry_points_are_declared_with_the_scaled_siblings_parameters():
    assert len(_params(SIBLING)) == 14
    for name in MIRRORS:
        assert _params(name) == _params(SIBLING), name
    # the header says which code of the reference this is: the API-0 encode and the helper's edge handling
    raw = _header()[0]
    decl = raw[raw.index("uhdr_hip_encode_api0_scans_scaled("):raw.index("uhdr_hip_encode_api0_scans_edges(")]
    assert "jpegr.cpp:179-244" in decl and "jpegencoderhelper.cpp:246-309" in decl


def test_both_entry_points_are_bound_in_capi_with_the_scaled_siblings_argtypes():
    lib = A.load()
    sib = getattr(lib, SIBLING)
    for name in MIRRORS:
        assert name in A.ABI_SYMBOLS and getattr(lib, name) is not None
        new = getattr(lib, name)
        assert new.restype is sib.restype is A.ErrorInfo and list(new.argtypes) == list(sib.argtypes), name
        # without a device each fails loudly on a null context instead of computing anything on the CPU
        st = new(None, None, None, None, None, None, None, None, None, 0, None, None, 0, None)
        assert st.error_code == A.UHDR_CODEC_INVALID_PARAM


def test_both_entry_points_are_mirrored_in_python_and_cpp():
    from libultrahdr_amd.ultrahdr import UltraHdr

    py = open(os.path.join(ROOT, "libultrahdr_amd", "ultrahdr.py")).read()
    hpp = open(os.path.join(ROOT, "include", "uhdr_hip.hpp")).read()
    for name, method in MIRRORS.items():
        assert callable(getattr(UltraHdr, method)), method
        assert name in py and name in hpp, name
        assert re.search(r"uhdr_error_info_t\s+" + method + r"\s*\(", hpp), method
