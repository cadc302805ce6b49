"""The four entry points of the API-3 encode -- generateGainMap from JPEG coefficients (two samplings) and the one-call form (host and
device data) -- through every layer that names them, without a GPU: exported by the library, declared in include/uhdr_hip.h with
matching parameter lists and the reference's line ranges, bound in capi.py, mirrored by the Python and the C++ class."""
import os
import re
import subprocess

from libultrahdr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPERATORS = ("uhdr_hip_generate_gainmap_coef_dev", "uhdr_hip_generate_gainmap_coef422_dev")
ONE_CALL = ("uhdr_hip_encode_api3_scans", "uhdr_hip_encode_api3_scans_dev")
MIRRORS = {"uhdr_hip_generate_gainmap_coef_dev": "generateGainMapFromCoefficients", "uhdr_hip_generate_gainmap_coef422_dev": "generateGainMapFromCoefficients",
           "uhdr_hip_encode_api3_scans": "encodeApi3Scans", "uhdr_hip_encode_api3_scans_dev": "encodeApi3Scans"}


def _header():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """The parameter list of a declaration in uhdr_hip.h, whitespace normalised."""
    m = re.search(r"uhdr_error_info_t\s+" + name + r"\s*\((.*?)\)\s*;", _header()[1], flags=re.S)
    assert m, f"{name} is not declared in uhdr_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_the_four_entry_points_are_exported():
    A.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(OPERATORS + ONE_CALL) <= exported, sorted(set(OPERATORS + ONE_CALL) - exported)


def test_the_four_entry_points_are_declared_in_pairs_of_identical_parameter_lists():
    assert _params(OPERATORS[0]) == _params(OPERATORS[1]) and len(_params(OPERATORS[0])) == 9
    assert _params(ONE_CALL[0]) == _params(ONE_CALL[1]) and len(_params(ONE_CALL[0])) == 13
    # the comment in front of each pair says which loops of the reference these are
    raw = _header()[0]
    for pair in (OPERATORS, ONE_CALL):
        first = min(raw.index(name + "(") for name in pair)
        comment = raw[raw.rindex("/*", 0, first):first]
        assert "jpegr.cpp:327-385" in comment and "jpegr.cpp:530-1050" in comment and "jpegdecoderhelper.cpp" in comment, pair


def test_the_four_entry_points_are_bound_in_capi():
    lib = A.load()
    for pair in (OPERATORS, ONE_CALL):
        a, b = (getattr(lib, n) for n in pair)
        assert all(n in A.ABI_SYMBOLS for n in pair)
        assert a.restype is b.restype is A.ErrorInfo and list(a.argtypes) == list(b.argtypes), pair
    # without a device each fails loudly on a null context instead of computing anything on the CPU
    for name in OPERATORS:
        st = getattr(lib, name)(None, None, 0, 0, 0, None, None, None, None)
        assert st.error_code == A.UHDR_CODEC_INVALID_PARAM, name
    for name in ONE_CALL:
        st = getattr(lib, name)(None, None, None, 0, 0, None, None, None, None, None, None, 0, None)
        assert st.error_code == A.UHDR_CODEC_INVALID_PARAM, name


def test_the_four_entry_points_are_mirrored_in_python_and_cpp():
    from libultrahdr_amd.ultrahdr import UltraHdr

    py = open(os.path.join(ROOT, "libultrahdr_amd", "ultrahdr.py")).read()
    hpp = open(os.path.join(ROOT, "include", "uhdr_hip.hpp")).read()
    for name, method in MIRRORS.items():
        assert callable(getattr(UltraHdr, method)), method
        assert name in py and name in hpp, name
        assert re.search(r"uhdr_error_info_t\s+" + method + r"\s*\(", hpp), method
