"""The two entry points of the fused API-0 encode for P010 intents through every layer that names them, without a GPU: exported
by the library, declared in include/uhdr_hip.h, bound in capi.py, mirrored by the Python and the C++ class."""
import os
import re
import subprocess

from libultrahdr_amd import capi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uhdr_hip_encode_api0_p010_fused_dev", "uhdr_hip_encode_api0_scans_any")


def _header():
    src = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _params(name):
    """The parameter list of a declaration in uhdr_hip.h, whitespace normalised."""
    m = re.search(r"uhdr_error_info_t\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in uhdr_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_both_entry_points_are_exported():
    A.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", A.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)


def test_both_entry_points_are_declared_and_scans_any_takes_its_siblings_parameters():
    assert _params("uhdr_hip_encode_api0_scans_any") == _params("uhdr_hip_encode_api0_scans")
    assert len(_params("uhdr_hip_encode_api0_scans")) == 14
    p = _params("uhdr_hip_encode_api0_p010_fused_dev")
    assert p == ["uhdr_hip_ctx_t* ctx", "const uhdr_raw_image_t* hdr", "const uhdr_hip_encode_cfg_t* cfg", "uhdr_raw_image_t* base_ycc420",
                 "uhdr_gainmap_metadata_t* metadata", "uhdr_raw_image_t* gainmap"]


def test_both_entry_points_are_bound_in_capi():
    lib = A.load()
    for name in NEW:
        assert name in A.ABI_SYMBOLS and getattr(lib, name) is not None
    any_, sib = lib.uhdr_hip_encode_api0_scans_any, lib.uhdr_hip_encode_api0_scans
    assert any_.restype is sib.restype is A.ErrorInfo and list(any_.argtypes) == list(sib.argtypes)
    fused = lib.uhdr_hip_encode_api0_p010_fused_dev
    assert fused.restype is A.ErrorInfo and len(fused.argtypes) == 6
    # without a device both fail loudly on a null context instead of computing anything on the CPU
    st = lib.uhdr_hip_encode_api0_p010_fused_dev(None, None, None, None, None, None)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM
    st = lib.uhdr_hip_encode_api0_scans_any(None, None, None, None, None, None, None, None, None, 0, None, None, 0, None)
    assert st.error_code == A.UHDR_CODEC_INVALID_PARAM


def test_both_entry_points_are_mirrored_in_python_and_cpp():
    from libultrahdr_amd.ultrahdr import UltraHdr

    assert callable(UltraHdr.encodeApi0FusedP010) and callable(UltraHdr.encodeApi0ScansAny)
    py = open(os.path.join(ROOT, "libultrahdr_amd", "ultrahdr.py")).read()
    hpp = open(os.path.join(ROOT, "include", "uhdr_hip.hpp")).read()
    for name in NEW:
        assert name in py and name in hpp, name
    assert re.search(r"uhdr_error_info_t\s+encodeApi0FusedP010\s*\(", hpp) and re.search(r"uhdr_error_info_t\s+encodeApi0ScansAny\s*\(", hpp)
