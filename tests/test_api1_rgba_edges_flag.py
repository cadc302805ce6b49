"""CPU: UHDR_HIP_ENCODE_RGBA_EDGES -- the Python mirror and the header agree on the value, the flag stays clear of the bits that must remain
unknown, and the header comment of the three entry points that take it names it."""
import os
import re

from libultrahdr_amd import capi as A

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "uhdr_hip.h")
ENTRY_POINTS = ["uhdr_hip_encode_api1_fused_edges_dev", "uhdr_hip_encode_api1_scans_edges", "uhdr_hip_encode_api1_scans_edges_dev"]


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_mirror_and_the_header_define_the_same_flag():
    assert A.UHDR_HIP_ENCODE_RGBA_EDGES == 0x4
    m = re.findall(r"^#define\s+UHDR_HIP_ENCODE_RGBA_EDGES\s+(\S+)\s*$", _header(), re.M)
    assert len(m) == 1 and int(m[0].rstrip("uU"), 0) == A.UHDR_HIP_ENCODE_RGBA_EDGES
    assert A.UHDR_HIP_ENCODE_RGBA_EDGES & A.UHDR_HIP_GENERATE_GAMMA_TABLE == 0
    assert A.UHDR_HIP_ENCODE_RGBA_EDGES & (0x2 | 0x10) == 0  # (bits the entry points keep answering INVALID_PARAM for)


def test_the_header_comment_of_the_three_entry_points_names_the_flag():
    text = _header()
    first = min(text.index("uhdr_error_info_t " + name + "(") for name in ENTRY_POINTS)
    comment_start = text.rindex("/*", 0, first)
    comment = text[comment_start:first]
    assert "UHDR_HIP_ENCODE_RGBA_EDGES" in comment and "UHDR_IMG_FMT_32bppRGBA8888" in comment
    # the three prototypes follow that comment back to back: nothing else is declared between them
    last = max(text.index("uhdr_error_info_t " + name + "(") for name in ENTRY_POINTS)
    between = text[first:last]
    assert between.count("uhdr_error_info_t uhdr_hip_") == 2 and "/*" not in between
