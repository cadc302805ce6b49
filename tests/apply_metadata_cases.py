"""Gain-map metadata as other encoders write it, with inputs that make it matter: a plain helper module for
tests/test_apply_metadata_cases.py (CPU), the port == ref pin in tests/test_oracle_vs_ref.py and the device modules
tests/test_gpu_apply_metadata.py / tests/test_gpu_apply_metadata_coef.py.  numpy only.

libultrahdr_amd/synth.py's default_metadata has offset_sdr == offset_hdr == 1e-7, a minimum content boost of 1 and an HDR capacity of
1 .. content boost, and so has every map this project's own encoder writes.  With such values ((e + offset_sdr) * f) - offset_hdr is never
negative, never cancels, and the weight's log2(hdr_capacity_min) term is zero.  The cases here have offsets of 1/64 (ISO 21496-1
writers), offset_hdr above offset_sdr, factors below 1, values per channel, hdr_capacity_min above 1, and gamma 1 on one channel only.

The inputs: a synth base image with two bands written over its luma (R, G, B of an RGBA base) -- sixteen rows of the codes 0..31, where
the HDR value cancels or goes negative, and eight rows of the codes 248..255, which reach the output ceilings under a large content
boost -- and a gain map in which every byte value occurs in every channel (synth.make_gainmap never goes below byte 85)."""
import numpy as np

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image

Y420, Y422, Y444, RGBA = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCr444, A.UHDR_IMG_FMT_32bppRGBA8888
LINEAR, HLG, PQ = A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ

_PER_CHANNEL = dict(min_boost=(0.5, 0.8, 1.0), max_boost=(6.0, 5.0, 4.0), offset_sdr=(0.0, 1 / 64, 1 / 32), offset_hdr=(1 / 32, 0.0, 1 / 64),
                    capacity=(1.5, 6.0))
_HDR_ABOVE = dict(min_boost=0.5, max_boost=6.0, offset_sdr=1 / 64, offset_hdr=1 / 16, capacity=(1.5, 6.0))

# name -> min / max content boost, gamma, offsets (a scalar for the three channels, or one value each), (hdr_capacity_min, hdr_capacity_max)
CASES = {
    "iso": dict(min_boost=1.0, max_boost=4.0, gamma=1.0, offset_sdr=1 / 64, offset_hdr=1 / 64, capacity=(1.0, 4.0)),
    "hdr-above": dict(_HDR_ABOVE, gamma=1.0),
    "per-channel": dict(_PER_CHANNEL, gamma=1.0),
    "zero-offsets": dict(min_boost=0.25, max_boost=8.0, gamma=1.0, offset_sdr=0.0, offset_hdr=0.0, capacity=(2.0, 8.0)),
    "ceiling": dict(min_boost=1.0, max_boost=64.0, gamma=1.0, offset_sdr=1 / 64, offset_hdr=1 / 64, capacity=(1.0, 64.0)),
    "mixed-gamma": dict(_PER_CHANNEL, gamma=(1.3, 1.0, 2.2)),
    "hdr-above-gamma": dict(_HDR_ABOVE, gamma=1.571),
}
NAMES = list(CASES)
GAMMA_NAMES = [n for n in NAMES if CASES[n]["gamma"] != 1.0]           # a gamma other than 1 on some channel
NEGATIVE_NAMES = ["hdr-above", "per-channel", "mixed-gamma", "hdr-above-gamma"]  # the pre-clamp HDR value goes below zero


def _three(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def metadata(name, use_base_cg=1) -> A.GainmapMetadata:
    c = CASES[name]
    md = A.GainmapMetadata()
    for field, key in (("min_content_boost", "min_boost"), ("max_content_boost", "max_boost"), ("gamma", "gamma"), ("offset_sdr", "offset_sdr"),
                       ("offset_hdr", "offset_hdr")):
        for i, v in enumerate(_three(c[key])):
            getattr(md, field)[i] = v
    md.hdr_capacity_min, md.hdr_capacity_max = c["capacity"]
    md.use_base_cg = use_base_cg
    return md


def boosts(name):
    """The display boosts of a case: none, the capacity's upper end exactly, 3.0 (inside the capacity where it allows), the lower end
    exactly, 1.2 -- below the lower end of the 1.5.. and 2.. cases: weight 0, every factor 1 -- and 4.7.  At 3.0 the weight of a
    1.5 .. 6 capacity is exactly 0.5 however its logarithms are rounded; at 4.7 the float log2 the reference's weight is written with
    (jpegr.cpp:1682-1684) and a double log2 give weights one ulp apart, and about half the GainLUT's entries follow
    (tests/test_apply_metadata_cases.py: test_boost_4_7_tells_a_float_log2_from_a_double_one)."""
    lo, hi = CASES[name]["capacity"]
    return [A.FLT_MAX, float(np.float32(hi)), 3.0, float(np.float32(lo)), 1.2, 4.7]


BOOST_IDS = ["none", "capacity-max", "3.0", "capacity-min", "1.2", "4.7"]

DARK_ROWS, BRIGHT_ROWS = 16, 8  # rows [r, r + 16) hold the codes 0..31, rows [r + 16, r + 24) the codes 248..255


def _bands(h, w, band_row, shift=0):
    """(rows, codes): the two bands as a (24, w) uint8 array; every code of a band occurs in every row of it."""
    x = np.arange(w)[None, :] + shift
    y = np.arange(DARK_ROWS + BRIGHT_ROWS)[:, None]
    codes = np.where(y < DARK_ROWS, (x + 3 * y) % 32, 248 + (x + 3 * y) % 8).astype(np.uint8)
    assert band_row + codes.shape[0] <= h
    return slice(band_row, band_row + codes.shape[0]), codes


def base(fmt, w, h, align=64, band_row=0, noise=0.05) -> Image:
    """A synth SDR image of the format with the two bands over rows [band_row, band_row + 24) of its luma plane (chroma as synth drew
    it), or of R, G and B -- five and eleven columns apart -- of an RGBA8888 image."""
    if fmt == RGBA:
        img = synth.make_sdr_rgba8888(w, h, noise=noise, align=align)
        v = img.valid(0)
        rows, r = _bands(h, w, band_row)
        _, g = _bands(h, w, band_row, 5)
        _, b = _bands(h, w, band_row, 11)
        v[rows] = r.astype(np.uint32) | (g.astype(np.uint32) << 8) | (b.astype(np.uint32) << 16) | (np.uint32(255) << 24)
        return img
    img = synth.make_sdr_yuv420(w, h, noise=noise, align=align) if fmt == Y420 else synth.make_sdr_planar(fmt, w, h, noise=noise, align=align)
    rows, codes = _bands(h, w, band_row)
    img.valid(0)[rows] = codes
    return img


MAP_KINDS = ["y400", "rgb888", "rgba8888"]


def map_plane(w, h, ch):
    """(7 x + 37 y + 91 ch) mod 256: at 128 x 32 and beyond every byte value occurs in the plane."""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    return ((7 * x + 37 * y + 91 * ch) % 256).astype(np.uint8)


def map_planes(gm):
    """The one or three byte planes of a map made by gain_map."""
    v = gm.valid(0)
    if gm.fmt == A.UHDR_IMG_FMT_8bppYCbCr400:
        return [v]
    if gm.fmt == A.UHDR_IMG_FMT_24bppRGB888:
        return [v[:, c::3] for c in range(3)]
    return [((v >> s) & 0xFF).astype(np.uint8) for s in (0, 8, 16)]


def gain_map(kind, w, h, cg=A.UHDR_CG_BT_2100, align=64) -> Image:
    if kind == "y400":
        gm = Image(A.UHDR_IMG_FMT_8bppYCbCr400, w, h, cg, align=align)
        gm.valid(0)[:] = map_plane(w, h, 0)
    elif kind == "rgb888":
        gm = Image(A.UHDR_IMG_FMT_24bppRGB888, w, h, cg, align=align)
        v = gm.valid(0)
        for c in range(3):
            v[:, c::3] = map_plane(w, h, c)
    else:
        gm = Image(A.UHDR_IMG_FMT_32bppRGBA8888, w, h, cg, align=align)
        p = [map_plane(w, h, c).astype(np.uint32) for c in range(3)]
        gm.valid(0)[:] = p[0] | (p[1] << 8) | (p[2] << 16) | (np.uint32(255) << 24)
    return gm


def out_fmt(ct):
    return A.UHDR_IMG_FMT_64bppRGBAHalfFloat if ct == LINEAR else A.UHDR_IMG_FMT_32bppRGBA1010102


def samples(img):
    """The R, G, B samples of an applyGainMap destination as one (h, w, 3) array: half-float bit patterns or 10-bit codes."""
    v = img.valid(0)
    if img.fmt == A.UHDR_IMG_FMT_64bppRGBAHalfFloat:
        return np.stack([((v >> np.uint64(s)) & np.uint64(0xFFFF)).astype(np.uint16) for s in (0, 16, 32)], -1)
    return np.stack([((v >> s) & 0x3FF).astype(np.uint16) for s in (0, 10, 20)], -1)


HALF_CEILING = 0x5228  # floatToHalf(kMaxPixelFloatHdrLinear = 10000 / 203)

# ---- the shape of the CPU module's checks, and of the port == ref pin -------------------------------------------------------------------
CPU_SIZE, CPU_MAP_SIZE = (256, 64), (128, 32)
