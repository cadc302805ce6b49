"""Deterministic images made of the input codes at which the encode and apply kernels' tables end: a plain helper
module for tests/test_code_lattice.py (CPU) and tests/test_gpu_code_lattice.py (device), numpy only.

libultrahdr_amd/synth.py draws a smooth field; on it no sample reaches the ends of the gain tables, the limited-range
bounds or the outside of the RGB cube.  The images built here are laid out in "cells" (one chroma sample with the luma
samples it covers; one pixel for 4:4:4 and RGB formats), in row-major cell order:

  1. ramp, pass A:   every code 0..N-1 in all channels at once (RGB) / in luma with neutral chroma (YCbCr)
  2. ramp, pass B:   every code 0..N-1 in each channel alone against 0 in the two others
  3. draws:          independent seeded draws from the edge set E8 / E10, per channel (per chroma sample where the
                     format subsamples); the SDR and the HDR image of a pair draw independently
  4. corners:        the last two rows hold 4-pixel wide vertical bars: SDR {black, white} against HDR {peak, zero} in
                     every combination, so the corner pairs do not hang on the draws

N is 256 (SDR) or 1024 (HDR).  The case lists of the two test modules live here too, so that the CPU module pins
port == ref on exactly what the device module runs."""
import numpy as np

from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image

SEED = 5
SIZE_MAIN = (256, 128)   # a multiple of 16: the fused API-1 chain accepts it
SIZE_PIXEL = (200, 72)   # not a whole 256-pixel tile: the pixel kernels' ragged end


def _codes(*spans):
    return np.concatenate([np.arange(a, b + 1) for a, b in spans]).astype(np.uint16)


# the ends, the limited-range bounds of luma (16..235 / 64..940) and chroma (16..240 / 64..960), mid grey, the HLG knee
E8 = _codes((0, 3), (15, 17), (127, 129), (234, 236), (239, 241), (252, 255))
E10 = _codes((0, 4), (63, 65), (255, 256), (511, 513), (767, 768), (939, 941), (959, 961), (1019, 1023))

S420, S422, S444, SRGBA = (A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCr444,
                           A.UHDR_IMG_FMT_32bppRGBA8888)
HP010, H444, H1010102 = A.UHDR_IMG_FMT_24bppYCbCrP010, A.UHDR_IMG_FMT_30bppYCbCr444, A.UHDR_IMG_FMT_32bppRGBA1010102
_SUB = {S420: (2, 2), HP010: (2, 2), S422: (2, 1), S444: (1, 1), H444: (1, 1), SRGBA: (1, 1), H1010102: (1, 1)}
_RGB = (SRGBA, H1010102)

CORNER_BAR = 4  # pixels per corner bar


def _cells(fmt, w, h, n, edge, rng, hdr):
    """(c0[ncell, sx*sy], c1[ncell], c2[ncell]) uint16 codes in cell order; c0 is luma (per covered luma sample) or R."""
    sx, sy = _SUB[fmt]
    assert w % sx == 0 and h % sy == 0 and w % (2 * CORNER_BAR) == 0 and h % 2 == 0
    cw, ch, k = w // sx, h // sy, sx * sy
    ncell = cw * ch
    rgb = fmt in _RGB
    mid = 0 if rgb else n // 2
    c0 = rng.choice(edge, size=(ncell, k))
    c1 = rng.choice(edge, size=ncell)
    c2 = rng.choice(edge, size=ncell)
    ramp = np.arange(n, dtype=np.uint16)
    pos = 0

    def luma_ramp(chroma):
        nonlocal pos
        m = -(-n // k)
        flat = c0[pos:pos + m].reshape(-1)
        flat[:n] = ramp
        flat[n:] = n - 1
        c1[pos:pos + m] = chroma
        c2[pos:pos + m] = chroma
        pos += m

    def one_ramp(which):
        nonlocal pos
        c0[pos:pos + n], c1[pos:pos + n], c2[pos:pos + n] = 0, 0, 0
        (c0, c1, c2)[which][pos:pos + n] = ramp[:, None] if which == 0 else ramp
        pos += n

    if rgb:  # pass A: grey ramp
        c0[:n, 0], c1[:n], c2[:n] = ramp, ramp, ramp
        pos = n
        one_ramp(0)
    else:
        luma_ramp(mid)
        luma_ramp(0)
    one_ramp(1)
    one_ramp(2)
    # corners: the last 2 image rows, vertical bars of CORNER_BAR pixels
    rows = 2 // sy
    assert pos <= ncell - rows * cw, "the image is too small for the ramps"
    top = n - 1
    bar = np.arange(0, w, sx) // CORNER_BAR  # per cell; bars are cell aligned: CORNER_BAR is a multiple of sx
    if hdr:  # peak white, zero
        table, cx = np.array([(top, mid or top, mid or top), (0, mid, mid)], dtype=np.uint16), (bar // 2) % 2
    else:  # black, white
        table, cx = np.array([(0, mid, mid), (top, mid or top, mid or top)], dtype=np.uint16), bar % 2
    for r in range(rows):
        s = ncell - (r + 1) * cw
        c0[s:s + cw] = table[cx, 0][:, None]
        c1[s:s + cw] = table[cx, 1]
        c2[s:s + cw] = table[cx, 2]
    return c0.astype(np.uint16), c1.astype(np.uint16), c2.astype(np.uint16)


def _planes(fmt, w, h, cells):
    sx, sy = _SUB[fmt]
    cw, ch = w // sx, h // sy
    c0, c1, c2 = cells
    luma = c0.reshape(ch, cw, sy, sx).transpose(0, 2, 1, 3).reshape(h, w)
    return luma, c1.reshape(ch, cw), c2.reshape(ch, cw)


def channels(img):
    """The (c0, c1, c2) code planes of a lattice image at their own resolution (what the builders wrote)."""
    if img.fmt == SRGBA:
        v = img.valid(0)
        return [((v >> s) & 0xFF).astype(np.uint16) for s in (0, 8, 16)]
    if img.fmt == H1010102:
        v = img.valid(0)
        return [((v >> s) & 0x3FF).astype(np.uint16) for s in (0, 10, 20)]
    if img.fmt == HP010:
        uv = img.valid(1)
        return [img.valid(0) >> 6, uv[:, 0::2] >> 6, uv[:, 1::2] >> 6]
    return [img.valid(i).astype(np.uint16) for i in range(3)]


def at_pixels(img):
    """channels() with the chroma planes repeated to the luma grid."""
    sx, sy = _SUB[img.fmt]
    c = channels(img)
    return [c[0]] + [np.repeat(np.repeat(p, sy, 0), sx, 1) for p in c[1:]]


def sdr(fmt, w, h, cg=A.UHDR_CG_BT_709, seed=SEED, align=64):
    """SDR lattice image: YCbCr 4:2:0 / 4:2:2 / 4:4:4 or RGBA8888, sRGB transfer, full range."""
    rng = np.random.default_rng([seed, 8, fmt])
    y, u, v = _planes(fmt, w, h, _cells(fmt, w, h, 256, E8, rng, hdr=False))
    img = Image(fmt, w, h, cg, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align)
    if fmt == SRGBA:
        img.valid(0)[:] = y.astype(np.uint32) | (u.astype(np.uint32) << 8) | (v.astype(np.uint32) << 16) | (np.uint32(255) << 24)
    else:
        for i, p in enumerate((y, u, v)):
            img.valid(i)[:] = p.astype(np.uint8)
    return img


def hdr(fmt, w, h, ct, cg=A.UHDR_CG_BT_2100, rng_range=A.UHDR_CR_FULL_RANGE, seed=SEED, align=64):
    """HDR lattice image: P010 or 30bppYCbCr444 (limited or full range: the codes are the same, what they mean differs)
    or RGBA1010102."""
    rng = np.random.default_rng([seed, 10, fmt])
    y, u, v = _planes(fmt, w, h, _cells(fmt, w, h, 1024, E10, rng, hdr=True))
    img = Image(fmt, w, h, cg, ct, rng_range, align)
    if fmt == H1010102:
        img.valid(0)[:] = y.astype(np.uint32) | (u.astype(np.uint32) << 10) | (v.astype(np.uint32) << 20) | (np.uint32(3) << 30)
    elif fmt == HP010:
        img.valid(0)[:] = y << 6
        uv = img.valid(1)
        uv[:, 0::2] = u << 6
        uv[:, 1::2] = v << 6
    else:
        for i, p in enumerate((y, u, v)):
            img.valid(i)[:] = p
    return img


# ---- the cases of tests/test_gpu_code_lattice.py (and of the port == ref pin in tests/test_code_lattice.py) ------------
HLG, PQ, LINEAR = A.UHDR_CT_HLG, A.UHDR_CT_PQ, A.UHDR_CT_LINEAR
BT709, P3, BT2100 = A.UHDR_CG_BT_709, A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_2100
LIMITED, FULL = A.UHDR_CR_LIMITED_RANGE, A.UHDR_CR_FULL_RANGE

# name -> (sdr fmt, sdr gamut, hdr fmt, hdr transfer, hdr gamut, hdr range)
PAIRS = {
    "420+p010-hlg-limited": (S420, BT709, HP010, HLG, BT2100, LIMITED),
    "420p3+p010-pq-full": (S420, P3, HP010, PQ, BT2100, FULL),
    "rgba+1010102-pq-2100": (SRGBA, BT709, H1010102, PQ, BT2100, FULL),
    "rgba+1010102-hlg-709": (SRGBA, BT709, H1010102, HLG, BT709, FULL),
    "422+444-pq-limited": (S422, BT709, H444, PQ, BT2100, LIMITED),
    "422+444-hlg-full": (S422, BT709, H444, HLG, P3, FULL),
    "444+444-pq-limited": (S444, BT709, H444, PQ, BT2100, LIMITED),
    "444+444-hlg-full": (S444, BT709, H444, HLG, P3, FULL),
}
MAIN_PAIRS = list(PAIRS)[:4]
YUV444_PAIRS = list(PAIRS)[4:]

CFGS = {
    "default": dict(),  # two pass, three channels, scale 1
    "realtime": dict(preset=A.UHDR_USAGE_REALTIME),
    "one-channel": dict(use_multi_channel_gainmap=0),
    "one-channel-max-realtime-s2": dict(use_multi_channel_gainmap=0, use_luminance=0, preset=A.UHDR_USAGE_REALTIME, map_dimension_scale_factor=2),
    "s4": dict(map_dimension_scale_factor=4),
    "gamma1.3": dict(gamma=1.3),
    "hints0.5-8": dict(min_content_boost=0.5, max_content_boost=8.0),
    "realtime-one-channel-s2": dict(preset=A.UHDR_USAGE_REALTIME, use_multi_channel_gainmap=0, map_dimension_scale_factor=2),
    "one-channel-s4": dict(use_multi_channel_gainmap=0, map_dimension_scale_factor=4),  # applyGainMap's second map
}
MAIN_CFGS = ["default", "realtime", "one-channel", "one-channel-max-realtime-s2", "s4", "gamma1.3", "hints0.5-8"]
GENERATE_CASES = [(p, c) for p in MAIN_PAIRS for c in MAIN_CFGS] + [(p, c) for p in YUV444_PAIRS for c in ("default", "realtime-one-channel-s2")]

# every lattice HDR image of PAIRS, each under HLG, PQ and LINEAR, at both sizes
TONEMAP_IMAGES = {"p010-limited": (HP010, BT2100, LIMITED), "p010-full": (HP010, BT2100, FULL), "1010102-2100": (H1010102, BT2100, FULL),
                  "1010102-709": (H1010102, BT709, FULL), "444-limited": (H444, BT2100, LIMITED), "444-full-p3": (H444, P3, FULL)}
TONEMAP_CASES = [(k, ct, size) for k in TONEMAP_IMAGES for ct in (HLG, PQ, LINEAR) for size in (SIZE_MAIN, SIZE_PIXEL)]

# applyGainMap: the reference's own map + metadata of these generate cases, on the pair's 4:2:0 lattice SDR (the PQ pair's
# HDR side goes up to 10000 nits, so its applied output sits at the ceiling; the HLG pair has the smaller capacity)
APPLY_MAPS = [(p, c) for p in ("420p3+p010-pq-full", "420+p010-hlg-limited") for c in ("default", "one-channel-s4")]
APPLY_CASES = [(m, ct, boost) for m in range(len(APPLY_MAPS)) for ct in (LINEAR, HLG, PQ) for boost in (A.FLT_MAX, 4.0)]

CLAMP_MIN_BOOST = float(np.float32(2.0) ** np.float32(-14.3))  # exp2f of the clamp constants of jpegr.cpp:973-974
CLAMP_MAX_BOOST = float(np.float32(2.0) ** np.float32(15.6))


def pair(name, size=SIZE_MAIN):
    sf, scg, hf, hct, hcg, hr = PAIRS[name]
    return sdr(sf, *size, cg=scg), hdr(hf, *size, ct=hct, cg=hcg, rng_range=hr)


def tonemap_image(key, ct, size):
    fmt, cg, rr = TONEMAP_IMAGES[key]
    return hdr(fmt, *size, ct=ct, cg=cg, rng_range=rr)


def cfg(name):
    return A.default_encode_cfg(**CFGS[name])
