"""The kernel routes of the pixel-format operators as functions of the caller's layout: a plain helper module for
tests/test_route_lattice.py (CPU) and tests/test_gpu_route_lattice.py (device), in the manner of tests/tile_loop_shapes.py.

The oldest launchers each choose between a vector ("wide" / VEC) kernel and a per-pixel one on width, height, strides and the
alignment of every plane base.  Each predicate is restated here as a list of named conjuncts over a Case (format, size, strides in
samples, byte offset of each plane base from a 256-byte boundary); route() names what a case selects.  CASES is the table both
tests walk: for every conjunct of every predicate one case with all conjuncts true and one in which that conjunct alone is false.
MIRRORED lists the source lines restated here; the CPU test checks that they still read the same.  REFUSED lists the routes a host
check keeps callers away from, with the check's place."""
from collections import namedtuple

from libultrahdr_amd import capi as A

P010, S420, S444, S444_10 = A.UHDR_IMG_FMT_24bppYCbCrP010, A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_24bppYCbCr444, A.UHDR_IMG_FMT_30bppYCbCr444
RGBA, RGB, R1010102, F16, Y400 = (A.UHDR_IMG_FMT_32bppRGBA8888, A.UHDR_IMG_FMT_24bppRGB888, A.UHDR_IMG_FMT_32bppRGBA1010102,
                                  A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_8bppYCbCr400)

# (file under libultrahdr_amd/csrc, text): what the functions below restate
MIRRORED = [
    ("convert.hip", "if (im.fmt == UHDR_IMG_FMT_12bppYCbCr420 && im.w % 8 == 0 && im.h % 2 == 0 && im.stride[0] % 8 == 0 && im.stride[1] % 4 == 0 &&"),
    ("convert.hip", "im.stride[2] % 4 == 0 && al(im.p[0], 8) && al(im.p[1], 4) && al(im.p[2], 4)) {"),
    ("convert.hip", "if (im.fmt == UHDR_IMG_FMT_24bppYCbCr444 && im.w % 8 == 0 && im.stride[0] % 8 == 0 && im.stride[1] % 8 == 0 && im.stride[2] % 8 == 0 &&"),
    ("convert.hip", "al(im.p[0], 8) && al(im.p[1], 8) && al(im.p[2], 8)) {"),
    ("convert.hip", "const bool packed32 = p.src.fmt == UHDR_IMG_FMT_32bppRGBA1010102 || p.src.fmt == UHDR_IMG_FMT_32bppRGBA8888;"),
    ("convert.hip", "bool wide = packed32 && p.src.w % 8 == 0 && p.src.stride[0] % 4 == 0 && al(p.src.p[0], 16) && (!sub || p.src.h % 2 == 0);"),
    ("convert.hip", "const size_t ya = ten ? 16 : 8;  // bytes of 8 luma samples"),
    ("convert.hip", "wide = al(p.dst.p[0], ya) && (p.dst.stride[0] * (ten ? 2 : 1)) % ya == 0;"),
    ("convert.hip", "if (ten) wide = wide && al(p.dst.p[1], 16) && (p.dst.stride[1] * 2) % 16 == 0;"),
    ("convert.hip", "else wide = wide && al(p.dst.p[1], 4) && al(p.dst.p[2], 4) && p.dst.stride[1] % 4 == 0 && p.dst.stride[2] % 4 == 0;"),
    ("convert.hip", "for (int c = 0; c < 3; c++) wide = wide && al(p.dst.p[c], ya) && (p.dst.stride[c] * (ten ? 2 : 1)) % ya == 0;"),
    ("pixel_io.h", "if (im.w % 2 || im.h % 2) return false;"),
    ("pixel_io.h", "return im.stride[0] % 2 == 0 && im.stride[1] % 2 == 0 && ((uintptr_t)im.p[0] % 4 == 0) && ((uintptr_t)im.p[1] % 4 == 0);"),
    ("pixel_io.h", "if (im.fmt == UHDR_IMG_FMT_12bppYCbCr420) return im.stride[0] % 2 == 0 && ((uintptr_t)im.p[0] % 2 == 0);"),
    ("tonemap.hip", "const bool vec_in = quad_layout_ok(p.hdr);"),
    ("tonemap.hip", "if (((sy | (uintptr_t)yp) & 1) == 0) {  // two luma bytes per row as one 16-bit store"),
    ("tonemap.hip", "const bool lut = p.hdr_inv_lut != nullptr;"),
    ("tonemap.hip", "if (p.gamut_on) {"),
    ("tonemap.hip", "if (p.hdr.fmt == UHDR_IMG_FMT_24bppYCbCrP010) {"),
    ("jpeg_decode.hip", "const bool vec = (p.w % 4 == 0) && al(p.rgb, p.bpp == 4 ? 16 : 4) && ((size_t)p.rgb_stride_px * p.bpp) % (p.bpp == 4 ? 16 : 4) == 0 &&"),
    ("jpeg_decode.hip", "al(p.po[0], 4) && al(p.po[1], 4) && al(p.po[2], 4) && p.stride[0] % 4 == 0 && p.stride[1] % 4 == 0 && p.stride[2] % 4 == 0;"),
    ("jpeg_decode.hip", "const bool vec = (p.w % 4 == 0) && al(p.rgb_out, p.bpp == 4 ? 16 : 4) && ((size_t)p.rgb_stride_px * p.bpp) % (p.bpp == 4 ? 16 : 4) == 0 &&"),
    ("jpeg_decode.hip", "al(p.p[0], 4) && al(p.p[1], 4) && al(p.p[2], 4) && p.stride[0] % 4 == 0 && p.stride[1] % 4 == 0 && p.stride[2] % 4 == 0;"),
    ("jpeg_decode.hip", "const bool vec_store = ((stride | (uintptr_t)plane) & 7) == 0;"),
    ("jpeg_decode.hip", "const bool vec_ok = ((a.pitch | (uintptr_t)a.rgb) & (BPP == 4 ? 15 : 7)) == 0;"),
    ("upsample_core.h", "if (vec_ok && x0 + 8 <= w) {"),
    ("fdct_quant.hip", "if (((uintptr_t)src & 3) == 0) {"),
    ("generate_gainmap.hip", "return p.scale == 1 && p.sdr.fmt == UHDR_IMG_FMT_12bppYCbCr420 && p.hdr.fmt == UHDR_IMG_FMT_24bppYCbCrP010 && quad_layout_ok(p.sdr) &&"),
    ("generate_gainmap.hip", "quad_layout_ok(p.hdr);"),
    ("generate_gainmap.hip", "if (p.gamma != 1.0f && !p.gamma_thr) {"),
    ("generate_gainmap.hip", "if ((p.nch == 1 || p.nch == 3) && p.map_w % 16 == 0 && ((size_t)p.out_stride * p.nch) % 16 == 0 && (((uintptr_t)p.out & 15) == 0) &&"),
    ("generate_gainmap.hip", "(((uintptr_t)p.gain_log2 & 15) == 0)) {"),
    ("generate_gainmap.hip", "const bool vec4 = (row_elems % 4 == 0) && ((p.out_stride * p.nch) % 4 == 0) && (((uintptr_t)p.out & 3) == 0) &&"),
    ("generate_gainmap.hip", "(((uintptr_t)p.gain_log2 & 15) == 0);"),
    ("api_jpeg.cpp", "if (pitch % al || ((uintptr_t)rgb->planes[0] % al))"),
]

# routes no caller reaches: (launcher, route, file, the line of the host check that refuses the layout first)
REFUSED = [
    ("fdct_quant_rgb", "fdct_quant_rgb_kernel on rows or a base off 8 (RGB888) / 16 (RGBA8888) bytes", "api_jpeg.cpp",
     "if (pitch % al || ((uintptr_t)rgb->planes[0] % al))"),
]

Layout = namedtuple("Layout", "fmt strides offsets")
# a, b, c: the images of the call in argument order (see the launcher's section below); opt: a dict of what else the call takes
Case = namedtuple("Case", "launcher name w h a b c opt")


def _al(off, n):
    """al(ptr, n) for a base `off` bytes past a 256-byte boundary."""
    return off % n == 0


# ---- the predicates: id -> (launcher, applies(case), conjuncts(case) -> [(name, bool)]) -------------------------------------------------
def _yuv420(c):
    s, o = c.a.strides, c.a.offsets
    return [("w % 8", c.w % 8 == 0), ("h % 2", c.h % 2 == 0), ("stride[0] % 8", s[0] % 8 == 0), ("stride[1] % 4", s[1] % 4 == 0),
            ("stride[2] % 4", s[2] % 4 == 0), ("al(p[0], 8)", _al(o[0], 8)), ("al(p[1], 4)", _al(o[1], 4)), ("al(p[2], 4)", _al(o[2], 4))]


def _yuv444(c):
    s, o = c.a.strides, c.a.offsets
    return [("w % 8", c.w % 8 == 0)] + [(f"stride[{i}] % 8", s[i] % 8 == 0) for i in range(3)] + [(f"al(p[{i}], 8)", _al(o[i], 8)) for i in range(3)]


def _rgb_sub(c):
    return c.b.fmt in (P010, S420)


def _rgb2ycbcr(c):
    ten = c.a.fmt == R1010102
    out = [("src.w % 8", c.w % 8 == 0), ("src.stride[0] % 4", c.a.strides[0] % 4 == 0), ("al(src.p[0], 16)", _al(c.a.offsets[0], 16))]
    if not ten:  # (a 10-bit destination has an RGBA1010102 source: packed32 holds)
        out.insert(0, ("packed32", c.a.fmt == RGBA))
    ds, do = c.b.strides, c.b.offsets
    ya, k = (16, 2) if ten else (8, 1)
    if _rgb_sub(c):
        out += [("src.h % 2", c.h % 2 == 0), (f"al(dst.p[0], {ya})", _al(do[0], ya)), (f"dst pitch[0] % {ya}", (ds[0] * k) % ya == 0)]
        if ten:
            out += [("al(dst.p[1], 16)", _al(do[1], 16)), ("dst pitch[1] % 16", (ds[1] * 2) % 16 == 0)]
        else:
            out += [("al(dst.p[1], 4)", _al(do[1], 4)), ("al(dst.p[2], 4)", _al(do[2], 4)), ("dst.stride[1] % 4", ds[1] % 4 == 0),
                    ("dst.stride[2] % 4", ds[2] % 4 == 0)]
    else:
        for i in range(3):
            out += [(f"al(dst.p[{i}], {ya})", _al(do[i], ya)), (f"dst pitch[{i}] % {ya}", (ds[i] * k) % ya == 0)]
    return out


def _jpeg_colour(c):
    """launch_jpeg_rgb_to_ycc (a = rgb, b = ycc) and launch_jpeg_ycc_to_rgb (a = ycc, b = rgb): the same predicate."""
    rgb, ycc = (c.a, c.b) if c.launcher == "jpeg_rgb_to_ycc" else (c.b, c.a)
    bpp = 4 if rgb.fmt == RGBA else 3
    n = 16 if bpp == 4 else 4
    return ([("w % 4", c.w % 4 == 0), (f"al(rgb, {n})", _al(rgb.offsets[0], n)), (f"rgb pitch % {n}", (rgb.strides[0] * bpp) % n == 0)] +
            [(f"al(p[{i}], 4)", _al(ycc.offsets[i], 4)) for i in range(3)] + [(f"stride[{i}] % 4", ycc.strides[i] % 4 == 0) for i in range(3)])


def _idct(c):
    return [("stride & 7", c.b.strides[0] % 8 == 0), ("plane & 7", _al(c.b.offsets[0], 8))]


def _idct_rgb(c):
    bpp = 4 if c.b.fmt == RGBA else 3
    n = 16 if bpp == 4 else 8
    return [(f"pitch & {n - 1}", (c.b.strides[0] * bpp) % n == 0), (f"rgb & {n - 1}", _al(c.b.offsets[0], n))]


def _fdct(c):
    """fdct_quant_kernel decides per row: every row of every block takes the dword loads when base and stride are multiples of 4."""
    return [("stride & 3", c.a.strides[0] % 4 == 0), ("plane & 3", _al(c.a.offsets[0], 4))]


def _quad_ok_p010(im, w, h, who):
    return [("w % 2", w % 2 == 0), ("h % 2", h % 2 == 0), (f"{who}.stride[0] % 2", im.strides[0] % 2 == 0), (f"{who}.stride[1] % 2", im.strides[1] % 2 == 0),
            (f"{who}.p[0] % 4", _al(im.offsets[0], 4)), (f"{who}.p[1] % 4", _al(im.offsets[1], 4))]


def _tone_load(c):
    return _quad_ok_p010(c.a, c.w, c.h, "hdr")


def _tone_store(c):
    return [("sdr.stride[0] & 1", c.b.strides[0] % 2 == 0), ("sdr.p[0] & 1", _al(c.b.offsets[0], 2))]


def _gen_quad(c):
    out = [("scale == 1", c.opt["scale"] == 1), ("sdr 4:2:0", c.a.fmt == S420), ("hdr P010", c.b.fmt == P010)]
    # (quad_layout_ok of an image of another format is false for the format alone: its layout terms then count as met)
    sdr = c.a if c.a.fmt == S420 else Layout(S420, (0, 0, 0), (0, 0, 0))
    hdr = c.b if c.b.fmt == P010 else Layout(P010, (0, 0), (0, 0))
    return out + [("sdr.stride[0] % 2", sdr.strides[0] % 2 == 0), ("sdr.p[0] % 2", _al(sdr.offsets[0], 2))] + _quad_ok_p010(hdr, c.w, c.h, "hdr")


def _map_geom(c):
    s = c.opt["scale"]
    return c.w // s, c.h // s, c.opt["nch"]


def _affine_exact(c):
    return c.opt["two_pass"] and c.opt["gamma"] != 1.0 and not c.opt.get("gamma_table")


def _affine_wide(c):
    mw, _, nch = _map_geom(c)
    return [("map_w % 16", mw % 16 == 0), ("out pitch % 16", (c.c.strides[0] * nch) % 16 == 0), ("out & 15", _al(c.c.offsets[0], 16)),
            ("gain_log2 & 15", _al(c.opt.get("gain_off", 0), 16))]


def _affine_vec4(c):
    mw, _, nch = _map_geom(c)
    return [("row_elems % 4", (mw * nch) % 4 == 0), ("out pitch % 4", (c.c.strides[0] * nch) % 4 == 0), ("out & 3", _al(c.c.offsets[0], 4)),
            ("gain_log2 & 15", _al(c.opt.get("gain_off", 0), 16))]


def _all(conj):
    return all(v for _, v in conj)


# launch_affine_map has two predicates in a row (the wide kernel, then vec4 below it); opt["affine_pairs"] says for which of the two a
# two-pass case was written, so that each predicate's pairs are looked for among its own cases
def _affine_applies(c):
    return c.launcher == "generate" and c.opt["two_pass"] and not _affine_exact(c)


PREDICATES = {
    "launch_transform_yuv 4:2:0": (lambda c: c.launcher == "transform_yuv" and c.a.fmt == S420, _yuv420),
    "launch_transform_yuv 4:4:4": (lambda c: c.launcher == "transform_yuv" and c.a.fmt == S444, _yuv444),
    "launch_rgb_to_ycbcr 8-bit 4:2:0": (lambda c: c.launcher == "rgb_to_ycbcr" and c.b.fmt == S420, _rgb2ycbcr),
    "launch_rgb_to_ycbcr 8-bit 4:4:4": (lambda c: c.launcher == "rgb_to_ycbcr" and c.b.fmt == S444, _rgb2ycbcr),
    "launch_rgb_to_ycbcr 10-bit 4:2:0": (lambda c: c.launcher == "rgb_to_ycbcr" and c.b.fmt == P010, _rgb2ycbcr),
    "launch_rgb_to_ycbcr 10-bit 4:4:4": (lambda c: c.launcher == "rgb_to_ycbcr" and c.b.fmt == S444_10, _rgb2ycbcr),
    "launch_jpeg_rgb_to_ycc BPP 3": (lambda c: c.launcher == "jpeg_rgb_to_ycc" and c.a.fmt == RGB, _jpeg_colour),
    "launch_jpeg_rgb_to_ycc BPP 4": (lambda c: c.launcher == "jpeg_rgb_to_ycc" and c.a.fmt == RGBA, _jpeg_colour),
    "launch_jpeg_ycc_to_rgb BPP 3": (lambda c: c.launcher == "jpeg_ycc_to_rgb" and c.b.fmt == RGB, _jpeg_colour),
    "launch_jpeg_ycc_to_rgb BPP 4": (lambda c: c.launcher == "jpeg_ycc_to_rgb" and c.b.fmt == RGBA, _jpeg_colour),
    "idct_dequant_kernel vec_store": (lambda c: c.launcher == "idct_dequant", _idct),
    "idct_dequant_rgb_kernel<3> vec_ok": (lambda c: c.launcher == "idct_dequant_rgb" and c.b.fmt == RGB, _idct_rgb),
    "idct_dequant_rgb_kernel<4> vec_ok": (lambda c: c.launcher == "idct_dequant_rgb" and c.b.fmt == RGBA, _idct_rgb),
    "fdct_quant_kernel dword rows": (lambda c: c.launcher == "fdct_quant", _fdct),
    "tonemap_p010_kernel quad_layout_ok(hdr)": (lambda c: c.launcher == "tone_map" and c.a.fmt == P010 and _all(_tone_store(c)), _tone_load),
    "tonemap_p010_kernel 16-bit luma store": (lambda c: c.launcher == "tone_map" and c.a.fmt == P010 and _all(_tone_load(c)), _tone_store),
    "gen_quad_path": (lambda c: c.launcher == "generate" and not c.opt["two_pass"], _gen_quad),
    "launch_affine_map wide": (lambda c: _affine_applies(c) and c.opt.get("affine_pairs") == "wide", _affine_wide),
    "launch_affine_map vec4": (lambda c: _affine_applies(c) and c.opt.get("affine_pairs") == "vec4", _affine_vec4),
}


# ---- the routes ---------------------------------------------------------------------------------------------------------------------------
def route(c):
    """The kernel routes case c selects, as a tuple of names (one launch, or one launch and the per-lane choices inside it)."""
    L = c.launcher
    if L == "transform_yuv":
        if c.a.fmt == S420:
            return ("transform_yuv420_wide_kernel" if _all(_yuv420(c)) else "transform_yuv420_kernel",)
        return ("transform_yuv444_wide_kernel" if _all(_yuv444(c)) else "transform_yuv444_kernel",)
    if L == "rgb_to_ycbcr":
        ten = "true" if c.a.fmt == R1010102 else "false"
        return (f"rgb_to_ycbcr{'420' if _rgb_sub(c) else '444'}{'_wide' if _all(_rgb2ycbcr(c)) else ''}_kernel<{ten}>",)
    if L in ("jpeg_rgb_to_ycc", "jpeg_ycc_to_rgb"):
        rgb = c.a if L == "jpeg_rgb_to_ycc" else c.b
        return (f"{L}_kernel<{4 if rgb.fmt == RGBA else 3}, {'true' if _all(_jpeg_colour(c)) else 'false'}>",)
    if L == "idct_dequant":
        return ("idct_dequant_kernel: 8-byte store" if _all(_idct(c)) else "idct_dequant_kernel: byte stores",)
    if L == "idct_dequant_rgb":
        k = f"idct_dequant_rgb_kernel<{4 if c.b.fmt == RGBA else 3}>"
        out = []
        if _all(_idct_rgb(c)) and c.w >= 8:
            out.append(f"{k}: vector stores")
        if not _all(_idct_rgb(c)):
            out.append(f"{k}: byte stores")
        if c.w % 8:
            out.append(f"{k}: partial last block")
        return tuple(out)
    if L == "fdct_quant":
        s, o = c.a.strides[0], c.a.offsets[0]
        if s % 4 == 0:
            return ("fdct_quant_kernel: dword loads" if o % 4 == 0 else "fdct_quant_kernel: byte loads",)
        return ("fdct_quant_kernel: dword and byte loads alternate by row",)
    if L == "fdct_quant_rgb":
        return ("fdct_quant_rgb_kernel" if _all(_idct_rgb(c._replace(b=c.a))) else "refused",)
    if L == "tone_map":
        if c.a.fmt == P010:
            gamut, lut = int(c.opt["cg"] != A.UHDR_CG_DISPLAY_P3), "true" if c.opt["ct"] != A.UHDR_CT_LINEAR else "false"
            return (f"tonemap_p010_kernel<{gamut}, {lut}>", "p010: quad loads" if _all(_tone_load(c)) else "p010: pixel loads",
                    "p010: 16-bit luma store" if _all(_tone_store(c)) else "p010: byte luma stores")
        name = {R1010102: "UHDR_IMG_FMT_32bppRGBA1010102", F16: "UHDR_IMG_FMT_64bppRGBAHalfFloat"}.get(c.a.fmt, "-1")
        return (f"tonemap_pixel_kernel<{name}> -> {'RGBA8888' if c.b.fmt == RGBA else 'YCbCr444'}",)
    if L == "generate":
        two = c.opt["two_pass"]
        out = [("generate_quad_kernel" if _all(_gen_quad(c)) else "generate_kernel") + ("<two pass>" if two else "<one pass>")]
        if two:
            nch = c.opt["nch"]
            if _affine_exact(c):
                out.append("affine_exact_kernel")
            elif _all(_affine_wide(c)):
                out.append(f"affine_wide_kernel<{nch}>")
            else:
                out.append("affine_kernel<true>" if _all(_affine_vec4(c)) else "affine_kernel<false>")
        return tuple(out)
    raise ValueError(f"unknown launcher {L!r}")


# every route of every launcher: what CASES has to reach
ROUTES = {
    "transform_yuv": ["transform_yuv420_wide_kernel", "transform_yuv420_kernel", "transform_yuv444_wide_kernel", "transform_yuv444_kernel"],
    "rgb_to_ycbcr": [f"rgb_to_ycbcr{s}{v}_kernel<{t}>" for s in ("420", "444") for v in ("_wide", "") for t in ("true", "false")],
    "jpeg_rgb_to_ycc": [f"jpeg_rgb_to_ycc_kernel<{b}, {v}>" for b in (3, 4) for v in ("true", "false")],
    "jpeg_ycc_to_rgb": [f"jpeg_ycc_to_rgb_kernel<{b}, {v}>" for b in (3, 4) for v in ("true", "false")],
    "idct_dequant": ["idct_dequant_kernel: 8-byte store", "idct_dequant_kernel: byte stores"],
    "idct_dequant_rgb": [f"idct_dequant_rgb_kernel<{b}>: {r}" for b in (3, 4) for r in ("vector stores", "byte stores", "partial last block")],
    "fdct_quant": ["fdct_quant_kernel: dword loads", "fdct_quant_kernel: byte loads", "fdct_quant_kernel: dword and byte loads alternate by row"],
    "fdct_quant_rgb": ["fdct_quant_rgb_kernel", "refused"],
    "tone_map": [f"tonemap_p010_kernel<{g}, {l}>" for g in (0, 1) for l in ("true", "false")] +
                ["p010: quad loads", "p010: pixel loads", "p010: 16-bit luma store", "p010: byte luma stores",
                 "tonemap_pixel_kernel<UHDR_IMG_FMT_32bppRGBA1010102> -> RGBA8888", "tonemap_pixel_kernel<UHDR_IMG_FMT_64bppRGBAHalfFloat> -> RGBA8888",
                 "tonemap_pixel_kernel<-1> -> YCbCr444"],
    "generate": ["generate_quad_kernel<one pass>", "generate_quad_kernel<two pass>", "generate_kernel<one pass>", "generate_kernel<two pass>",
                 "affine_exact_kernel", "affine_wide_kernel<1>", "affine_wide_kernel<3>", "affine_kernel<true>", "affine_kernel<false>"],
}


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def _planes(fmt):
    return {P010: 2, S420: 3, S444: 3, S444_10: 3}.get(fmt, 1)


def _lay(fmt, strides, offsets=None):
    strides = list(strides)
    return Layout(fmt, tuple(strides), tuple(offsets) if offsets is not None else (0,) * len(strides))


def _put(t, i, v):
    t = list(t)
    t[i] = v
    return tuple(t)


def _flips(base, image, sizes, strides, offsets):
    """`base` and one case per entry: sizes = [(tag, w, h)], strides = [(plane, value)], offsets = [(plane, bytes)] applied to the image
    in field `image` ('a', 'b' or 'c') of base."""
    out = [base]
    for tag, w, h in sizes:
        out.append(base._replace(name=f"{base.name}/{tag}", w=w, h=h))
    lay = getattr(base, image)
    for i, v in strides:
        out.append(base._replace(name=f"{base.name}/{image}.stride[{i}]={v}", **{image: lay._replace(strides=_put(lay.strides, i, v))}))
    for i, v in offsets:
        out.append(base._replace(name=f"{base.name}/{image}.p[{i}]+{v}", **{image: lay._replace(offsets=_put(lay.offsets, i, v))}))
    return out


def _cases():
    cs = []
    # convertYuv, in place: a = the image.  72 x 20 inside strides of 80 / 40: every flip keeps every stride at least the width
    b = Case("transform_yuv", "yuv420", 72, 20, _lay(S420, (80, 40, 40)), None, None, {})
    cs += _flips(b, "a", [("w=74", 74, 20), ("h=19", 72, 19), ("w=73,h=19", 73, 19)], [(0, 84), (1, 42), (2, 42), (1, 37)], [(0, 4), (1, 2), (2, 2), (2, 1)])
    b = Case("transform_yuv", "yuv444", 72, 18, _lay(S444, (80, 80, 80)), None, None, {})
    cs += _flips(b, "a", [("w=74", 74, 18)], [(0, 84), (1, 84), (2, 84)], [(0, 4), (1, 4), (2, 4)])
    # convert_raw_input_to_ycbcr: a = the packed source, b = the destination
    b = Case("rgb_to_ycbcr", "rgba->420", 72, 20, _lay(RGBA, (76,)), _lay(S420, (80, 40, 40)), None, {})
    cs += _flips(b, "a", [("w=74", 74, 20), ("h=19", 72, 19)], [(0, 75)], [(0, 4)])
    cs += _flips(b, "b", [], [(0, 84), (1, 42), (2, 42)], [(0, 4), (1, 2), (2, 2)])[1:]
    cs.append(b._replace(name="rgb888->420", a=_lay(RGB, (76,))))
    b = Case("rgb_to_ycbcr", "rgba->444", 72, 18, _lay(RGBA, (76,)), _lay(S444, (80, 80, 80)), None, {})
    cs += _flips(b, "a", [("w=74", 74, 18)], [(0, 75)], [(0, 8)])
    cs += _flips(b, "b", [], [(0, 84), (1, 84), (2, 84)], [(0, 4), (1, 4), (2, 4)])[1:]
    cs.append(b._replace(name="rgb888->444", a=_lay(RGB, (76,))))
    cs.append(b._replace(name="rgb888->444/tight", a=_lay(RGB, (72,), (1,)), b=_lay(S444, (72, 73, 75), (0, 1, 2))))
    b = Case("rgb_to_ycbcr", "1010102->p010", 72, 20, _lay(R1010102, (76,)), _lay(P010, (80, 80)), None, {})
    cs += _flips(b, "a", [("w=74", 74, 20), ("h=19", 72, 19)], [(0, 75)], [(0, 4)])
    cs += _flips(b, "b", [], [(0, 84), (1, 84)], [(0, 8), (1, 8)])[1:]
    b = Case("rgb_to_ycbcr", "1010102->444", 72, 18, _lay(R1010102, (76,)), _lay(S444_10, (80, 80, 80)), None, {})
    cs += _flips(b, "a", [("w=74", 74, 18)], [(0, 75)], [(0, 8)])
    cs += _flips(b, "b", [], [(0, 84), (1, 84), (2, 84)], [(0, 8), (1, 2), (2, 8)])[1:]
    # libjpeg's colour conversions: a = the source, b = the destination.  The RGB888 rows need a pixel stride that is a multiple of 4
    for rgbf, tag, so, n in ((RGB, "rgb888", 1, 4), (RGBA, "rgba8888", 4, 16)):
        b = Case("jpeg_rgb_to_ycc", f"{tag}->ycc", 72, 18, _lay(rgbf, (76,)), _lay(S444, (76, 76, 76)), None, {})
        cs += _flips(b, "a", [("w=74", 74, 18)], [(0, 75)], [(0, so)])
        cs += _flips(b, "b", [], [(0, 78), (1, 78), (2, 75)], [(0, 2), (1, 1), (2, 3)])[1:]
        b = Case("jpeg_ycc_to_rgb", f"ycc->{tag}", 72, 18, _lay(S444, (76, 76, 76)), _lay(rgbf, (76,)), None, {})
        cs += _flips(b, "a", [("w=74", 74, 18)], [(0, 78), (1, 75), (2, 78)], [(0, 1), (1, 2), (2, 3)])
        cs += _flips(b, "b", [], [(0, 75)], [(0, so)])[1:]
    # idct_dequant: b = the plane, whole blocks (72 x 24 is nine blocks per row: two groups of eight, the second with one block)
    b = Case("idct_dequant", "idct", 72, 24, None, _lay(Y400, (80,)), None, {})
    cs += _flips(b, "b", [], [(0, 84), (0, 75)], [(0, 4), (0, 1)])
    # idct_dequant_rgb: b = the packed destination; 74 and 66 end in a block that is partly outside w, 7 is nothing but such a block
    for rgbf, tag, sv, so in ((RGB, "rgb888", 75, 4), (RGBA, "rgba8888", 75, 4)):
        b = Case("idct_dequant_rgb", f"idct->{tag}", 72, 20, None, _lay(rgbf, (80,)), None, {})
        cs += _flips(b, "b", [("w=74", 74, 20), ("w=66,h=18", 66, 18), ("w=7", 7, 20)], [(0, sv)], [(0, so)])
        cs.append(b._replace(name=f"idct->{tag}/w=74/b.stride[0]={sv}", w=74, b=_lay(rgbf, (sv,))))
        cs.append(b._replace(name=f"idct->{tag}/w=74/tight", w=74, b=_lay(rgbf, (74,), (so,))))
    # fdct_quant: a = the plane
    b = Case("fdct_quant", "fdct", 72, 24, _lay(Y400, (80,)), None, None, {})
    cs += _flips(b, "a", [], [(0, 75), (0, 82)], [(0, 1), (0, 3), (0, 2)])
    cs.append(b._replace(name="fdct/a.stride[0]=75/a.p[0]+1", a=_lay(Y400, (75,), (1,))))
    # fdct_quant_rgb: a = the packed source; everything off the vector layout is refused by the host entry point
    for rgbf, tag in ((RGB, "rgb888"), (RGBA, "rgba8888")):
        b = Case("fdct_quant_rgb", f"{tag}->fdct", 72, 24, _lay(rgbf, (80,)), None, None, {})
        cs += _flips(b, "a", [], [(0, 75)], [(0, 4)])
    # toneMap at the size of tests/test_gpu_formats.py: a = the HDR intent, b = the SDR destination
    hlg, pq, lin = A.UHDR_CT_HLG, A.UHDR_CT_PQ, A.UHDR_CT_LINEAR
    c2100, p3, c709 = A.UHDR_CG_BT_2100, A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_709
    W, H = 256, 96
    b = Case("tone_map", "p010-hlg-2100", W, H, _lay(P010, (260, 260)), _lay(S420, (260, 130, 130)), None, dict(ct=hlg, cg=c2100))
    cs += _flips(b, "a", [("w=255", 255, H), ("h=95", W, 95)], [(0, 261), (1, 261)], [(0, 2), (1, 2)])
    cs += _flips(b, "b", [], [(0, 261), (1, 131), (2, 129)], [(0, 1), (1, 1), (2, 3)])[1:]
    cs.append(b._replace(name="p010-pq-p3", opt=dict(ct=pq, cg=p3)))
    cs.append(b._replace(name="p010-linear-709", opt=dict(ct=lin, cg=c709)))
    cs.append(b._replace(name="p010-linear-p3", opt=dict(ct=lin, cg=p3)))
    cs.append(b._replace(name="p010-linear-p3/tight", a=_lay(P010, (W, W), (2, 6)), b=_lay(S420, (W + 1, W // 2, W // 2), (1, 0, 0)), opt=dict(ct=lin, cg=p3)))
    cs.append(Case("tone_map", "1010102-pq", W, H, _lay(R1010102, (259,), (4,)), _lay(RGBA, (257,), (4,)), None, dict(ct=pq, cg=c2100)))
    cs.append(Case("tone_map", "f16-linear", W, H, _lay(F16, (257,), (8,)), _lay(RGBA, (259,), (12,)), None, dict(ct=lin, cg=c2100)))
    cs.append(Case("tone_map", "444-10bit-pq", W, H, _lay(S444_10, (257, 259, 261), (2, 4, 6)), _lay(S444, (257, 259, 261), (1, 2, 3)), None, dict(ct=pq, cg=c2100)))
    # generateGainMap at the same size: a = the SDR intent, b = the HDR intent, c = the map
    sdr, hdr = _lay(S420, (260, 130, 130)), _lay(P010, (260, 260))
    one = dict(two_pass=False, nch=1, scale=1, gamma=1.0)
    b = Case("generate", "one-pass-1ch", W, H, sdr, hdr, _lay(Y400, (272,)), one)
    cs += _flips(b, "a", [("w=255", 255, H), ("h=95", W, 95)], [(0, 261), (1, 129), (2, 131)], [(0, 1), (1, 1), (2, 3)])
    cs += _flips(b, "b", [], [(0, 261), (1, 261)], [(0, 2), (1, 2)])[1:]
    cs.append(b._replace(name="one-pass-1ch/scale=2", opt=dict(one, scale=2), c=_lay(Y400, (136,))))
    cs.append(b._replace(name="one-pass-1ch/sdr-444", a=_lay(S444, (260, 260, 260))))
    cs.append(b._replace(name="one-pass-1ch/hdr-1010102", b=_lay(R1010102, (260,))))
    cs.append(b._replace(name="one-pass-3ch", c=_lay(RGB, (259,), (1,)), opt=dict(one, nch=3)))
    cs.append(b._replace(name="one-pass-3ch/pixel", a=_lay(S420, (257, 129, 131), (1, 1, 3)), c=_lay(RGB, (259,), (1,)), opt=dict(one, nch=3)))
    for nch, mfmt in ((1, Y400), (3, RGB)):
        two = dict(two_pass=True, nch=nch, scale=1, gamma=1.0, affine_pairs="wide")
        b = Case("generate", f"two-pass-{nch}ch", W, H, sdr, hdr, _lay(mfmt, (272,)), two)
        cs += _flips(b, "c", [("w=252", 252, H)], [(0, 260 if nch == 1 else 268)], [(0, 4)])
        cs.append(b._replace(name=f"{b.name}/gain_log2+4", opt=dict(two, gain_off=4)))
        # below the wide kernel (w = 252): affine_kernel<true> against affine_kernel<false>
        v4 = dict(two, affine_pairs="vec4")
        b4 = b._replace(name=f"two-pass-{nch}ch/w=252/vec4", w=252, c=_lay(mfmt, (260,)), opt=v4)
        cs += _flips(b4, "c", [("w=254" if nch == 1 else "w=250", 254 if nch == 1 else 250, H)], [(0, 261 if nch == 1 else 262)], [(0, 1)])
        cs.append(b4._replace(name=f"{b4.name}/gain_log2+4", opt=dict(v4, gain_off=4)))
        cs.append(b._replace(name=f"two-pass-{nch}ch/pixel", a=_lay(S420, (257, 129, 131), (1, 1, 3)), opt=dict(two, affine_pairs=None)))
    cs.append(Case("generate", "two-pass-1ch/gamma-exact", W, H, sdr, hdr, _lay(Y400, (259,), (3,)), dict(two_pass=True, nch=1, scale=1, gamma=1.571)))
    cs.append(Case("generate", "two-pass-3ch/gamma-exact", W, H, sdr, hdr, _lay(RGB, (272,)), dict(two_pass=True, nch=3, scale=1, gamma=1.571)))
    return cs


CASES = _cases()


def cases_of(launcher):
    return [c for c in CASES if c.launcher == launcher]


def flipping_pairs(pid):
    """{conjunct name: (the case with every conjunct true, a case in which that conjunct alone is false) or None} for predicate pid."""
    applies, conj = PREDICATES[pid]
    cs = [c for c in CASES if applies(c)]
    full = [c for c in cs if _all(conj(c))]
    names = [n for n, _ in conj(full[0])] if full else []
    out = {}
    for i, n in enumerate(names):
        hit = None
        for c in cs:
            v = conj(c)
            if len(v) == len(names) and [k for k, (_, ok) in enumerate(v) if not ok] == [i]:
                hit = (full[0], c)
                break
        out[n] = hit
    return out


def describe():
    """Per launcher: the routes its cases take and how many cases take each."""
    lines = []
    for launcher in ROUTES:
        count = {}
        for c in cases_of(launcher):
            for r in route(c):
                count[r] = count.get(r, 0) + 1
        lines.append(f"{launcher}: {len(cases_of(launcher))} cases; " + "; ".join(f"{r} x {n}" for r, n in count.items()))
    return "\n".join(lines)
