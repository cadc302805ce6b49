"""The kernel routes of applyGainMap as a function of the caller's layout, and the geometry of its quad kernel: a plain helper module
for tests/test_apply_lattice.py (CPU) and tests/test_gpu_apply_lattice.py (device), the sibling of tests/route_lattice.py.

launch_apply_gainmap (apply_gainmap.hip) chooses between three entry points of the quad kernel and two forms of the generic kernel on
apply_quad_mode's conjuncts.  They are restated here by name over a Case: base format, w, h, y0, full_h, a Layout (strides in samples,
byte offset of each plane base from a 256-byte boundary) for the base image, the map and the destination, the map's format and size,
the output transfer, the gamma of each channel and the flags of the _ex entry point.  route() names what a case selects.

CASES is the first table: for every conjunct a caller of the C ABI can reach, a case in which every conjunct holds (an "anchor", with
every stride and base the predicate leaves alone odd or off every alignment) and a case in which that conjunct alone is false
(opt["flip_of"], opt["flips"]).  GEOMETRY is the second: legal layouts at the smallest sizes at which the quad kernel's own arithmetic --
ragged strips, row groups, map clamps, stripes, the frame table -- and the generic kernel's tile loop can still go wrong.  REFUSALS are
calls the C ABI answers with a code.  MIRRORED lists the source lines restated here, UNREACHABLE the conjuncts no caller can flip with
the host line that says why; the CPU test checks that all of them still stand."""
from collections import namedtuple

import numpy as np

from libultrahdr_amd import capi as A

S420, S422, S444 = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCr444
RGBA, RGB, Y400 = A.UHDR_IMG_FMT_32bppRGBA8888, A.UHDR_IMG_FMT_24bppRGB888, A.UHDR_IMG_FMT_8bppYCbCr400
F16, R1010102 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_32bppRGBA1010102
LINEAR, HLG, PQ = A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ
GAMMA_TABLE, RESIZED_MAP = A.UHDR_HIP_APPLY_GAMMA_TABLE, A.UHDR_HIP_APPLY_RESIZED_MAP
INVALID, UNSUPPORTED = A.UHDR_CODEC_INVALID_PARAM, A.UHDR_CODEC_UNSUPPORTED_FEATURE

K_BLOCK, K_QUADS_PER_LANE, K_MAX_IDW_SCALE, K_MAX_BATCH = 256, 2, 8, 16  # kBlock, kQuadsPerLane, kMaxIdwScaleLds, kMaxBatchFrames

# (file under libultrahdr_amd/csrc, text): what the functions below restate
MIRRORED = [
    # apply_quad_mode
    ("apply_gainmap.hip", "if (p.resize_on) return -1;  // the resizing sampler exists in the generic kernel only"),
    ("apply_gainmap.hip", "const size_t out_bytes = out == 0 ? 8 : 4;"),
    ("apply_gainmap.hip", "if (p.sdr.fmt == UHDR_IMG_FMT_12bppYCbCr420 || p.sdr.fmt == UHDR_IMG_FMT_16bppYCbCr422) {"),
    ("apply_gainmap.hip", "base_ok = (p.sdr.stride[0] % 2 == 0) && aligned_to(p.sdr.p[0], 2) && fits32(0) && fits32(1) && fits32(2);"),
    ("apply_gainmap.hip", "base_ok = (p.sdr.stride[0] % 2 == 0) && (p.sdr.stride[1] % 2 == 0) && (p.sdr.stride[2] % 2 == 0) &&"),
    ("apply_gainmap.hip", "aligned_to(p.sdr.p[0], 2) && aligned_to(p.sdr.p[1], 2) && aligned_to(p.sdr.p[2], 2) && fits32(0) && fits32(1) && fits32(2);"),
    ("apply_gainmap.hip", "base_ok = (p.sdr.stride[0] % 2 == 0) && aligned_to(p.sdr.p[0], 8) && (uint64_t)p.sdr.stride[0] * 4 * p.sdr.h < 0xFFFFFFFFull;"),
    ("apply_gainmap.hip", "const bool quad = base_ok && (p.sdr.w % 2 == 0) && (p.sdr.h % 2 == 0) &&"),
    ("apply_gainmap.hip", "(p.y0 % 2 == 0) &&"),
    ("apply_gainmap.hip", "aligned_to(p.dst.p[0], 16) && ((p.dst.stride[0] * out_bytes) % 16 == 0) &&"),
    ("apply_gainmap.hip", "p.sdr.w < 65536 && (p.sdr.h + p.y0) < 65536 && p.sdr.w >= 128 &&"),
    ("apply_gainmap.hip", "if (out != 0 && (!p.oetf_buckets || p.oetf_n == 0)) return -1;  // HLG / PQ: the verified output-code bucket table"),
    ("apply_gainmap.hip", "if (p.gm.w < p.sdr.w || p.gm.h < p.sdr.h + p.y0) return -1;"),
    ("apply_gainmap.hip", "if (mapfmt == 0 && !(p.gm.stride[0] % 2 == 0 && aligned_to(p.gm.p[0], 2))) return -1;"),
    ("apply_gainmap.hip", "if (mapfmt == 1 && !((p.gm.stride[0] * 3) % 2 == 0 && aligned_to(p.gm.p[0], 2))) return -1;"),
    ("apply_gainmap.hip", "if (mapfmt == 2 && !(p.gm.stride[0] % 2 == 0 && aligned_to(p.gm.p[0], 8))) return -1;"),
    ("apply_gainmap.hip", "if (p.scale >= 2 && p.scale % 2 == 0 && p.scale <= (uint32_t)kMaxIdwScaleLds && p.gamma_is_one[0] &&"),
    ("apply_gainmap.hip", "p.gamma_is_one[1] && p.gamma_is_one[2])"),
    ("apply_gainmap.hip", "if (p.gamma_thr && p.gamma_same && !p.gamma_is_one[0] && !p.resize_on && p.scale >= 2 && p.scale % 2 == 0 && p.scale <= (uint32_t)kMaxIdwScaleLds) return 2;"),
    ("uhdr_types.h", "constexpr int kMaxIdwScaleLds = 8;"),
    # apply_gamma_route
    ("apply_gainmap.hip", "if (!p.gamma_thr || (p.gamma_is_one[0] && p.gamma_is_one[1] && p.gamma_is_one[2])) return 0;"),
    ("apply_gainmap.hip", "return smode == 2 ? 1 : (smode < 0 ? 2 : 0);"),
    # launch_apply_gainmap
    ("apply_gainmap.hip", "if (smode >= 0) return launch_quad_o<0>(p, out, base_index(p), mapfmt_index(p), smode, s);"),
    ("apply_gainmap.hip", "if (p.n_frames > 1) return hipErrorInvalidValue;"),
    ("apply_gainmap.hip", "const size_t total = (size_t)((p.sdr.w + kBlock - 1) / kBlock) * p.sdr.h;  // tiles"),
    ("apply_gainmap.hip", "int grid = (int)min(total, (size_t)2048);"),
    ("apply_gainmap.hip", "if (apply_gamma_route(p) == 2) {  // gamma != 1 at a scale other than 1, through the threshold table"),
    # the entry points of the quad kernel and launch_quad
    ("apply_gainmap.hip", "template <int OUT> constexpr int quad_block() { return OUT == 0 ? kBlock : 768; }"),
    ("apply_gainmap.hip", "template <int SMODE, int SRC> constexpr int quad_sgprs() { return (SMODE == 0 && SRC == 0) ? 80 : 96; }"),
    ("apply_gainmap.hip", "constexpr bool kSpills = !k80 && OUT != 0 && MAPFMT != 0 && SMODE != 0;  // see apply_quad_kernel_s96w3"),
    ("apply_gainmap.hip", "constexpr int kQuadsPerLane = 2;"),
    ("apply_gainmap.hip", "constexpr int kOversub = 1;"),
    ("apply_gainmap.hip", "if (per_cu > 8) per_cu = 8;"),
    ("apply_gainmap.hip", "return per_cu * cus;"),
    ("apply_gainmap.hip", "const uint32_t strips_x = (p.sdr.w / 2 + 64 * kQuadsPerLane - 1) / (64 * kQuadsPerLane), qh = p.sdr.h / 2;"),
    ("apply_gainmap.hip", "if (BASE == 0 && SMODE != 0 && n_frames == 1 && (size_t)p.sdr.w * p.sdr.h >= (size_t)3840 * 2160 && p.sdr.stride[1] == p.sdr.stride[2] &&"),
    ("apply_gainmap.hip", "const uint32_t max_waves = ((uint32_t)resident - pf) * (BLK / 64) * over;"),
    ("apply_gainmap.hip", "uint32_t groups = max_waves / (strips_x * n_frames);"),
    ("apply_gainmap.hip", "if (groups > qh) groups = qh;"),
    ("apply_gainmap.hip", "if (groups < 1) groups = 1;"),
    ("apply_gainmap.hip", "q.tiles_per_wave = (qh + groups - 1) / groups;  // quad rows per wave"),
    # the quad kernel's own geometry
    ("apply_gainmap.hip", "col[hq] = make_col(SRC == 0 ? (min((sx * kQuadsPerLane + hq) * 64, qw - 64) + lane) * 2 : lane * 2);  // SRC 1: set per tile"),
    ("apply_gainmap.hip", "qy_ = min(qy_, qh - 1);  // past the end: recompute the last row (identical bytes)"),
    ("apply_gainmap.hip", "if ((yg + k) < gmh1) {  // wave-uniform"),
    ("apply_gainmap.hip", "const uint32_t yu = min(yl + 1, gmh1);"),
    ("apply_gainmap.hip", "const uint32_t xu = min(xl + 1, gmw1);"),
    # build_apply_params
    ("api_gainmap.cpp", "const unsigned int whole_h = full_height ? full_height : sdr->h;"),
    ("api_gainmap.cpp", "if (full_height == 0 && y0 != 0)"),
    ("api_gainmap.cpp", "if ((uint64_t)y0 + sdr->h > whole_h)"),
    ("api_gainmap.cpp", "const float pa = (float)sdr->w / whole_h, ga = (float)gm->w / gm->h;"),
    ("api_gainmap.cpp", "if (fabsf(pa - ga) / pa > 0.01f) resized = true;"),
    ("api_gainmap.cpp", "if (resized && !resize_in_kernel)"),
    ("api_gainmap.cpp", "const float msf = resized ? 1.0f : (float)sdr->w / gm->w;"),
    ("api_gainmap.cpp", "const bool use_table = (msf == floorf(msf));"),
    ("api_gainmap.cpp", "p.scale = use_table ? (uint32_t)msf : 0u;"),
    ("api_gainmap.cpp", "p.resize_on = 1;"),
    ("api_gainmap.cpp", "const bool single = host::metadata_channels_identical(*md);"),
    ("api_gainmap.cpp", "p.gamma_inv[i] = 1.0f / md->gamma[k];"),
    ("api_gainmap.cpp", "p.gamma_is_one[i] = p.gamma_inv[i] == 1.0f ? 1 : 0;"),
    ("api_gainmap.cpp", "p.gamma_same = (!memcmp(&p.gamma_inv[0], &p.gamma_inv[1], 4) && !memcmp(&p.gamma_inv[0], &p.gamma_inv[2], 4)) ? 1 : 0;"),
    ("api_gainmap.cpp", "UHDR_TRY(get_apply_tables(c, *md, weight, use_table ? (int)p.scale : msf_rnd, &p.tables, gamma_table ? &p.gamma_thr : nullptr));"),
    # the batch entry point
    ("api_gainmap.cpp", "!memcmp(sdr[i].stride, sdr[0].stride, sizeof sdr[0].stride) && gm[i].stride[0] == gm[0].stride[0] &&"),
    ("api_gainmap.cpp", "if (n == 1 || !uniform || apply_quad_mode(p) < 0) {  // no batch kernel for this combination: frame by frame"),
    # the fused route of the _any entry points
    ("api_gainmap.cpp", "if (!strcmp(e, \"fused\")) return false;"),
]

# conjuncts no caller of the C ABI can flip: (conjunct, what keeps it, file, the host line that says so)
UNREACHABLE = [
    ("p.gm.w < p.sdr.w (scale 1)", "at scale 1 the map is as wide as the base image: the scale IS sdr.w / gm.w", "api_gainmap.cpp",
     "const float msf = resized ? 1.0f : (float)sdr->w / gm->w;"),
    ("!map_even (the 8-byte load of an RGB888 map at an odd row pitch)", "the predicate sends an RGB888 map with an odd stride to the generic kernel",
     "apply_gainmap.hip", "if (mapfmt == 1 && !((p.gm.stride[0] * 3) % 2 == 0 && aligned_to(p.gm.p[0], 2))) return -1;"),
    ("p.sdr.w < 65536 && (p.sdr.h + p.y0) < 65536", "build_apply_params refuses such an image at every integer scale, and a non-integer scale is the generic kernel's",
     "api_gainmap.cpp", "if (use_table && (sdr->w >= 65536 || (uint64_t)sdr->h + y0 >= 65536))"),
    ("fits32(plane)", "a base plane of 4 GiB: reachable, but only with an allocation no test makes (stride x (h + 1) >= 2^32 - 1)", "apply_gainmap.hip",
     "auto fits32 = [&](int pl) { return (uint64_t)p.sdr.stride[pl] * ((uint64_t)p.sdr.h + 1) < 0xFFFFFFFFull; };"),
    ("dst.stride[0] * out_bytes * sdr.h < 2^32 - 1", "a destination of 4 GiB: reachable, but only with an allocation no test makes", "apply_gainmap.hip",
     "(uint64_t)p.dst.stride[0] * out_bytes * p.sdr.h < 0xFFFFFFFFull &&"),
    ("gm.stride[0] * gm.h * 4 < 2^32 - 1", "a map of 1 GiB: reachable, but only with an allocation no test makes", "apply_gainmap.hip",
     "(uint64_t)p.gm.stride[0] * p.gm.h * 4 < 0xFFFFFFFFull;"),
    ("!p.oetf_buckets || p.oetf_n == 0 (HLG / PQ)", "the host sets both whenever its bucket table verified itself, and it does with the libm the library is built "
     "against (the quad profile families that tests/test_gpu_apply_gamma.py counts for HLG and PQ pin it on the device)",
     "api_gainmap.cpp", "if (b.exact) {  // otherwise the quad kernel is not offered this transfer (apply_quad_mode) and the generic kernel runs"),
    ("p.scale >= 2 (scale != 1)", "an integer scale is at least 1 (msf_rnd and the table scale come from sdr.w / gm.w >= 1 after the guard), and 0 stands for a "
     "non-integer ratio, which the `scale integer` conjunct below covers", "api_gainmap.cpp", "p.scale = use_table ? (uint32_t)msf : 0u;"),
    ("!p.resize_on inside the SMODE 2 line", "apply_quad_mode has returned for resize_on before", "apply_gainmap.hip",
     "if (p.resize_on) return -1;  // the resizing sampler exists in the generic kernel only"),
    ("p.n_frames > 1 on the generic route", "the batch entry point asks apply_quad_mode first and goes frame by frame", "api_gainmap.cpp",
     "if (n == 1 || !uniform || apply_quad_mode(p) < 0) {  // no batch kernel for this combination: frame by frame"),
]

Layout = namedtuple("Layout", "fmt strides offsets")
# entry: "dev", "ex_dev", "any_dev" or "batch_dev".  base / gm / dst: the Layout of each image's FRAME.  opt: stripe (the call gets
# views of rows [y0, y0 + h) of frames that hold full_h rows), n (frames of a batch), second_gm_stride (the map stride of a batch's
# second frame), ubc / map_cg (use_base_cg and the map's gamut), flip_of / flips (first table), family (second table)
Case = namedtuple("Case", "name entry w h y0 full_h base gm dst gm_w gm_h out_ct gamma flags opt")


def lay(fmt, strides, offsets):
    return Layout(fmt, tuple(strides), tuple(offsets))


def out_fmt(ct):
    return F16 if ct == LINEAR else R1010102


def out_index(ct):
    return {LINEAR: 0, HLG: 1, PQ: 2}[ct]


def mapfmt_index(fmt):
    return {Y400: 0, RGB: 1, RGBA: 2}[fmt]


def base_index(fmt):
    return {S420: 0, S444: 1, S422: 3}.get(fmt, 2)


def bytes_per_sample(fmt):
    return {RGB: 3, RGBA: 4, R1010102: 4, F16: 8}.get(fmt, 1)


# ---- build_apply_params, restated -------------------------------------------------------------------------------------------------------
f32 = np.float32


def needs_resize(w, whole_h, gm_w, gm_h):
    """The 1 % aspect guard, in float32 as written."""
    pa, ga = f32(w) / f32(whole_h), f32(gm_w) / f32(gm_h)
    return bool(np.abs(pa - ga) / pa > f32(0.01))


Params = namedtuple("Params", "refused scale resize_on gamma_is_one gamma_same gamma_thr")


def params(c):
    """What build_apply_params makes of a case: a refusal code, or the scale (0: not an integer), resize_on, the gamma fields."""
    whole_h = c.full_h if c.full_h else c.h
    if c.dst.strides[0] < c.w:
        return Params(INVALID, 0, False, None, None, None)
    if c.full_h == 0 and c.y0 != 0:
        return Params(INVALID, 0, False, None, None, None)
    if c.y0 + c.h > whole_h:
        return Params(INVALID, 0, False, None, None, None)
    resized = needs_resize(c.w, whole_h, c.gm_w, c.gm_h)
    if resized and not (c.flags & RESIZED_MAP):
        return Params(UNSUPPORTED, 0, False, None, None, None)
    msf = f32(1.0) if resized else f32(c.w) / f32(c.gm_w)
    scale = int(msf) if msf == np.floor(msf) else 0
    # (the three channels of the tables' metadata differ in their boosts when the map has three channels, so gamma k is channel k's)
    inv = [f32(1.0) / f32(g) for g in c.gamma]
    is_one = tuple(bool(v == f32(1.0)) for v in inv)
    same = bool(inv[0] == inv[1] == inv[2])
    # (the gammas of this module's cases have verified threshold tables: tests/test_gamma_index_table.py)
    thr = bool(c.flags & GAMMA_TABLE)
    return Params(None, scale, resized, is_one, same, thr)


def effective(c):
    """(base, gm, dst) as the call hands them over: the frames' layouts, the bases moved down to row y0 for a stripe."""
    if not c.opt.get("stripe"):
        return c.base, c.gm, c.dst
    def down(layout, rows_of):
        bps = bytes_per_sample(layout.fmt)
        return layout._replace(offsets=tuple(o + rows_of(i) * s * bps for i, (o, s) in enumerate(zip(layout.offsets, layout.strides))))
    sub = c.base.fmt == S420
    return down(c.base, lambda i: c.y0 // 2 if (sub and i) else c.y0), c.gm, down(c.dst, lambda i: c.y0)


# ---- apply_quad_mode, restated ------------------------------------------------------------------------------------------------------------
def conjuncts(c):
    """[(name, holds)] of the quad kernel's contract for case c, in the order apply_quad_mode asks; every one true: the quad kernel."""
    p = params(c)
    assert p.refused is None, c.name
    base, gm, dst = effective(c)
    out = [("!resize_on", not p.resize_on)]
    s, o = base.strides, base.offsets
    if base.fmt in (S420, S422):
        out += [("sdr.stride[0] % 2", s[0] % 2 == 0), ("al(sdr.p[0], 2)", o[0] % 2 == 0)]
    elif base.fmt == S444:
        out += [(f"sdr.stride[{i}] % 2", s[i] % 2 == 0) for i in range(3)] + [(f"al(sdr.p[{i}], 2)", o[i] % 2 == 0) for i in range(3)]
    elif base.fmt == RGBA:
        out += [("sdr.stride[0] % 2", s[0] % 2 == 0), ("al(sdr.p[0], 8)", o[0] % 8 == 0)]
    else:
        out += [("base format", False)]
    ob = 8 if c.out_ct == LINEAR else 4
    out += [("sdr.w % 2", c.w % 2 == 0), ("sdr.h % 2", c.h % 2 == 0), ("y0 % 2", c.y0 % 2 == 0), ("al(dst.p[0], 16)", dst.offsets[0] % 16 == 0),
            ("dst pitch % 16", (dst.strides[0] * ob) % 16 == 0), ("sdr.w >= 128", c.w >= 128)]
    if p.scale == 1:
        out += [("gm.h >= sdr.h + y0", c.gm_h >= c.h + c.y0)]
        if gm.fmt == Y400:
            out += [("gm.stride[0] % 2", gm.strides[0] % 2 == 0), ("al(gm.p[0], 2)", gm.offsets[0] % 2 == 0)]
        elif gm.fmt == RGB:
            out += [("(gm.stride[0] * 3) % 2", (gm.strides[0] * 3) % 2 == 0), ("al(gm.p[0], 2)", gm.offsets[0] % 2 == 0)]
        else:
            out += [("gm.stride[0] % 2", gm.strides[0] % 2 == 0), ("al(gm.p[0], 8)", gm.offsets[0] % 8 == 0)]
        return out
    out += [("scale integer", p.scale != 0), ("scale % 2", p.scale % 2 == 0), ("scale <= 8", p.scale <= K_MAX_IDW_SCALE)]
    if all(p.gamma_is_one):
        return out
    return out + [("gamma_thr", p.gamma_thr), ("gamma_same", p.gamma_same), ("!gamma_is_one[0]", not p.gamma_is_one[0])]


def quad_mode(c):
    """apply_quad_mode: the SMODE, or -1."""
    if not all(v for _, v in conjuncts(c)):
        return -1
    p = params(c)
    return 0 if p.scale == 1 else (1 if all(p.gamma_is_one) else 2)


def gamma_route(c):
    p = params(c)
    if not p.gamma_thr or all(p.gamma_is_one):
        return 0
    smode = quad_mode(c)
    return 1 if smode == 2 else (2 if smode < 0 else 0)


def quad_entry(out, mapfmt, smode):
    """launch_quad's choice among the three __global__ entry points."""
    if smode == 0:
        return "apply_quad_kernel"  # 80 SGPRs
    return "apply_quad_kernel_s96w3" if (out != 0 and mapfmt != 0) else "apply_quad_kernel_s96"


POW_ROUTE = "pow per sample"


def route(c):
    """What case c selects: ("refused", code); (entry point, (OUT, MAPFMT, SMODE, BASE)) of the quad kernel, with "frame table" behind
    it for a batch launch; or the generic kernel's form and its sampler.  A gamma != 1 that reaches the generic kernel without its
    table is POW_ROUTE, which no case of this module takes (tests/test_gpu_parity.py keeps its allowance)."""
    p = params(c)
    if p.refused is not None:
        return ("refused", p.refused)
    out = out_index(c.out_ct)
    smode = quad_mode(c)
    if smode >= 0:
        r = (quad_entry(out, mapfmt_index(c.gm.fmt), smode), (out, mapfmt_index(c.gm.fmt), smode, base_index(c.base.fmt)))
        if c.entry == "batch_dev" and c.opt.get("n", 1) > 1 and batch_uniform(c):
            r += ("frame table",)
        return r
    sampler = "resizing sampler" if p.resize_on else ("table sampler" if p.scale else "distance sampler")
    if gamma_route(c) == 2:
        return (f"apply_generic_kernel<{out}, 1>", sampler)
    if not all(p.gamma_is_one) and p.scale != 1:
        return (f"apply_generic_kernel<{out}>", sampler, POW_ROUTE)
    return (f"apply_generic_kernel<{out}>", sampler)


def batch_uniform(c):
    """The batch entry point's own test of frames 1 .. n - 1 (the frames of a case share everything but opt["second_gm_stride"])."""
    base, gm, dst = effective(c)
    return ("second_gm_stride" not in c.opt and base.offsets[0] % 2 == 0 and dst.offsets[0] % 16 == 0 and gm.offsets[0] % 8 == 0 and
            base.fmt in (S420, S422, S444))


# every route the tables have to reach
QUAD_ROUTES = [(o, s) for o in (0, 1, 2) for s in (0, 1, 2)]  # every (OUT, SMODE)
ENTRY_POINTS = ["apply_quad_kernel", "apply_quad_kernel_s96", "apply_quad_kernel_s96w3"]
GENERIC_FORMS = ["apply_generic_kernel<%d>" % o for o in (0, 1, 2)] + ["apply_generic_kernel<%d, 1>" % o for o in (0, 1, 2)]


# ---- launch_quad, restated ------------------------------------------------------------------------------------------------------------------
def quad_block(out):
    return K_BLOCK if out == 0 else 768


def strips_of(w):
    return (w // 2 + 64 * K_QUADS_PER_LANE - 1) // (64 * K_QUADS_PER_LANE)


def row_groups(cus, per_cu, blk, strips_x, qh, n_frames=1, pf=0, over=1):
    """(groups, tiles_per_wave, workgroups) of launch_quad."""
    resident = per_cu * cus
    max_waves = (resident - pf) * (blk // 64) * over
    groups = max_waves // (strips_x * n_frames)
    groups = max(1, min(groups, qh))
    nwaves = groups * strips_x * n_frames
    return groups, (qh + groups - 1) // groups, (nwaves + blk // 64 - 1) // (blk // 64) + pf


def row_group_condition(cus, blk, w, h, n_frames=1):
    """For every answer of the occupancy query from 1 to 8 workgroups per compute unit: fewer row groups than quad rows, and a number
    of them that does not divide the quad rows -- some waves then own one quad row fewer than tiles_per_wave says, and their look-ahead
    row is the clamped, recomputed last one."""
    qh = h // 2
    return all(g < qh and qh % g != 0 for g in (row_groups(cus, k, blk, strips_of(w), qh, n_frames)[0] for k in range(1, 9)))


def row_group_shape(cus, blk, w=130):
    """-> (h, n_frames): the smaller of a single w-wide frame and a batch of sixteen such frames at which row_group_condition holds.
    Both come to the same number of waves, so to the same number of pixels give or take a row: the single frame is taken on a tie."""
    best = None
    for n in (1, K_MAX_BATCH):
        h = 2 * (8 * cus * (blk // 64) // (strips_of(w) * n)) + 2
        while not row_group_condition(cus, blk, w, h, n):
            h += 2
        if best is None or h * n < best[0] * best[1]:
            best = (h, n)
    return best


def generic_grid(w, h):
    tiles = ((w + K_BLOCK - 1) // K_BLOCK) * h
    return max(1, min(tiles, 2048)), tiles


# ---- the first table: every reachable conjunct, true and false ------------------------------------------------------------------------------
G1 = (1.0, 1.0, 1.0)


def _put(t, i, v):
    t = list(t)
    t[i] = v
    return tuple(t)


def _dst(ct, w, stride=None, off=48):
    """An awkward legal destination: rows of a whole number of 16 bytes just above the width, the base 48 bytes past a 256-byte boundary."""
    if stride is None:
        k = 2 if ct == LINEAR else 4
        stride = (w // k + 1) * k
    return lay(out_fmt(ct), (stride,), (off,))


def _base(fmt, w):
    """An awkward legal base image: what the predicate leaves alone is odd (the chroma strides and bases of 4:2:0 / 4:2:2)."""
    e = w + 2 + w % 2  # the smallest even stride above the width
    c = (w + 1) // 2
    if fmt in (S420, S422):
        return lay(fmt, (e, c + 1 + c % 2, c + 3 + c % 2), (2, 1, 3))  # odd chroma strides, odd chroma bases, luma 2 (mod 4)
    if fmt == S444:
        return lay(fmt, (e, e + 2, e + 4), (2, 6, 10))
    if fmt == RGBA:
        return lay(fmt, (e,), (8,))
    return lay(fmt, (w + 1,), (1,))


def _map(fmt, gm_w, scale1):
    """An awkward legal map: at scale 1 an even stride just above the width and the least alignment its loads need; at any other
    scale, where the kernel reads bytes, an odd stride and an odd base."""
    if scale1:
        return lay(fmt, (gm_w + 2 - gm_w % 2,), (8 if fmt == RGBA else 2,))
    return lay(fmt, (gm_w + 1 + gm_w % 2,), (4 if fmt == RGBA else 1,))


def make(name, entry, fmt, w, h, gm_fmt, scale, ct, gamma=G1, flags=0, y0=0, full_h=0, gm_w=None, gm_h=None, base=None, gm=None, dst=None, **opt):
    whole_h = full_h if full_h else h
    gm_w = w // scale if gm_w is None else gm_w
    gm_h = whole_h // scale if gm_h is None else gm_h
    return Case(name, entry, w, h, y0, full_h, base or _base(fmt, w), gm or _map(gm_fmt, gm_w, scale == 1 and not opt.get("bytewise_map")),
                dst or _dst(ct, w), gm_w, gm_h, ct, tuple(gamma), flags, opt)


def _flip(anchor, what, **kw):
    """The anchor with one thing changed: w / h / y0 / full_h / gm_w / gm_h / gamma / flags / entry given, or an image's layout through
    base_stride=(plane, value), base_off, gm_stride, gm_off, dst_stride, dst_off."""
    c = anchor
    tag = []
    for key in ("w", "h", "y0", "full_h", "gm_w", "gm_h", "gamma", "flags", "entry", "base", "gm", "dst"):
        if key in kw:
            c = c._replace(**{key: kw[key]})
            tag.append(f"{key}={kw[key]}" if key not in ("base", "gm", "dst") else key)
    for image in ("base", "gm", "dst"):
        layout = getattr(c, image)
        if image + "_stride" in kw:
            i, v = kw[image + "_stride"]
            layout = layout._replace(strides=_put(layout.strides, i, v))
            tag.append(f"{image}.stride[{i}]={v}")
        if image + "_off" in kw:
            i, v = kw[image + "_off"]
            layout = layout._replace(offsets=_put(layout.offsets, i, v))
            tag.append(f"{image}.p[{i}]+{v}")
        c = c._replace(**{image: layout})
    return c._replace(name=f"{anchor.name}/{kw.get('tag') or ','.join(tag)}", opt=dict(anchor.opt, flip_of=anchor.name, flips=what, **kw.get("opt", {})))


G_ONE, G_THREE = (1.571, 1.571, 1.571), (1.3, 1.7, 2.2)


def slack_rows(w, scale):
    """The smallest h, a multiple of 2 and of the scale, at which a map of w / scale columns may have one row fewer AND one row more
    than h / scale without leaving the 1 % aspect guard."""
    h = 2 * scale if scale % 2 == 0 else 2
    step = scale if scale % 2 == 0 else 2 * scale
    while h // scale < 2 or needs_resize(w, h, w // scale, h // scale - 1) or needs_resize(w, h, w // scale, h // scale + 1):
        h += step
    return h


def _cases():
    cs = []
    # -- the anchors at scale 1 (SMODE 0, the 80-SGPR entry point): one per base format, the three map formats and outputs among them
    a420 = make("420/y400/s1/linear", "dev", S420, 130, 6, Y400, 1, LINEAR)
    a422 = make("422/rgb888/s1/hlg", "dev", S422, 130, 6, RGB, 1, HLG, ubc=0, map_cg=A.UHDR_CG_BT_2100)
    a444 = make("444/rgba8888/s1/pq", "dev", S444, 130, 6, RGBA, 1, PQ)
    argba = make("rgba/y400/s2/linear", "dev", RGBA, 130, 6, Y400, 2, LINEAR)
    cs += [a420, a422, a444, argba]
    # what every base format shares, on the 4:2:0 anchor
    cs += [_flip(a420, "sdr.w % 2", w=131, gm_w=131),
           _flip(a420, "sdr.h % 2", h=7, gm_h=7),
           _flip(a420, "sdr.w >= 128", w=126, gm_w=126),
           _flip(a420, "y0 % 2", y0=1, full_h=7, gm_h=7, tag="y0=1"),
           _flip(a420, "!resize_on", entry="any_dev", flags=RESIZED_MAP, gm_w=40, gm_h=7, gm=lay(Y400, (42,), (2,)), tag="any_dev,map=40x7")]
    # the base image's own conjuncts, per format
    for a in (a420, a422):
        cs += [_flip(a, "sdr.stride[0] % 2", base_stride=(0, a.base.strides[0] + 1)), _flip(a, "al(sdr.p[0], 2)", base_off=(0, 3))]
    for i in range(3):
        cs += [_flip(a444, f"sdr.stride[{i}] % 2", base_stride=(i, a444.base.strides[i] + 1)), _flip(a444, f"al(sdr.p[{i}], 2)", base_off=(i, 2 * i + 1))]
    cs += [_flip(argba, "sdr.stride[0] % 2", base_stride=(0, 133)), _flip(argba, "al(sdr.p[0], 8)", base_off=(0, 4))]
    cs.append(make("rgb888/y400/s1/linear", "dev", RGB, 130, 6, Y400, 1, LINEAR, flip_of=a420.name, flips="base format"))
    # the destination's, per output format (16-byte rows: an even stride of half floats, a multiple of four RGBA1010102 pixels)
    cs += [_flip(a420, "dst pitch % 16", dst_stride=(0, 133)), _flip(a420, "al(dst.p[0], 16)", dst_off=(0, 56)),
           _flip(a422, "dst pitch % 16", dst_stride=(0, 134)), _flip(a422, "al(dst.p[0], 16)", dst_off=(0, 52)),
           _flip(a444, "dst pitch % 16", dst_stride=(0, 133)), _flip(a444, "al(dst.p[0], 16)", dst_off=(0, 56))]
    # the map's at scale 1, per map format
    cs += [_flip(a420, "gm.stride[0] % 2", gm_stride=(0, 131)), _flip(a420, "al(gm.p[0], 2)", gm_off=(0, 3)),
           _flip(a422, "(gm.stride[0] * 3) % 2", gm_stride=(0, 131)), _flip(a422, "al(gm.p[0], 2)", gm_off=(0, 1)),
           _flip(a444, "gm.stride[0] % 2", gm_stride=(0, 131)), _flip(a444, "al(gm.p[0], 8)", gm_off=(0, 4))]
    # ... and its height, at the smallest size at which a map one row short still passes the aspect guard
    hs = slack_rows(130, 1)
    tall = make(f"420/y400/s1/linear/h={hs}", "dev", S420, 130, hs, Y400, 1, LINEAR)
    cs += [tall, _flip(tall, "gm.h >= sdr.h + y0", gm_h=hs - 1)]
    # a gamma other than 1 at scale 1 is folded into the byte -> factor table: the same route with and without the flag
    cs += [make("420/rgb888/s1/linear/gamma", "dev", S420, 130, 6, RGB, 1, LINEAR, gamma=G_ONE),
           make("420/rgb888/s1/pq/gamma+flag", "ex_dev", S420, 130, 6, RGB, 1, PQ, gamma=G_THREE, flags=GAMMA_TABLE)]
    # -- the scale side: SMODE 1 at scales 2 / 4 / 8 (the RGBA anchor above is scale 2), one anchor per output
    s4 = make("420/y400/s4/hlg", "dev", S420, 132, 12, Y400, 4, HLG)                       # _s96
    s8 = make("444/rgb888/s8/pq", "dev", S444, 136, 8, RGB, 8, PQ, ubc=0, map_cg=A.UHDR_CG_BT_2100)  # _s96w3
    s2 = make("422/rgba8888/s2/hlg", "dev", S422, 130, 6, RGBA, 2, HLG)                      # _s96w3
    cs += [s4, s8, s2]
    cs += [make("420/y400/s3/hlg", "dev", S420, 132, 12, Y400, 3, HLG, flip_of=s4.name, flips="scale % 2"),
           make("420/y400/s16/hlg", "dev", S420, 144, 16, Y400, 16, HLG, flip_of=s4.name, flips="scale <= 8"),
           make("420/y400/s2.5/hlg", "dev", S420, 130, 10, Y400, 1, HLG, gm_w=52, gm_h=4, bytewise_map=True, flip_of=s4.name, flips="scale integer"),
           make("rgba/y400/s3/linear", "dev", RGBA, 132, 6, Y400, 3, LINEAR, flip_of=argba.name, flips="scale % 2"),
           make("444/rgb888/s16/pq", "dev", S444, 144, 16, RGB, 16, PQ, flip_of=s8.name, flips="scale <= 8")]
    # -- SMODE 2: one gamma != 1 for the three channels, with the flag; one anchor per output
    g0 = make("420/rgb888/s2/linear/gamma+flag", "ex_dev", S420, 130, 6, RGB, 2, LINEAR, gamma=G_ONE, flags=GAMMA_TABLE)  # _s96
    g1 = make("420/rgb888/s4/hlg/gamma+flag", "ex_dev", S420, 132, 12, RGB, 4, HLG, gamma=G_ONE, flags=GAMMA_TABLE)      # _s96w3
    g2 = make("rgba/rgba8888/s2/pq/gamma+flag", "ex_dev", RGBA, 130, 6, RGBA, 2, PQ, gamma=(0.8, 0.8, 0.8), flags=GAMMA_TABLE)  # _s96w3
    cs += [g0, g1, g2, make("422/y400/s8/pq/gamma+flag", "ex_dev", S422, 136, 8, Y400, 8, PQ, gamma=G_ONE, flags=GAMMA_TABLE)]        # _s96
    for a in (g0, g1, g2):  # three gammas (the maps have three channels): the generic kernel's table form
        cs.append(_flip(a, "gamma_same", gamma=G_THREE, tag="three-gammas"))
    return cs


CASES = _cases()

# `gamma_thr` false with a gamma != 1 at a scale other than 1 is the pow per sample (POW_ROUTE), and `!gamma_is_one[0]` false beside a
# channel whose gamma is not 1 needs gamma_same false as well: neither has a pair in this table
NO_PAIR = {"gamma_thr": "the pow-per-sample route keeps its allowance in tests/test_gpu_parity.py", "!gamma_is_one[0]": "implied by gamma_same beside a gamma != 1"}


# ---- the second table: the quad kernel's geometry, the generic kernel's loop ------------------------------------------------------------------
EDGE_WIDTHS, EDGE_HEIGHTS = (128, 130, 254, 256, 258, 514), (2, 4, 6, 136)


def _geometry():
    gs = []
    fmts, maps, cts = (S420, S422, S444, RGBA), (Y400, RGB, RGBA), (LINEAR, HLG, PQ)
    k = 0
    # widths at which strips_x is 1, 2 and 3 and the last strip is whole, two pixels or half full; heights of one, two and three quad rows
    # (`groups > qh`) and one in the hundreds; at scale 1 and at the largest of 8 / 4 / 2 that divides both
    for w in EDGE_WIDTHS:
        for h in EDGE_HEIGHTS:
            for scale in (1, next(s for s in (8, 4, 2) if w % s == 0 and h % s == 0)):
                gs.append(make(f"edge/{w}x{h}/s{scale}", "dev", fmts[k % 4], w, h, maps[(k // 2) % 3], scale, cts[k % 3], family="edge"))
                k += 1
    # map rows with slack: one row fewer and one row more than h / scale, at the smallest h the aspect guard lets pass
    for scale, w, fmt, gm_fmt, ct in ((1, 130, S420, RGB, LINEAR), (2, 130, S422, Y400, PQ), (4, 132, S444, RGBA, LINEAR), (8, 136, S420, RGB, HLG)):
        h = slack_rows(w, scale)
        for d in (-1, 1):
            gs.append(make(f"slack/{w}x{h}/s{scale}/rows{d:+d}", "dev", fmt, w, h, gm_fmt, scale, ct, gm_h=h // scale + d, family="slack"))
    # the issue's own example of a height that is no multiple of the scale
    for gm_h in (125, 126):
        gs.append(make(f"slack/1024x1004/s8/map128x{gm_h}", "dev", S420, 1024, 1004, Y400, 8, LINEAR, gm_h=gm_h, family="slack"))
    # an RGB888 map at scale 1 whose last row is the last row the image reads: the exact loads of the last map row
    gs.append(make("exact/130x6/rgb888-last-row", "dev", S420, 130, 6, RGB, 1, LINEAR, family="exact"))
    gs.append(make("exact/258x4/rgb888-last-row", "dev", RGBA, 258, 4, RGB, 1, PQ, family="exact"))
    # stripes: views of rows [y0, y0 + h) inside frames of full_h rows; y0 = 2 (mod scale), two rows, the first and the last stripe
    for scale, w, full_h, fmt, gm_fmt, ct, stripes in ((4, 132, 24, S420, RGB, LINEAR, ((0, 2), (2, 2), (6, 10), (22, 2))),
                                                       (8, 136, 32, S422, Y400, PQ, ((0, 2), (10, 6), (26, 6))),
                                                       (1, 130, 12, S444, RGB, HLG, ((0, 2), (2, 4), (6, 6)))):
        for y0, h in stripes:
            gs.append(make(f"stripe/{w}x{full_h}/s{scale}/rows{y0}+{h}", "ex_dev" if scale == 8 else "dev", fmt, w, h, gm_fmt, scale, ct, y0=y0, full_h=full_h,
                           stripe=True, family="stripe"))
    # batches: three frames of one awkward layout (the frame table), and one whose second frame's map has a stride of its own (frame by frame)
    gs.append(make("batch/3x130x6/s1", "batch_dev", S420, 130, 6, RGBA, 1, LINEAR, n=3, family="batch"))
    gs.append(make("batch/3x258x4/s2", "batch_dev", S422, 258, 4, Y400, 2, PQ, n=3, gm=lay(Y400, (131,), (8,)), family="batch"))
    gs.append(make("batch/3x130x6/s1/second-stride", "batch_dev", S420, 130, 6, RGBA, 1, LINEAR, n=3, second_gm_stride=134, family="batch"))
    # the generic kernel's tile loop past its 2048 workgroups
    gs.append(make("wrap/126x2050", "dev", S420, 126, 2050, Y400, 2, LINEAR, family="wrap"))
    gs.append(make("wrap/258x1030", "dev", S420, 258, 1030, RGB, 1, PQ, base=lay(S420, (261, 131, 133), (1, 1, 3)), family="wrap"))
    return gs


GEOMETRY = _geometry()


def row_group_cases(cus):
    """The two shapes at which launch_quad hands a wave several quad rows (row_group_shape): 256-thread workgroups (F16) and 768-thread
    ones (PQ).  They depend on the device's compute units, so they are made where the count is known."""
    out = []
    for ct, gm_fmt, scale in ((LINEAR, RGBA, 1), (PQ, Y400, 2)):
        blk = quad_block(out_index(ct))
        h, n = row_group_shape(cus, blk)
        out.append(make(f"rowgroups/{cus}cus/blk{blk}/{n}x130x{h}", "batch_dev" if n > 1 else "dev", S420, 130, h, gm_fmt, scale, ct, n=n, family="rowgroups"))
    return out


# ---- calls the C ABI answers with a code ---------------------------------------------------------------------------------------------------
def _refusals():
    a = make("refused/y0-without-full-height", "dev", S420, 130, 6, Y400, 1, LINEAR, y0=1, gm_h=8)
    return [a,
            a._replace(name="refused/even-y0-without-full-height", y0=2),
            a._replace(name="refused/stripe-past-the-full-height", y0=2, full_h=6),
            make("refused/another-aspect-ratio", "dev", S420, 130, 6, Y400, 1, LINEAR, gm_w=40, gm_h=7, gm=_map(Y400, 40, False)),
            make("refused/another-aspect-ratio-ex", "ex_dev", S420, 130, 6, Y400, 1, LINEAR, gm_w=40, gm_h=7, gm=_map(Y400, 40, False), flags=GAMMA_TABLE),
            make("refused/destination-stride-below-the-width", "dev", S420, 130, 6, Y400, 1, LINEAR, dst=lay(F16, (128,), (48,)))]


REFUSALS = _refusals()

# ---- the applyGainMap launches of BASELINE.json's five configurations as bench.py lays them out: library images, strides of 64 samples,
# bases on 256 bytes.  A fix to the predicate must leave every one of them on the route written beside it
def _bench(name, w, h, gm_fmt, scale, ct, n=1):
    a = lambda v: -(-v // 64) * 64
    base = lay(S420, (a(w), a(w) // 2, a(w) // 2), (0, 0, 0))
    return make(name, "batch_dev" if n > 1 else "dev", S420, w, h, gm_fmt, scale, ct, n=n, base=base, gm=lay(gm_fmt, (a(w // scale),), (0,)),
                dst=lay(out_fmt(ct), (a(w),), (0,)))


BENCH = [(_bench("1280x720 round trip, three-channel map at scale 1", 1280, 720, RGB, 1, LINEAR), ("apply_quad_kernel", (0, 1, 0, 0))),
         (_bench("16 x 4K to linear F16, map C", 3840, 2160, RGBA, 1, LINEAR, 16), ("apply_quad_kernel", (0, 2, 0, 0), "frame table")),
         (_bench("16 x 4K to linear F16, map B", 3840, 2160, RGB, 1, LINEAR, 16), ("apply_quad_kernel", (0, 1, 0, 0), "frame table")),
         (_bench("16 x 4K to linear F16, map A", 3840, 2160, Y400, 4, LINEAR, 16), ("apply_quad_kernel_s96", (0, 0, 1, 0), "frame table")),
         (_bench("one 8K frame to linear F16, map C (the roofline figure)", 7680, 4320, RGBA, 1, LINEAR), ("apply_quad_kernel", (0, 2, 0, 0))),
         (_bench("a 2048-row stripe of a 16K frame, map A", 16384, 2048, Y400, 4, LINEAR), ("apply_quad_kernel_s96", (0, 0, 1, 0))),
         (_bench("16 x 4K to HLG RGBA1010102, map A", 3840, 2160, Y400, 4, HLG, 16), ("apply_quad_kernel_s96", (1, 0, 1, 0), "frame table"))]


def describe(cases):
    count = {}
    for c in cases:
        count[route(c)] = count.get(route(c), 0) + 1
    return "\n".join(f"{n:3d} x {r}" for r, n in sorted(count.items(), key=str))
