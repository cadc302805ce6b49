"""GPU: every case of tests/route_lattice.py through the device entry points, on views inside 0xA5 frames (tests/framed.py):
sources and destinations of the caller's own strides and base offsets, so that each launcher is pushed onto each of its kernel
routes by one conjunct of its predicate at a time.

Integer operators (convertYuv, convert_raw_input_to_ycbcr, libjpeg's colour conversions, idct_dequant, idct_dequant_rgb, fdct_quant):
the valid samples equal the oracle bit for bit on independent random bytes.  toneMap and generateGainMap: every route meets the
bar of tests/test_gpu_formats.py against the oracle (+-1 code on <= 1e-4 of the samples, metadata 1e-6 relative), and the routes
that differ only in how bytes are packed (16-bit against byte luma stores; affine_wide_kernel, affine_kernel<true> and
affine_kernel<false>) equal the aligned case bit for bit.  Every frame, of every output and every input, is intact afterwards, and
the descriptors a call rewrites equal the aligned case's.

An image of odd width or height in a subsampled format is taken as the reference's loops take it: the whole 2 x 2 quads are
converted, the last column / row stays as it was (the reference's toneMap and convert_raw_input_to_ycbcr would read past an odd
edge; their oracle runs on the even crop)."""
import ctypes as C
import functools

import numpy as np
import pytest

import framed as F
import route_lattice as RL
import test_gpu_formats as TF
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FULL = A.UHDR_CR_FULL_RANGE
UNSUPPORTED = A.UHDR_CODEC_UNSUPPORTED_FEATURE


def _params(launcher):
    cs = RL.cases_of(launcher)
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def _base_of(case):
    """The aligned case a case was derived from: the one named by what stands in front of the first '/'."""
    name = case.name.split("/")[0]
    return next(c for c in RL.cases_of(case.launcher) if c.name == name)


def _even(n):
    return n - n % 2


@functools.lru_cache(maxsize=None)
def _random(fmt, w, h, seed, cg=A.UHDR_CG_BT_709):
    """Independent random bytes in every sample of an (even-sized) host image: a sample written to a neighbour's place shows."""
    img = Image(fmt, w + w % 2, h + h % 2, cg, A.UHDR_CT_SRGB, FULL, align=2)
    img.buf[:] = np.random.default_rng(seed).integers(0, 256, img.buf.size, dtype=np.uint8)
    return img


def _frame(lay, w, h, src=None, **kw):
    return F.framed(lay.fmt, w, h, lay.strides, lay.offsets, src=src, device=DEV, **kw)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if not np.array_equal(g, w):
            ys, xs = np.nonzero(g != w)
            raise AssertionError(f"{what}: plane {i}: {ys.size} samples differ, the first at row {ys[0]}, column {xs[0]}: {g[ys[0], xs[0]]} for {w[ys[0], xs[0]]}")


_CACHE = {}


def _once(key, fn):
    """Results of the aligned cases and of the oracle: computed once, shared, never written to."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def test_the_routes_of_the_table(hip_ctx):
    print("oracle:", TF.oracle_kind())
    print(RL.describe())
    for launcher, what, name, line in RL.REFUSED:
        print(f"refused: {launcher}: {what} ({name}: `{line}`)")


# ---- convertYuv -----------------------------------------------------------------------------------------------------------------------
@_params("transform_yuv")
@pytest.mark.parametrize("enc", [(A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100), (A.UHDR_CG_DISPLAY_P3, A.UHDR_CG_BT_709)], ids=["709->2100", "p3->709"])
def test_convert_yuv(hip_ctx, case, enc):
    w, h, lay = case.w, case.h, case.a
    src = _random(lay.fmt, w, h, 101)
    want = _once(("yuv", lay.fmt, w, h, enc), lambda: L.convert_yuv(TF.oracle_kind(), F.tight(lay.fmt, w, h, src), *enc).planes_valid())
    fr = _frame(lay, w, h, src)
    before = fr.desc()
    A.check(hip_ctx.lib.uhdr_hip_convert_yuv_dev(hip_ctx.handle, C.byref(fr.raw), *enc))
    hip_ctx.synchronize()
    _same(fr.valid(), want, f"{case.name} {RL.route(case)}")
    # in place: the padding is the caller's, and so are the last column / row of an odd-sized 4:2:0 image
    F.assert_frame_intact(fr, written=(_even(w), _even(h)) if lay.fmt == RL.S420 else None, what=case.name)
    assert fr.desc() == before


# ---- convert_raw_input_to_ycbcr ---------------------------------------------------------------------------------------------------------
def _run_raw_to_ycbcr(hip_ctx, case):
    w, h = case.w, case.h
    sub = RL._rgb_sub(case)
    cg = {RL.S420: A.UHDR_CG_BT_709, RL.S444: A.UHDR_CG_DISPLAY_P3, RL.P010: A.UHDR_CG_BT_2100, RL.S444_10: A.UHDR_CG_BT_709}[case.b.fmt]
    src = _random(case.a.fmt, w, h, 103, cg)
    sfr, dfr = _frame(case.a, w, h, src), _frame(case.b, w, h)
    A.check(hip_ctx.lib.uhdr_hip_convert_raw_input_to_ycbcr_dev(hip_ctx.handle, C.byref(sfr.raw), int(sub), C.byref(dfr.raw)))
    hip_ctx.synchronize()
    hw = _even(h) if sub else h  # whole quad rows
    F.assert_frame_intact(sfr, written=(), what=case.name + " source")
    F.assert_frame_intact(dfr, written=(w, hw), what=case.name + " destination")
    return src, dfr.valid(w, hw), dfr.desc()


@_params("rgb_to_ycbcr")
def test_convert_raw_input_to_ycbcr(hip_ctx, case):
    w, h = case.w, case.h
    hw = _even(h) if RL._rgb_sub(case) else h
    src, got, desc = _run_raw_to_ycbcr(hip_ctx, case)
    want = _once(("raw", case.a.fmt, case.b.fmt, w, hw),
                 lambda: L.convert_raw_input_to_ycbcr(TF.oracle_kind(), F.tight(case.a.fmt, w, hw, src), RL._rgb_sub(case)))
    assert want.raw.fmt == case.b.fmt
    _same(got, want.planes_valid(), f"{case.name} {RL.route(case)}")
    base = _base_of(case)
    bdesc = _once(("raw-desc", base.name), lambda: _run_raw_to_ycbcr(hip_ctx, base)[2])
    assert desc[:4] == bdesc[:4] == (case.b.fmt, src.raw.cg, src.raw.ct, FULL) and desc[4:] == (w, h)


# ---- libjpeg's colour conversions -------------------------------------------------------------------------------------------------------
def _rgb888_of(img, w, h):
    bpp = 4 if img.fmt == RL.RGBA else 3
    packed = img.plane(0).view(np.uint8).reshape(img.layout[0][0], -1)[:h, : w * bpp]
    return np.ascontiguousarray(packed if bpp == 3 else packed.reshape(h, w, 4)[:, :, :3].reshape(h, w * 3))


@_params("jpeg_rgb_to_ycc")
def test_jpeg_rgb_to_ycc(hip_ctx, case):
    w, h = case.w, case.h
    src = _random(case.a.fmt, w, h, 107)
    want = _once(("rgb2ycc", case.a.fmt, w, h), lambda: L.jpeg_rgb_to_ycc_port(_rgb888_of(src, w, h), w, w, h))
    sfr, dfr = _frame(case.a, w, h, src), _frame(case.b, w, h)
    A.check(hip_ctx.lib.uhdr_hip_jpeg_rgb_to_ycc_dev(hip_ctx.handle, C.byref(sfr.raw), C.byref(dfr.raw)))
    hip_ctx.synchronize()
    _same(dfr.valid(), want, f"{case.name} {RL.route(case)}")
    F.assert_frame_intact(sfr, written=(), what=case.name + " source")
    F.assert_frame_intact(dfr, what=case.name + " destination")
    assert dfr.desc() == (RL.S444, src.raw.cg, src.raw.ct, FULL, w, h)


@_params("jpeg_ycc_to_rgb")
@pytest.mark.parametrize("variant", [0, 1], ids=["turbo", "ijg9"])
def test_jpeg_ycc_to_rgb(hip_ctx, case, variant):
    w, h = case.w, case.h
    bpp = 4 if case.b.fmt == RL.RGBA else 3
    src = _random(case.a.fmt, w, h, 109)
    t = F.tight(case.a.fmt, w, h, src)
    want = _once(("ycc2rgb", bpp, w, h, variant), lambda: L.jpeg_ycc_to_rgb_port(t.valid(0), t.valid(1), t.valid(2), out_bpp=bpp, variant=variant))
    sfr, dfr = _frame(case.a, w, h, src), _frame(case.b, w, h)
    A.check(hip_ctx.lib.uhdr_hip_jpeg_ycc_to_rgb_dev(hip_ctx.handle, C.byref(sfr.raw), variant, C.byref(dfr.raw)))
    hip_ctx.synchronize()
    _same([dfr.valid()[0].view(np.uint8).reshape(h, w * bpp)], [want], f"{case.name} {RL.route(case)}")
    F.assert_frame_intact(sfr, written=(), what=case.name + " source")
    F.assert_frame_intact(dfr, what=case.name + " destination")
    assert dfr.desc() == (case.b.fmt, src.raw.cg, src.raw.ct, FULL, w, h)


# ---- the DCT stages ---------------------------------------------------------------------------------------------------------------------
def _qt(hip_ctx, quality, chroma):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return _once(("qt", quality, chroma), lambda: UltraHdr(ctx=hip_ctx).quant_table(quality, chroma))


def _ctab(qt):
    return (C.c_uint16 * 64)(*[int(v) for v in qt])


def _coefs(hip_ctx, w, h, seed):
    """Three components of random samples on the ceil(w / 8) x ceil(h / 8) block grid: (coefficients, the oracle's planes, tables)."""
    def make():
        bw, bh = -(-w // 8), -(-h // 8)
        ql, qc = _qt(hip_ctx, 90, False), _qt(hip_ctx, 90, True)
        src = np.random.default_rng(seed).integers(0, 256, (3, bh * 8, bw * 8), dtype=np.uint8)
        coefs = [L.fdct_quant_port(np.ascontiguousarray(src[c]), bw * 8, bw, bh, ql if c == 0 else qc) for c in range(3)]
        planes = [L.idct_dequant_port(coefs[c], ql if c == 0 else qc) for c in range(3)]
        return coefs, planes, ql, qc
    return _once(("coefs", w, h, seed), make)


@_params("idct_dequant")
def test_idct_dequant(hip_ctx, case):
    import torch

    w, h = case.w, case.h
    coefs, planes, ql, _ = _coefs(hip_ctx, w, h, 113)
    dcoef = torch.from_numpy(coefs[0]).to(DEV)
    dfr = _frame(case.b, w, h)
    torch.cuda.synchronize()
    A.check(hip_ctx.lib.uhdr_hip_idct_dequant_dev(hip_ctx.handle, C.c_void_p(dcoef.data_ptr()), w // 8, h // 8, _ctab(ql), C.c_void_p(dfr.raw.planes[0]),
                                                  case.b.strides[0]))
    hip_ctx.synchronize()
    _same(dfr.valid(), [planes[0]], f"{case.name} {RL.route(case)}")
    F.assert_frame_intact(dfr, what=case.name)
    assert torch.equal(dcoef.cpu(), torch.from_numpy(coefs[0])), "the coefficients are an input"


@_params("idct_dequant_rgb")
@pytest.mark.parametrize("variant", [0, 1], ids=["turbo", "ijg9"])
def test_idct_dequant_rgb(hip_ctx, case, variant):
    """Against the four-step route of test_idct_dequant_rgb_fused_equals_four_step_route (tests/test_gpu_parity.py): three IDCTs and
    libjpeg's ycc_rgb_convert, by the oracle."""
    import torch

    w, h = case.w, case.h
    bpp = 4 if case.b.fmt == RL.RGBA else 3
    coefs, planes, ql, qc = _coefs(hip_ctx, w, h, 127)
    want = _once(("idct-rgb", w, h, bpp, variant),
                 lambda: L.jpeg_ycc_to_rgb_port(*[np.ascontiguousarray(pl[:h, :w]) for pl in planes], out_bpp=bpp, variant=variant))
    dco = [torch.from_numpy(c).to(DEV) for c in coefs]
    dfr = _frame(case.b, w, h)
    torch.cuda.synchronize()
    before = dfr.desc()
    A.check(hip_ctx.lib.uhdr_hip_idct_dequant_rgb_dev(hip_ctx.handle, *[C.c_void_p(c.data_ptr()) for c in dco], -(-w // 8), -(-h // 8), _ctab(ql), _ctab(qc),
                                                      variant, C.byref(dfr.raw)))
    hip_ctx.synchronize()
    _same([dfr.valid()[0].view(np.uint8).reshape(h, w * bpp)], [want], f"{case.name} {RL.route(case)}")
    F.assert_frame_intact(dfr, what=case.name)
    assert dfr.desc() == before[:3] + (FULL,) + before[4:]


@_params("fdct_quant")
def test_fdct_quant(hip_ctx, case):
    import torch

    w, h = case.w, case.h
    src = _random(RL.Y400, w, h, 131)
    qt = _qt(hip_ctx, 85, False)
    want = _once(("fdct", w, h), lambda: L.fdct_quant_port(np.ascontiguousarray(src.valid(0)[:h, :w]), w, w // 8, h // 8, qt))
    sfr = _frame(case.a, w, h, src)
    out = torch.full((h // 8, w // 8, 64), 0x5a5a, dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    A.check(hip_ctx.lib.uhdr_hip_fdct_quant_dev(hip_ctx.handle, C.c_void_p(sfr.raw.planes[0]), case.a.strides[0], w // 8, h // 8, _ctab(qt), C.c_void_p(out.data_ptr())))
    hip_ctx.synchronize()
    _same([out.cpu().numpy().reshape(-1, 64)], [want.reshape(-1, 64)], f"{case.name} {RL.route(case)}")
    F.assert_frame_intact(sfr, written=(), what=case.name)


@_params("fdct_quant_rgb")
def test_fdct_quant_rgb_takes_the_vector_layout_and_refuses_the_rest(hip_ctx, case):
    import torch

    w, h = case.w, case.h
    src = _random(case.a.fmt, w, h, 137)
    ql, qc = _qt(hip_ctx, 85, False), _qt(hip_ctx, 85, True)
    sfr = _frame(case.a, w, h, src)
    outs = [torch.full((h // 8, w // 8, 64), 0x5a5a, dtype=torch.int16, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    st = hip_ctx.lib.uhdr_hip_fdct_quant_rgb_dev(hip_ctx.handle, C.byref(sfr.raw), _ctab(ql), _ctab(qc), *[C.c_void_p(o.data_ptr()) for o in outs])
    hip_ctx.synchronize()
    if RL.route(case) == ("refused",):
        assert st.error_code == UNSUPPORTED, (case.name, st.error_code)
        assert all(bool((o == 0x5a5a).all()) for o in outs), "a refused call wrote coefficients"
    else:
        A.check(st)
        planes = L.jpeg_rgb_to_ycc_port(_rgb888_of(src, w, h), w, w, h)
        for c in range(3):
            want = L.fdct_quant_port(planes[c], w, w // 8, h // 8, ql if c == 0 else qc)
            _same([outs[c].cpu().numpy().reshape(-1, 64)], [want.reshape(-1, 64)], f"{case.name} component {c}")
    F.assert_frame_intact(sfr, written=(), what=case.name)


# ---- toneMap ----------------------------------------------------------------------------------------------------------------------------
def _tone_hdr(case):
    ct, cg = case.opt["ct"], case.opt["cg"]
    def make():
        if case.a.fmt == RL.P010:
            return synth.make_hdr_p010(256, 96, ct=ct, cg=cg, noise=0.04)
        if case.a.fmt == RL.R1010102:
            return synth.make_hdr_rgba1010102(256, 96, ct=ct, cg=cg, noise=0.04)
        if case.a.fmt == RL.F16:
            return synth.make_hdr_rgba_f16(256, 96, cg=cg, noise=0.04)
        return synth.make_hdr_yuv444_10bit(256, 96, ct=ct, cg=cg, noise=0.04)
    return _once(("tone-hdr", case.a.fmt, ct, cg), make)


def _bytes(planes):
    return [p.view(np.uint8) if p.dtype != np.uint8 else p for p in planes]


def _run_tone_map(hip_ctx, case):
    w, h = case.w, case.h
    hdr = _tone_hdr(case)
    sub = case.a.fmt == RL.P010
    ww, hw = (_even(w), _even(h)) if sub else (w, h)
    hfr, sfr = _frame(case.a, w, h, hdr), _frame(case.b, w, h)
    A.check(hip_ctx.lib.uhdr_hip_tone_map_dev(hip_ctx.handle, C.byref(hfr.raw), C.byref(sfr.raw)))
    hip_ctx.synchronize()
    F.assert_frame_intact(hfr, written=(), what=case.name + " hdr intent")
    F.assert_frame_intact(sfr, written=(ww, hw), what=case.name + " sdr intent")
    return _bytes(sfr.valid(ww, hw)), sfr.desc()


@_params("tone_map")
def test_tone_map(hip_ctx, case):
    w, h = case.w, case.h
    sub = case.a.fmt == RL.P010
    ww, hw = (_even(w), _even(h)) if sub else (w, h)
    hdr = _tone_hdr(case)
    want = _once(("tone-want", case.a.fmt, case.opt["ct"], case.opt["cg"], ww, hw),
                 lambda: _bytes(L.tone_map(TF.oracle_kind(), F.tight(case.a.fmt, ww, hw, hdr)).planes_valid()))
    got, desc = _run_tone_map(hip_ctx, case)
    routes = RL.route(case)
    for i, (g, wnt) in enumerate(zip(got, want)):
        d = np.abs(g.astype(np.int64) - wnt.astype(np.int64))
        print(f"{case.name} {routes}: plane {i}: max code diff {d.max()}, {(d != 0).sum()} of {d.size} samples differ from the oracle")
        TF.assert_close_codes(g, wnt, 1e-4, f"{case.name} plane {i}")
    base = _base_of(case)
    bgot, bdesc = _once(("tone-base", base.name), lambda: _run_tone_map(hip_ctx, base))
    assert desc[:4] == bdesc[:4] == (case.b.fmt, A.UHDR_CG_DISPLAY_P3, A.UHDR_CT_SRGB, FULL) and desc[4:] == (w, h)
    if sub and (w, h) == (base.w, base.h) and case.opt == base.opt:
        same = all(np.array_equal(a, b) for a, b in zip(got, bgot))
        print(f"{case.name}: {'equals' if same else 'differs from'} the aligned case bit for bit")
        if routes[1] == RL.route(base)[1]:  # the same loads: only the packing of the luma bytes differs
            _same(got, bgot, f"{case.name} against the aligned case")


# ---- generateGainMap --------------------------------------------------------------------------------------------------------------------
def _gen_intents(case):
    def sdr():
        return synth.make_sdr_planar(case.a.fmt, 256, 96, cg=A.UHDR_CG_BT_709, noise=0.04)

    def hdr():
        return TF._hdr("p010" if case.b.fmt == RL.P010 else "1010102", 256, 96)
    return _once(("gen-sdr", case.a.fmt), sdr), _once(("gen-hdr", case.b.fmt), hdr)


def _gen_cfg(case):
    o = case.opt
    return A.default_encode_cfg(preset=A.UHDR_USAGE_BEST_QUALITY if o["two_pass"] else A.UHDR_USAGE_REALTIME, use_multi_channel_gainmap=int(o["nch"] == 3),
                                map_dimension_scale_factor=o["scale"], gamma=o["gamma"])


def _run_generate(hip_ctx, case):
    import torch

    w, h, o = case.w, case.h, case.opt
    mw, mh = w // o["scale"], h // o["scale"]
    sdr, hdr = _gen_intents(case)
    cfg = _gen_cfg(case)
    sfr, hfr, gfr = _frame(case.a, w, h, sdr), _frame(case.b, w, h, hdr), _frame(case.c, mw, mh)
    md = A.GainmapMetadata()
    lib = hip_ctx.lib
    if "gain_off" in o:  # the two passes on their own: the ratio plane is the caller's, here off its 16-byte boundary
        store = torch.zeros(mw * mh * o["nch"] + 8, dtype=torch.float32, device=DEV)
        mm = torch.zeros(6, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        ratio = store.data_ptr() + (-store.data_ptr()) % 16 + o["gain_off"]
        ubc = C.c_int(-1)
        A.check(lib.uhdr_hip_generate_gainmap_pass1_dev(hip_ctx.handle, C.byref(sfr.raw), C.byref(hfr.raw), C.byref(cfg), C.c_void_p(ratio), C.c_void_p(mm.data_ptr()),
                                                        C.byref(ubc)))
        hip_ctx.synchronize()
        fin = (C.c_float * 6)(*mm.cpu().tolist())
        A.check(lib.uhdr_hip_generate_gainmap_finalize(C.byref(cfg), hdr.raw.ct, ubc.value, fin, C.byref(md)))
        gfr.raw.w, gfr.raw.h = mw, mh
        A.check(lib.uhdr_hip_generate_gainmap_pass2_dev(hip_ctx.handle, C.c_void_p(ratio), fin, C.byref(cfg), C.byref(gfr.raw)))
    else:
        A.check(lib.uhdr_hip_generate_gainmap_dev(hip_ctx.handle, C.byref(sfr.raw), C.byref(hfr.raw), C.byref(cfg), C.byref(md), C.byref(gfr.raw)))
    hip_ctx.synchronize()
    F.assert_frame_intact(sfr, written=(), what=case.name + " sdr intent")
    F.assert_frame_intact(hfr, written=(), what=case.name + " hdr intent")
    F.assert_frame_intact(gfr, what=case.name + " map")
    return gfr.valid()[0], md.as_dict(), gfr.desc()


@_params("generate")
def test_generate_gainmap(hip_ctx, case):
    w, h, o = case.w, case.h, case.opt
    sdr, hdr = _gen_intents(case)
    cfg = _gen_cfg(case)
    md_w, gm_w = _once(("gen-want", case.a.fmt, case.b.fmt, w, h, o["two_pass"], o["nch"], o["scale"], o["gamma"]),
                       lambda: L.generate_gainmap(TF.oracle_kind(), F.tight(case.a.fmt, w, h, sdr), F.tight(case.b.fmt, w, h, hdr), cfg))
    got, md, desc = _run_generate(hip_ctx, case)
    routes = RL.route(case)
    d = np.abs(got.astype(np.int64) - gm_w.valid(0).astype(np.int64))
    print(f"{case.name} {routes}: max code diff {d.max()}, {(d != 0).sum()} of {d.size} samples differ from the oracle")
    TF.assert_close_codes(got, gm_w.valid(0), 1e-4, case.name)
    for k, v in md_w.as_dict().items():
        assert np.allclose(md[k], v, rtol=1e-6, atol=0), (case.name, k, md[k], v)
    if "gain_off" not in o:  # (pass 2 on its own fills the map and leaves its description to the caller)
        assert desc == (gm_w.raw.fmt, gm_w.raw.cg, gm_w.raw.ct, gm_w.raw.range, gm_w.raw.w, gm_w.raw.h)
    # the routes of launch_affine_map differ only in how the bytes are packed: against the aligned case of the same samples
    anchor = next((c for c in RL.cases_of("generate") if c.name == case.name.rsplit("/", 1)[0]), None) if o.get("affine_pairs") else None
    if anchor is not None and (anchor.w, anchor.h) == (w, h):
        agot, amd, adesc = _once(("gen-anchor", anchor.name), lambda: _run_generate(hip_ctx, anchor))
        _same([got], [agot], f"{case.name} {routes} against {anchor.name} {RL.route(anchor)}")
        assert md == amd
        if "gain_off" not in o:
            assert desc == adesc
