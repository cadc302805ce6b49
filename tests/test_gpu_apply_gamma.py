"""GPU: uhdr_hip_apply_gainmap_ex / _ex_dev with UHDR_HIP_APPLY_GAMMA_TABLE -- a gain-map gamma other than 1 at a map scale other
than 1 through the host-built thresholds of GainLUT::getGainFactor's table index (gainmapmath.h:483-489) instead of a pow per
sample.  The thresholds come from the host libm the oracle calls, so the bar is ZERO differing samples wherever only that pow stood
between the device and the reference; the non-integer scale keeps the older allowance for its untouched sqrt site.  The profile
families say which kernel ran."""
import ctypes as C

import numpy as np
import pytest

from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image, stripe_view
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, P1010102 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat, A.UHDR_IMG_FMT_32bppRGBA1010102
Y420, Y422, Y444, RGBA = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_16bppYCbCr422, A.UHDR_IMG_FMT_24bppYCbCr444, A.UHDR_IMG_FMT_32bppRGBA8888
LINEAR, HLG, PQ = A.UHDR_CT_LINEAR, A.UHDR_CT_HLG, A.UHDR_CT_PQ
GT = A.UHDR_HIP_APPLY_GAMMA_TABLE
QUAD, GENERIC, PLAIN = "apply_gainmap_gamma_quad", "apply_gainmap_gamma_generic", "apply_gainmap"


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def out_fmt(ct):
    return F16 if ct == LINEAR else P1010102


def make_base(fmt, w, h):
    if fmt == Y420:
        return synth.make_sdr_yuv420(w, h, noise=0.05)
    if fmt == RGBA:
        return synth.make_sdr_rgba8888(w, h, noise=0.05)
    return synth.make_sdr_planar(fmt, w, h, noise=0.05)


def make_map(kind, w, h):
    return synth.make_gainmap(w, h, 1 if kind == "y400" else 3, kind == "rgba8888", cg=A.UHDR_CG_BT_2100)


def apply_ex(uhdr, sdr, gm, md, ct, flags, boost=A.FLT_MAX, device=True):
    if not device:
        dest = Image(out_fmt(ct), sdr.w, sdr.h, align=1)
        uhdr.applyGainMapEx(sdr, gm, md, ct, out_fmt(ct), boost, dest, flags)
        return dest
    dest = Image(out_fmt(ct), sdr.w, sdr.h, align=4, device=DEV)
    uhdr.applyGainMapEx(sdr.to(DEV), gm.to(DEV), md, ct, out_fmt(ct), boost, dest, flags)
    uhdr.ctx.synchronize()
    return dest.to_host()


def launches(ctx, family):
    return ctx.profile_read(family)[0]


class Profiled:
    """Profiling on for the block, every family's tally emptied at both ends (the context is the session's)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.synchronize()
        self.ctx.profile(True)
        self.ctx.profile_read(None)
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        self.ctx.profile_read(None)
        self.ctx.profile(False)


# ---- 1. the quad kernel against the oracle ----------------------------------------------------------------------------------------------
# 384 x 192: two column strips, whole.  258 x 130: a second strip of two pixels, shifted left to end at the image edge; 258 = 2 * 3 * 43,
# so only scale 2 leaves a whole-number map -- 264 x 136 (a ragged second strip again, eight pixels wide) carries scales 4 and 8 for that
# shape.  256 x 64: one strip wide, the three other base layouts.
BASES = [(Y420, 384, 192), (Y420, 258, 130), (Y420, 264, 136), (Y422, 256, 64), (Y444, 256, 64), (RGBA, 256, 64)]
BASE_IDS = ["420-384x192", "420-258x130", "420-264x136", "422-256x64", "444-256x64", "rgba-256x64"]


@pytest.mark.parametrize("out_ct", [LINEAR, HLG, PQ], ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_quad_cases_equal_the_oracle(uhdr, base, out_ct):
    fmt, w, h = base
    sdr = make_base(fmt, w, h)
    dsdr = sdr.to(DEV)
    ran = 0
    with Profiled(uhdr.ctx) as prof:
        for scale in (2, 4, 8):
            if w % scale or h % scale:
                continue
            for kind in ("y400", "rgb888", "rgba8888"):
                gm = make_map(kind, w // scale, h // scale)
                dgm = gm.to(DEV)
                for gamma in (1.571, 0.8):
                    for ubc in (0, 1):
                        md = synth.default_metadata(gamma=gamma, use_base_cg=ubc, per_channel=(kind != "y400"))
                        # a display boost below the content boost (weight < 1) on one gamut side, the full boost on the other
                        boost = 2.5 if ubc == 0 else A.FLT_MAX
                        want = L.apply_gainmap(oracle_kind(), sdr, gm, md, out_ct, boost)
                        dest = Image(out_fmt(out_ct), w, h, align=4, device=DEV)
                        uhdr.applyGainMapEx(dsdr, dgm, md, out_ct, out_fmt(out_ct), boost, dest, GT)
                        uhdr.ctx.synchronize()
                        got = dest.to_host()
                        diff = int((got.valid(0) != want.valid(0)).sum())
                        print(f"{w}x{h} fmt={fmt} {kind} scale={scale} gamma={gamma} ubc={ubc} ct={out_ct}: {diff} differing samples")
                        assert diff == 0
                        assert got.raw.cg == want.raw.cg
                        ran += 1
        uhdr.ctx.synchronize()
        assert launches(uhdr.ctx, QUAD) == ran and launches(uhdr.ctx, PLAIN) == 0 and launches(uhdr.ctx, GENERIC) == 0
    assert ran >= 12


def test_host_images_take_the_same_route(uhdr):
    sdr = make_base(Y420, 384, 192)
    gm = make_map("y400", 96, 48)
    md = synth.default_metadata(gamma=1.571)
    got = apply_ex(uhdr, sdr, gm, md, LINEAR, GT, device=False)
    assert np.array_equal(got.valid(0), L.apply_gainmap(oracle_kind(), sdr, gm, md, LINEAR).valid(0))


@pytest.mark.parametrize("out_ct", [LINEAR, PQ], ids=["linear", "pq"])
def test_a_stripe_through_ex_dev(uhdr, out_ct):
    """Rows 64-127 of 192: the stripe's pixels are the whole image's."""
    w, h = 384, 192
    sdr, gm = make_base(Y420, w, h), make_map("rgb888", w // 4, h // 4)
    md = synth.default_metadata(gamma=1.571, per_channel=True, use_base_cg=0)
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, out_ct).valid(0)
    dsdr, dgm = sdr.to(DEV), gm.to(DEV)
    dest = Image(out_fmt(out_ct), w, h, align=4, device=DEV)
    s, d = stripe_view(dsdr, 64, 64), stripe_view(dest, 64, 64)
    with Profiled(uhdr.ctx):
        A.check(uhdr.lib.uhdr_hip_apply_gainmap_ex_dev(uhdr.ctx.handle, C.byref(s), C.byref(dgm.raw), C.byref(md), out_ct, out_fmt(out_ct), A.FLT_MAX,
                                                       C.byref(d), 64, h, GT))
        uhdr.ctx.synchronize()
        assert launches(uhdr.ctx, QUAD) == 1
    got = dest.to_host().valid(0)
    assert np.array_equal(got[64:128], want[64:128])
    assert not got[:64].any() and not got[128:].any()


# ---- 2. the generic kernel ----------------------------------------------------------------------------------------------------------
def per_channel_gammas(md, gammas=(1.3, 1.7, 2.2)):
    for i, g in enumerate(gammas):
        md.gamma[i] = g
    return md


GENERIC_CASES = {
    # three gammas: three tables do not fit beside the quad kernel's tiles, so even geometry goes to the generic kernel too
    "per-channel gammas, scale 2": lambda: (make_base(Y420, 384, 192), make_map("rgb888", 192, 96), per_channel_gammas(synth.default_metadata(per_channel=True))),
    "scale 3": lambda: (make_base(Y420, 384, 192), make_map("y400", 128, 64), synth.default_metadata(gamma=1.571)),
    "scale 3, three channels": lambda: (make_base(Y444, 264, 48), make_map("rgba8888", 88, 16), synth.default_metadata(gamma=0.8, per_channel=True, use_base_cg=0)),
    "scale 16": lambda: (make_base(Y420, 384, 192), make_map("y400", 24, 12), synth.default_metadata(gamma=1.571)),
    "131 x 67": lambda: (synth.make_sdr_yuv420(131, 67, align=1), make_map("rgb888", 131, 67), per_channel_gammas(synth.default_metadata(per_channel=True))),
}


@pytest.mark.parametrize("out_ct", [LINEAR, HLG, PQ], ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("case", list(GENERIC_CASES), ids=[k.replace(" ", "_").replace(",", "") for k in GENERIC_CASES])
def test_generic_cases_equal_the_oracle(uhdr, case, out_ct):
    sdr, gm, md = GENERIC_CASES[case]()
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, out_ct)
    with Profiled(uhdr.ctx):
        got = apply_ex(uhdr, sdr, gm, md, out_ct, GT)
        assert launches(uhdr.ctx, GENERIC) == 1 and launches(uhdr.ctx, QUAD) == 0 and launches(uhdr.ctx, PLAIN) == 0
    diff = int((got.valid(0) != want.valid(0)).sum())
    print(f"{case} ct={out_ct}: {diff} differing samples")
    assert diff == 0


def test_a_non_integer_scale_keeps_its_allowance(uhdr):
    """240 x 120 under a 160 x 80 map: the sampler's double sqrt is the device's, as before -- one half-float code on at most 0.1 % of
    the samples.  The pow is gone from this route as well."""
    sdr, gm = synth.make_sdr_yuv420(240, 120), synth.make_gainmap(160, 80, 1)
    md = synth.default_metadata(gamma=1.571)
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, LINEAR)
    with Profiled(uhdr.ctx):
        got = apply_ex(uhdr, sdr, gm, md, LINEAR, GT)
        assert launches(uhdr.ctx, GENERIC) == 1
    a = got.valid(0).view(np.uint16).astype(np.int64)
    b = want.valid(0).view(np.uint16).astype(np.int64)
    d = np.abs(a - b)
    print(f"non-integer scale: max code diff {d.max()}, {(d != 0).mean():.4%} of samples differ")
    assert d.max() <= 1 and (d != 0).mean() <= 0.001


# ---- 3. routes and flags ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_ct", [LINEAR, PQ], ids=["linear", "pq"])
def test_without_the_flag_nothing_changes(uhdr, out_ct):
    """flags 0 is applyGainMap: the same bytes (the pow per sample), recorded under apply_gainmap."""
    sdr, gm = make_base(Y420, 384, 192), make_map("y400", 96, 48)
    md = synth.default_metadata(gamma=1.571)
    dsdr, dgm = sdr.to(DEV), gm.to(DEV)
    with Profiled(uhdr.ctx):
        old = Image(out_fmt(out_ct), sdr.w, sdr.h, align=4, device=DEV)
        uhdr.applyGainMap(dsdr, dgm, md, out_ct, out_fmt(out_ct), A.FLT_MAX, old)
        uhdr.ctx.synchronize()
        assert launches(uhdr.ctx, PLAIN) == 1 and launches(uhdr.ctx, QUAD) == 0 and launches(uhdr.ctx, GENERIC) == 0
        zero = apply_ex(uhdr, sdr, gm, md, out_ct, 0)
        assert launches(uhdr.ctx, PLAIN) == 1 and launches(uhdr.ctx, QUAD) == 0 and launches(uhdr.ctx, GENERIC) == 0
    assert np.array_equal(zero.valid(0), old.to_host().valid(0))


def test_gamma_one_and_scale_one_stay_on_the_old_kernels(uhdr):
    sdr = make_base(Y420, 384, 192)
    with Profiled(uhdr.ctx):
        for gm, md in ((make_map("y400", 96, 48), synth.default_metadata()), (make_map("rgb888", 384, 192), synth.default_metadata(gamma=2.2, per_channel=True))):
            got = apply_ex(uhdr, sdr, gm, md, LINEAR, GT)
            assert np.array_equal(got.valid(0), L.apply_gainmap(oracle_kind(), sdr, gm, md, LINEAR).valid(0))
        assert launches(uhdr.ctx, PLAIN) == 2 and launches(uhdr.ctx, QUAD) == 0 and launches(uhdr.ctx, GENERIC) == 0


def test_a_gamma_without_a_table_keeps_the_pow(uhdr):
    """NaN passes no table check; validate_metadata decides what the call answers, exactly as without the flag."""
    sdr, gm = make_base(Y420, 384, 192), make_map("y400", 96, 48)
    md = synth.default_metadata(gamma=float("nan"))
    outs = []
    for call in (lambda d: uhdr.applyGainMap(sdr, gm, md, LINEAR, F16, A.FLT_MAX, d), lambda d: uhdr.applyGainMapEx(sdr, gm, md, LINEAR, F16, A.FLT_MAX, d, GT)):
        dest = Image(F16, sdr.w, sdr.h, align=1)
        try:
            call(dest)
            outs.append((0, dest.valid(0).copy()))
        except A.UhdrError as e:
            outs.append((e.code, None))
    assert outs[0][0] == outs[1][0]
    if outs[0][1] is not None:
        assert np.array_equal(outs[0][1], outs[1][1])


def test_the_resized_map_flag_is_apply_gainmap_any(uhdr):
    """A 4:3 map under a 2:1 base: flag 1 gives applyGainMapAny's bytes, with and without the gamma flag beside it at gamma 1."""
    sdr, gm = make_base(Y420, 384, 192), make_map("y400", 96, 72)
    md = synth.default_metadata()
    want = Image(F16, sdr.w, sdr.h, align=1)
    uhdr.applyGainMapAny(sdr, gm, md, LINEAR, F16, A.FLT_MAX, want)
    for flags in (A.UHDR_HIP_APPLY_RESIZED_MAP, A.UHDR_HIP_APPLY_RESIZED_MAP | GT):
        assert np.array_equal(apply_ex(uhdr, sdr, gm, md, LINEAR, flags).valid(0), want.valid(0))
    with pytest.raises(A.UhdrError) as e:  # without flag 1 such a map is refused, as by applyGainMap
        apply_ex(uhdr, sdr, gm, md, LINEAR, GT)
    assert e.value.code == A.UHDR_CODEC_UNSUPPORTED_FEATURE


def test_a_resized_map_with_a_gamma_equals_the_reference(uhdr):
    """The reference resizes the map and samples it at scale 1 (jpegr.cpp:1651-1671): both flags together, the oracle's bytes."""
    import resize_port

    sdr, gm = make_base(Y420, 384, 192), make_map("y400", 96, 72)
    md = synth.default_metadata(gamma=1.571)
    resized = resize_port.resize_image(gm, sdr.w, sdr.h)
    want = L.apply_gainmap(oracle_kind(), sdr, resized, md, LINEAR)
    got = apply_ex(uhdr, sdr, gm, md, LINEAR, A.UHDR_HIP_APPLY_RESIZED_MAP | GT)
    assert np.array_equal(got.valid(0), want.valid(0))


@pytest.mark.parametrize("flags", [0x4, 0x80000000, 0x2 | 0x10])
def test_unknown_flag_bits_are_refused(uhdr, flags):
    sdr, gm = make_base(Y420, 384, 192), make_map("y400", 96, 48)
    md = synth.default_metadata(gamma=1.571)
    for device in (False, True):
        with pytest.raises(A.UhdrError) as e:
            apply_ex(uhdr, sdr, gm, md, LINEAR, flags, device=device)
        assert e.value.code == A.UHDR_CODEC_INVALID_PARAM


# ---- 4. the lookup itself, device wide -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.571, 0.25])
def test_device_sweep_of_the_lookup(hip_ctx, gamma):
    """uhdr_hip_selftest 5: every float from 0 to eight ulps past the last threshold, the estimate-and-settle lookup against the
    binary search over the same thresholds."""
    out = (C.c_ulonglong * 8)()
    mm = (C.c_float * 6)(gamma, 0, 0, 0, 0, 0)
    A.check(hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, 5, 0, 0, 0, mm, out))
    bad, swept, searched, no_table = out[0], out[1], out[2], out[3]
    print(f"gamma {gamma}: {swept} floats swept, {bad} mismatches, {searched} needed the search")
    assert no_table == 0 and swept > 0x3F000000 and bad == 0


def test_device_sweep_reports_a_gamma_without_a_table(hip_ctx):
    out = (C.c_ulonglong * 8)()
    mm = (C.c_float * 6)(-1.0, 0, 0, 0, 0, 0)
    A.check(hip_ctx.lib.uhdr_hip_selftest(hip_ctx.handle, 5, 0, 0, 0, mm, out))
    assert out[3] == 1 and out[1] == 0
