"""GPU: applyGainMap on the gain-map metadata other encoders write (tests/apply_metadata_cases.py) -- offsets of 1/64, offset_hdr above
offset_sdr, factors below 1, values per channel, hdr_capacity_min above 1, a gamma on some channels only -- against the oracle, on
every kernel form: the quad kernel at scale 1 (byte -> factor tables), at scales 2 and 4 (interpolating), with the gamma-table flag
(quad and generic forms), the generic kernel at odd, large and non-integer scales, the resized-map entry point, host images, a stripe,
and more table keys than the context has slots.  tests/test_apply_metadata_cases.py shows on the CPU that these inputs send 1 - 30 % of
the samples below zero before the clamp and reach both output ceilings; synth's default metadata does neither.

The bar is each route's bar at default metadata, no wider: zero differing samples wherever every transcendental comes from a host-built
table (the quad kernel in all its modes, the generic kernel at an integer scale with gamma 1 or with the gamma-table flag, the resized
map); one half-float code on at most 0.1 % of the samples where the device's own double sqrt (non-integer scale) or pow (gamma != 1
without the flag) stands in for the host's -- tests/test_gpu_parity.py:113, tests/test_gpu_apply_gamma.py:198.  The profile families say
which kernel ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import apply_metadata_cases as M
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image, stripe_view
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LINEAR, HLG, PQ = M.LINEAR, M.HLG, M.PQ
CTS = [LINEAR, HLG, PQ]
GT, RESIZED = A.UHDR_HIP_APPLY_GAMMA_TABLE, A.UHDR_HIP_APPLY_RESIZED_MAP
QUAD, GENERIC, PLAIN = "apply_gainmap_gamma_quad", "apply_gainmap_gamma_generic", "apply_gainmap"
BT709, BT2100 = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
PLAIN_NAMES = [n for n in M.NAMES if n not in M.GAMMA_NAMES]


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


@functools.lru_cache(maxsize=None)
def base_pair(fmt, w, h, align=64):
    """(host, device) base image; built once and left unchanged."""
    img = M.base(fmt, w, h, align=align)
    return img, img.to(DEV)


@functools.lru_cache(maxsize=None)
def map_pair(kind, w, h, cg=BT2100):
    gm = M.gain_map(kind, w, h, cg=cg)
    return gm, gm.to(DEV)


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

    def launches(self):
        self.ctx.synchronize()
        return {f: self.ctx.profile_read(f)[0] for f in (PLAIN, QUAD, GENERIC)}


def differing(uhdr, base, gmap, md, ct, boost, flags=None, what=""):
    """One device call against the oracle: the number of differing samples (R, G, B; printed), the two sample arrays."""
    (sdr, dsdr), (gm, dgm) = base, gmap
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, ct, boost)
    dest = Image(M.out_fmt(ct), sdr.w, sdr.h, align=4, device=DEV)
    if flags is None:
        uhdr.applyGainMap(dsdr, dgm, md, ct, M.out_fmt(ct), boost, dest)
    else:
        uhdr.applyGainMapEx(dsdr, dgm, md, ct, M.out_fmt(ct), boost, dest, flags)
    uhdr.ctx.synchronize()
    got = dest.to_host()
    assert got.raw.cg == want.raw.cg
    assert (got.valid(0) >> (48 if ct == LINEAR else 30) == (0x3C00 if ct == LINEAR else 3)).all()  # alpha: 1.0 / 3
    a, b = M.samples(got), M.samples(want)
    n = int((a != b).sum())
    print(f"{what} {sdr.w}x{sdr.h} fmt={sdr.fmt} map={gm.fmt} {gm.w}x{gm.h} ubc={md.use_base_cg} ct={ct} boost={boost:g}: {n} differing samples")
    return n, a, b


def assert_one_code(a, b, what):
    """tests/test_gpu_parity.py:113 -- identical codes on >= 99.9 % of the samples, never more than one apart."""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    print(f"{what}: max code diff {d.max()}, {(d != 0).mean():.4%} of samples differ")
    assert d.max() <= 1 and (d != 0).mean() <= 0.001, what


# ---- 1. scale 1: the byte -> factor tables (SMODE 0), a gamma folded in on the host --------------------------------------------------
# 384 x 192: two column strips; 256 x 64: the other base layouts
SCALE1_BASES = [(M.Y420, 384, 192, CTS), (M.Y422, 256, 64, [LINEAR, PQ]), (M.Y444, 256, 64, [LINEAR, PQ]), (M.RGBA, 256, 64, [LINEAR, PQ])]


@pytest.mark.parametrize("name", M.NAMES)
def test_scale_1_equals_the_oracle(uhdr, name):
    boosts = M.boosts(name)
    ran = 0
    with Profiled(uhdr.ctx) as prof:
        for fmt, w, h, cts in SCALE1_BASES:
            for kind in M.MAP_KINDS:
                for ct in cts:
                    md = M.metadata(name, use_base_cg=ran % 2)  # BT.2100 map over a BT.709 base: the matrix on the SDR side (0) / the HDR side (1)
                    n, _, _ = differing(uhdr, base_pair(fmt, w, h), map_pair(kind, w, h), md, ct, boosts[ran % 6], what=f"{name} scale 1 {kind}")
                    assert n == 0
                    ran += 1
        assert prof.launches() == {PLAIN: ran, QUAD: 0, GENERIC: 0}
    assert ran == 27


# ---- 2. scales 2 and 4: the interpolating quad kernel (SMODE 1) ----------------------------------------------------------------------
# 384 x 192: two column strips; 258 x 130 (scale 2) and 264 x 136 (scale 4): a ragged second strip, shifted left to end at the image edge
EVEN_SCALES = [(384, 192, 2), (384, 192, 4), (258, 130, 2), (264, 136, 4)]


@pytest.mark.parametrize("ct", CTS, ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_scales_2_and_4_equal_the_oracle(uhdr, name, ct):
    """use_base_cg 0 and 1 under a BT.2100 map: the gamut matrix before / after the gain, and the output-code table on the scaled value;
    a map in the base image's gamut: no matrix, and the table on the unscaled value (the prescaled form, its own clamp bounds)."""
    boosts = M.boosts(name)
    ran = 0
    with Profiled(uhdr.ctx) as prof:
        for w, h, scale in EVEN_SCALES:
            for kind in M.MAP_KINDS:
                for ubc, cg in ((0, BT2100), (1, BT2100), (1, BT709)):
                    if cg == BT709 and (w, scale) != (384, 2):
                        continue
                    md = M.metadata(name, use_base_cg=ubc)
                    n, _, _ = differing(uhdr, base_pair(M.Y420, w, h), map_pair(kind, w // scale, h // scale, cg), md, ct, boosts[ran % 2 * 2], what=f"{name} {kind}")
                    assert n == 0
                    ran += 1
        assert prof.launches() == {PLAIN: ran, QUAD: 0, GENERIC: 0}
    assert ran == 27


@pytest.mark.parametrize("kind,scale", [("y400", 4), ("rgb888", 2)])
@pytest.mark.parametrize("name", M.NAMES)
def test_the_display_boosts(uhdr, name, kind, scale):
    """The weight: none, both ends of the capacity exactly, between them (3.0, and 4.7, where a weight from double logarithms would differ
    from host::gainmap_weight's float ones), below the lower end (weight 0: the base image in linear light, minus the offsets'
    difference).  Cases with a gamma go with the gamma-table flag."""
    flags = GT if name in M.GAMMA_NAMES else None
    w, h = 384, 192
    outs = {}
    for boost, bid in zip(M.boosts(name), M.BOOST_IDS):
        for i, ct in enumerate(CTS):
            md = M.metadata(name, use_base_cg=i % 2)
            n, a, _ = differing(uhdr, base_pair(M.Y420, w, h), map_pair(kind, w // scale, h // scale), md, ct, boost, flags, what=f"{name} {kind} boost {bid}")
            assert n == 0
            outs[bid, ct] = a
    for ct in CTS:
        assert np.array_equal(outs["none", ct], outs["capacity-max", ct])  # both are weight 1
        lo, hi = M.CASES[name]["capacity"]
        assert np.array_equal(outs["capacity-min", ct], outs["1.2", ct]) == (lo >= 1.2)  # both are weight 0 then
        assert not np.array_equal(outs["3.0", ct], outs["none", ct]) and not np.array_equal(outs["3.0", ct], outs["capacity-min", ct])
        assert not np.array_equal(outs["4.7", ct], outs["3.0", ct])


# ---- 3. a gamma other than 1 at scales 2 and 4 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", CTS, ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("name", M.GAMMA_NAMES)
def test_gamma_table_flag_equals_the_oracle(uhdr, name, ct):
    """One gamma for the three channels: the quad kernel's SMODE 2.  Gamma 1 on one channel only: the generic kernel's table form, which
    must skip that channel's block (left at +inf) through gamma_is_one."""
    family = QUAD if name == "hdr-above-gamma" else GENERIC
    boosts = M.boosts(name)
    ran = 0
    with Profiled(uhdr.ctx) as prof:
        for w, h, scale in EVEN_SCALES:
            for kind in M.MAP_KINDS:
                for ubc in (0, 1):
                    md = M.metadata(name, use_base_cg=ubc)
                    n, _, _ = differing(uhdr, base_pair(M.Y420, w, h), map_pair(kind, w // scale, h // scale), md, ct, boosts[ran % 2 * 2], GT, what=f"{name} {kind} GT")
                    assert n == 0
                    ran += 1
        want = {PLAIN: 0, QUAD: 0, GENERIC: 0}
        want[family] = ran
        assert prof.launches() == want
    assert ran == 24


@pytest.mark.parametrize("name", M.GAMMA_NAMES)
def test_without_the_flag_the_pow_route_keeps_its_allowance(uhdr, name):
    """The generic kernel with a double pow per sample: the device's libm against the host's -- tests/test_gpu_parity.py:113 allows one
    half-float code on at most 0.1 % of the samples (linear output, the only transfer it checks)."""
    ran = 0
    with Profiled(uhdr.ctx) as prof:
        for (w, h, scale), kind in zip(EVEN_SCALES[:2] + [(384, 192, 3)], M.MAP_KINDS):
            for ubc in (0, 1):
                md = M.metadata(name, use_base_cg=ubc)
                for flags in (None, 0):
                    _, a, b = differing(uhdr, base_pair(M.Y420, w, h), map_pair(kind, w // scale, h // scale), md, LINEAR, A.FLT_MAX, flags, what=f"{name} {kind} pow")
                    assert_one_code(a, b, f"{name} {kind} scale {scale} ubc {ubc} without the flag")
                    ran += 1
        assert prof.launches() == {PLAIN: ran, QUAD: 0, GENERIC: 0}


# ---- 4. the generic kernel ----------------------------------------------------------------------------------------------------------
# scale 3 (odd), scale 16 (beyond the quad kernel's weight tables), 131 x 67 with unaligned rows at scale 1 (odd sizes)
GENERIC_SHAPES = [(M.Y420, 384, 192, 64, "y400", 3), (M.Y444, 264, 48, 64, "rgba8888", 3), (M.Y420, 384, 192, 64, "rgb888", 16), (M.Y420, 384, 192, 64, "y400", 16),
                  (M.Y420, 131, 67, 1, "rgb888", 1), (M.Y420, 131, 67, 1, "y400", 1)]


@pytest.mark.parametrize("ct", CTS, ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("name", M.NAMES)
def test_generic_kernel_equals_the_oracle(uhdr, name, ct):
    gamma = name in M.GAMMA_NAMES
    boosts = M.boosts(name)
    ran = tabled = 0
    with Profiled(uhdr.ctx) as prof:
        for i, (fmt, w, h, align, kind, scale) in enumerate(GENERIC_SHAPES):
            md = M.metadata(name, use_base_cg=i % 2)
            n, _, _ = differing(uhdr, base_pair(fmt, w, h, align), map_pair(kind, w // scale, h // scale), md, ct, boosts[i % 3], GT if gamma else None,
                                what=f"{name} {kind} scale {scale}")
            assert n == 0
            ran += 1
            tabled += gamma  # 131 x 67 too: the byte -> factor table with the gamma folded in is the quad kernel's, which takes no odd size
        assert prof.launches() == {PLAIN: ran - tabled, QUAD: 0, GENERIC: tabled}


@pytest.mark.parametrize("name", M.NAMES)
def test_a_non_integer_scale_keeps_its_allowance(uhdr, name):
    """240 x 120 under a 160 x 80 map: the sampler's double sqrt is the device's -- one half-float code on at most 0.1 % of the samples
    (tests/test_gpu_parity.py:113, tests/test_gpu_apply_gamma.py:198)."""
    flags = GT if name in M.GAMMA_NAMES else None
    with Profiled(uhdr.ctx) as prof:
        for kind, ubc in (("y400", 1), ("rgb888", 0)):
            _, a, b = differing(uhdr, base_pair(M.Y420, 240, 120), map_pair(kind, 160, 80), M.metadata(name, use_base_cg=ubc), LINEAR, A.FLT_MAX, flags,
                                what=f"{name} {kind} scale 1.5")
            assert_one_code(a, b, f"{name} {kind} non-integer scale")
        assert prof.launches() == ({PLAIN: 0, QUAD: 0, GENERIC: 2} if flags else {PLAIN: 2, QUAD: 0, GENERIC: 0})


# ---- 5. the resized map, host images, a stripe ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.NAMES)
def test_a_resized_map_equals_the_reference(uhdr, name):
    """A 4:3 map under a 2:1 base: the reference resizes the map and samples it at scale 1 (jpegr.cpp:1651-1671)."""
    import resize_port

    flags = RESIZED | (GT if name in M.GAMMA_NAMES else 0)
    sdr, dsdr = base_pair(M.Y420, 384, 192)
    for kind, ct, ubc in (("y400", LINEAR, 1), ("rgb888", PQ, 0), ("rgba8888", HLG, 1)):
        gm, dgm = map_pair(kind, 96, 72)
        md = M.metadata(name, use_base_cg=ubc)
        want = L.apply_gainmap(oracle_kind(), sdr, resize_port.resize_image(gm, sdr.w, sdr.h), md, ct)
        dest = Image(M.out_fmt(ct), sdr.w, sdr.h, align=4, device=DEV)
        uhdr.applyGainMapEx(dsdr, dgm, md, ct, M.out_fmt(ct), A.FLT_MAX, dest, flags)
        uhdr.ctx.synchronize()
        n = int((M.samples(dest.to_host()) != M.samples(want)).sum())
        print(f"{name} resized {kind} ct={ct}: {n} differing samples")
        assert n == 0
        if not flags & GT:
            other = Image(M.out_fmt(ct), sdr.w, sdr.h, align=4, device=DEV)
            uhdr.applyGainMapAny(dsdr, dgm, md, ct, M.out_fmt(ct), A.FLT_MAX, other)
            uhdr.ctx.synchronize()
            assert np.array_equal(other.to_host().valid(0), dest.to_host().valid(0))


@pytest.mark.parametrize("name", M.NAMES)
def test_host_images(uhdr, name):
    sdr, gm = base_pair(M.Y420, 384, 192)[0], map_pair("rgb888", 96, 48)[0]
    md = M.metadata(name, use_base_cg=0)
    for ct in (LINEAR, PQ):
        dest = Image(M.out_fmt(ct), sdr.w, sdr.h, align=1)
        if name in M.GAMMA_NAMES:
            uhdr.applyGainMapEx(sdr, gm, md, ct, M.out_fmt(ct), 3.0, dest, GT)
        else:
            uhdr.applyGainMap(sdr, gm, md, ct, M.out_fmt(ct), 3.0, dest)
        want = L.apply_gainmap(oracle_kind(), sdr, gm, md, ct, 3.0)
        n = int((dest.valid(0) != want.valid(0)).sum())
        print(f"{name} host images ct={ct}: {n} differing pixels")
        assert n == 0 and dest.raw.cg == want.raw.cg


@pytest.mark.parametrize("ct", [LINEAR, PQ], ids=["linear", "pq"])
def test_a_stripe_through_dev(uhdr, ct):
    """Rows 64-127 of 192, the bands at the stripe's top: the stripe's pixels are the whole image's, the rows around it stay untouched."""
    w, h = 384, 192
    sdr = M.base(M.Y420, w, h, band_row=64)
    gm, dgm = map_pair("rgb888", w // 4, h // 4)
    md = M.metadata("per-channel", use_base_cg=1)
    want = L.apply_gainmap(oracle_kind(), sdr, gm, md, ct, 3.0).valid(0)
    dsdr = sdr.to(DEV)
    dest = Image(M.out_fmt(ct), w, h, align=4, device=DEV, fill=0xA5)
    s, d = stripe_view(dsdr, 64, 64), stripe_view(dest, 64, 64)
    A.check(uhdr.lib.uhdr_hip_apply_gainmap_dev(uhdr.ctx.handle, C.byref(s), C.byref(dgm.raw), C.byref(md), ct, M.out_fmt(ct), 3.0, C.byref(d), 64, h))
    uhdr.ctx.synchronize()
    got = dest.to_host().valid(0)
    assert np.array_equal(got[64:128], want[64:128])
    untouched = np.frombuffer(bytes([0xA5]) * got.dtype.itemsize, dtype=got.dtype)[0]
    assert (got[:64] == untouched).all() and (got[128:] == untouched).all()


# ---- 6. more table keys than slots, with work in flight -------------------------------------------------------------------------------
def test_table_slots_with_work_in_flight():
    """The context keeps four table blocks, keyed by metadata, weight, scale and the gamma flag, and hands them out round robin.  Sixteen
    distinct keys, then the first three again, back to back on one stream with no synchronize in between: a block may only be overwritten
    behind the launches that read it, and a slot must regrow when a block with gamma thresholds follows a plain one of the same
    metadata.  Every destination against the oracle, at section 1 - 4's bar: zero differing samples (no call here takes the pow route)."""
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)
    try:
        u = UltraHdr(ctx=ctx)
        w, h = 384, 192
        base = base_pair(M.Y420, w, h)
        # (case, display boost, scale, flags): the seven cases; one at two more boosts (only the weight changes); one at two more scales;
        # the gamma cases without and with the flag, alternating, so that a plain block and a longer gamma block of one key prefix
        # follow each other through the slots
        keys = [(n, A.FLT_MAX, 4, GT if n in M.GAMMA_NAMES else None) for n in M.NAMES]
        keys += [("hdr-above", 3.0, 4, None), ("hdr-above", 1.2, 4, None), ("per-channel", A.FLT_MAX, 2, None), ("per-channel", A.FLT_MAX, 1, None)]
        keys += [("hdr-above-gamma", 3.0, 1, None), ("hdr-above-gamma", 3.0, 1, GT), ("mixed-gamma", 3.0, 1, None), ("mixed-gamma", 3.0, 1, GT),
                 ("hdr-above-gamma", 3.0, 2, GT)]
        keys += keys[:3] + [keys[15]]  # three that have left the slots long ago, and one that is still in its slot
        assert len(set(keys)) == 16 and len(keys) == 20
        calls = []
        for i, (name, boost, scale, flags) in enumerate(keys):
            ct = CTS[i % 3]
            gmap = map_pair("rgb888" if i % 2 else "y400", w // scale, h // scale)
            md = M.metadata(name, use_base_cg=i % 2)
            dest = Image(M.out_fmt(ct), w, h, align=4, device=DEV)
            if flags is None:
                u.applyGainMap(base[1], gmap[1], md, ct, M.out_fmt(ct), boost, dest)
            else:
                u.applyGainMapEx(base[1], gmap[1], md, ct, M.out_fmt(ct), boost, dest, flags)
            calls.append((name, boost, scale, flags, ct, gmap[0], md, dest))
        ctx.synchronize()
        for name, boost, scale, flags, ct, gm, md, dest in calls:
            want = L.apply_gainmap(oracle_kind(), base[0], gm, md, ct, boost)
            n = int((M.samples(dest.to_host()) != M.samples(want)).sum())
            print(f"{name} boost={boost:g} scale={scale} flags={flags} ct={ct}: {n} differing samples")
            assert n == 0
    finally:
        ctx.close()
