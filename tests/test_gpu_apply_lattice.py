"""GPU: every case of tests/apply_lattice.py through uhdr_hip_apply_gainmap_dev / _ex_dev / _any_dev / _batch_dev, on views inside 0xA5
frames (tests/framed.py): base image, map and destination at the caller's own strides and base offsets, so that launch_apply_gainmap
is pushed onto each of its routes by one conjunct of apply_quad_mode at a time, and the quad kernel's own geometry -- ragged strips,
row groups, map clamps, stripes, the frame table -- is driven at the smallest sizes at which it can go wrong.

Base and map samples are independent random bytes over the whole code range, seeded per case, so a sample taken from a neighbour's
place shows (tests/test_apply_lattice.py shows on the CPU that a map row or a stripe offset off by one does).  The destination's valid
samples equal the oracle's on tight copies bit for bit, its gamut equals the oracle's, only its w x h samples (the stripe's rows of
them) have changed and no input frame has changed at all.  No kernel and no predicate is altered for a test."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import apply_lattice as AL
import framed as F
import resize_port
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILY = {0: "apply_gainmap", 1: "apply_gainmap_gamma_quad", 2: "apply_gainmap_gamma_generic"}


@pytest.fixture(scope="module")
def ctx():
    """One context for the file."""
    from libultrahdr_amd.ultrahdr import Context

    c = Context(0)
    yield c
    c.close()


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def _params(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


def random_image(fmt, w, h, seed, cg=A.UHDR_CG_BT_709):
    img = Image(fmt, w + w % 2, h + h % 2, cg, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    img.buf[:] = np.random.default_rng(seed).integers(0, 256, img.buf.size, dtype=np.uint8)
    return img


def metadata(case):
    md = synth.default_metadata(use_base_cg=case.opt.get("ubc", 1), per_channel=case.gm.fmt != AL.Y400)
    for i in range(3):
        md.gamma[i] = case.gamma[i]
    return md


def rows_of(img, fmt, w, row0, n):
    """A tight host image of rows [row0, row0 + n) of a single-plane image."""
    out = Image(fmt, w, n, img.raw.cg, img.raw.ct, img.raw.range, align=2)
    k = 3 if fmt == AL.RGB else 1
    out.plane(0)[:n, : w * k] = img.plane(0)[row0: row0 + n, : w * k]
    return out


def inputs(case, frame=0):
    """(base image of the frame's rows, map): random bytes, seeded by the case's name and the frame's number."""
    rows = case.full_h if case.opt.get("stripe") else case.h
    seed = zlib.crc32(case.name.encode()) + 7919 * frame
    return (random_image(case.base.fmt, case.w, rows, seed),
            random_image(case.gm.fmt, case.gm_w, case.gm_h, seed + 1, case.opt.get("map_cg", A.UHDR_CG_UNSPECIFIED)))


def expected(case, base, gm):
    """The oracle on tight copies -> (the rows the call writes, the destination's gamut)."""
    rows = case.full_h if case.opt.get("stripe") else case.h
    p = AL.params(case)
    tb, tg = F.tight(case.base.fmt, case.w, rows, base), F.tight(case.gm.fmt, case.gm_w, case.gm_h, gm)
    if p.resize_on:  # the reference resizes the map to the base image's size and samples it at scale 1 (jpegr.cpp:1651-1671)
        tg = resize_port.resize_image(tg, case.w, case.full_h or case.h, align=2)
    elif case.y0 and not case.opt.get("stripe"):  # rows [y0, y0 + h) of a taller image: at scale 1 those are the map's rows from y0 on
        assert p.scale == 1
        tg = rows_of(tg, case.gm.fmt, case.gm_w, case.y0, case.h)
    want = L.apply_gainmap(oracle_kind(), tb, tg, metadata(case), case.out_ct)
    v = want.valid(0)
    return (v[case.y0: case.y0 + case.h] if case.opt.get("stripe") else v), want.raw.cg


class _Fused:
    """UHDR_HIP_APPLY_RESIZE=fused for the duration of a call: the resizing sampler inside the kernel."""

    def __enter__(self):
        self.old = os.environ.get("UHDR_HIP_APPLY_RESIZE")
        os.environ["UHDR_HIP_APPLY_RESIZE"] = "fused"

    def __exit__(self, *exc):
        os.environ.pop("UHDR_HIP_APPLY_RESIZE", None)
        if self.old is not None:
            os.environ["UHDR_HIP_APPLY_RESIZE"] = self.old


def frames_of(case, base, gm, frame=0):
    rows = case.full_h if case.opt.get("stripe") else case.h
    gl = case.gm
    if frame == 1 and "second_gm_stride" in case.opt:
        gl = gl._replace(strides=(case.opt["second_gm_stride"],))
    sfr = F.framed(case.base.fmt, case.w, rows, case.base.strides, case.base.offsets, src=base, device=DEV)
    gfr = F.framed(gl.fmt, case.gm_w, case.gm_h, gl.strides, gl.offsets, src=gm, device=DEV)
    dfr = F.framed(case.dst.fmt, case.w, rows, (max(case.dst.strides[0], case.w),), case.dst.offsets, device=DEV)
    dfr.raw.stride[0] = case.dst.strides[0]  # (below the width only in a call that is refused for it)
    return sfr, gfr, dfr


def call(ctx, case, sdr, gm, dst, n=1):
    """sdr, gm, dst: uhdr_raw_image_t (arrays of n for the batch entry point) -> the status."""
    md, ct, fmt, lib = metadata(case), case.out_ct, AL.out_fmt(case.out_ct), ctx.lib
    if case.entry == "batch_dev":
        return lib.uhdr_hip_apply_gainmap_batch_dev(ctx.handle, n, sdr, gm, C.byref(md), ct, fmt, A.FLT_MAX, dst)
    args = (ctx.handle, C.byref(sdr), C.byref(gm), C.byref(md), ct, fmt, A.FLT_MAX, C.byref(dst), case.y0, case.full_h)
    if case.entry == "dev":
        return lib.uhdr_hip_apply_gainmap_dev(*args)
    if case.entry == "ex_dev":
        return lib.uhdr_hip_apply_gainmap_ex_dev(*args, case.flags)
    assert case.entry == "any_dev" and case.flags == AL.RESIZED_MAP
    with _Fused():
        return lib.uhdr_hip_apply_gainmap_any_dev(*args)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = got != want
    print(f"{what}: {int(bad.sum())} of {bad.size} output pixels differ from the oracle")
    if bad.any():
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"{what}: {ys.size} output pixels differ; the first at row {ys[0]}, column {xs[0]}: 0x{int(got[ys[0], xs[0]]):x} for "
                             f"0x{int(want[ys[0], xs[0]]):x}; rows {sorted(set(ys.tolist()))[:8]}, columns {sorted(set(xs.tolist()))[:8]}")


def run(ctx, case):
    """One case: the call on framed views, against the oracle, every frame checked."""
    n = case.opt.get("n", 1)
    route = AL.route(case)
    frames, wants = [], []
    for f in range(n):
        base, gm = inputs(case, f)
        frames.append(frames_of(case, base, gm, f))
        wants.append(expected(case, base, gm))
    stripe = case.opt.get("stripe")
    views = [(F.stripe(s, case.y0, case.h) if stripe else s.raw, g.raw, F.stripe(d, case.y0, case.h) if stripe else d.raw) for s, g, d in frames]
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_read(None)
    try:
        if case.entry == "batch_dev":
            arrs = [(A.RawImage * n)(*[v[k] for v in views]) for k in range(3)]
            A.check(call(ctx, case, *arrs, n=n))
            cgs = [arrs[2][i].cg for i in range(n)]
        else:
            A.check(call(ctx, case, *views[0]))
            cgs = [views[0][2].cg]
        ctx.synchronize()
        launches = {fam: ctx.profile_read(fam)[0] for fam in FAMILY.values()}
    finally:
        ctx.profile_read(None)
        ctx.profile(False)
    # the profile family says which of the gamma forms ran; a batch on the frame table is one launch, a batch frame by frame is n
    fam = FAMILY[AL.gamma_route(case)]
    assert launches == {f: ((1 if route[-1] == "frame table" else n) if f == fam else 0) for f in FAMILY.values()}, (case.name, route, launches)
    for i, ((sfr, gfr, dfr), (want, want_cg)) in enumerate(zip(frames, wants)):
        what = f"{case.name} {route}" + (f" frame {i}" if n > 1 else "")
        got = dfr.valid()[0]
        same(got[case.y0: case.y0 + case.h] if stripe else got, want, what)
        assert cgs[i] == want_cg, (what, cgs[i], want_cg)
        F.assert_frame_intact(dfr, what=what + " destination", rows=(case.y0, case.h) if stripe else None)
        F.assert_frame_intact(sfr, written=(), what=what + " base image")
        F.assert_frame_intact(gfr, written=(), what=what + " map")


def test_the_routes_of_the_tables(ctx):
    print("oracle:", oracle_kind())
    print(AL.describe(AL.CASES))
    print(AL.describe(AL.GEOMETRY))
    for conjunct, why, name, line in AL.UNREACHABLE:
        print(f"unreachable: {conjunct}: {why} ({name}: `{line}`)")


@_params(AL.CASES)
def test_every_conjunct_true_and_false(ctx, case):
    run(ctx, case)


@_params(AL.GEOMETRY)
def test_geometry(ctx, case):
    run(ctx, case)


def test_row_groups(ctx):
    """launch_quad hands a wave several quad rows only when the image has more quad rows than the device has resident waves per strip:
    a single 130-wide frame of just over 2 x CUs x 8 x (waves of a workgroup) rows -- 16386 rows for the 256-thread F16 variant and
    49154 for the 768-thread PQ one on 256 compute units, 2.1 and 6.4 megapixels; a batch of sixteen frames of a sixteenth of the height
    comes to the same number of waves and a few rows more, so the single frame is taken.  At those heights groups < qh and groups
    does not divide qh whatever the occupancy query answers from 1 to 8: some waves' look-ahead row is the clamped last one."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for case in AL.row_group_cases(cus):
        blk = AL.quad_block(AL.out_index(case.out_ct))
        assert AL.row_group_condition(cus, blk, case.w, case.h, case.opt["n"])
        print(f"{case.name}: groups at 1 .. 8 workgroups per CU:", [AL.row_groups(cus, k, blk, 1, case.h // 2, case.opt["n"])[:2] for k in range(1, 9)])
        run(ctx, case)


@_params(AL.REFUSALS)
def test_refusals(ctx, case):
    base, gm = inputs(case)
    sfr, gfr, dfr = frames_of(case, base, gm)
    st = call(ctx, case, sfr.raw, gfr.raw, dfr.raw)
    ctx.synchronize()
    assert ("refused", st.error_code) == AL.route(case), (case.name, st.error_code, AL.route(case))
    for fr in (sfr, gfr, dfr):
        F.assert_frame_intact(fr, written=(), what=case.name)


# An anchor again after a case of another route on the same context: the tables the previous call staged or cached (the byte -> factor
# table against the GainLUT, another scale's weights, another gamma's thresholds, the other transfer's code buckets) do not leak
SECOND_TRIPS = [("420/y400/s1/linear", "420/rgb888/s2/linear/gamma+flag"), ("420/rgb888/s2/linear/gamma+flag", "420/rgb888/s2/linear/gamma+flag/three-gammas"),
                ("420/y400/s4/hlg", "420/y400/s3/hlg"), ("444/rgb888/s8/pq", "420/rgb888/s1/pq/gamma+flag"),
                ("rgba/rgba8888/s2/pq/gamma+flag", "444/rgba8888/s1/pq"), ("422/rgb888/s1/hlg", "420/rgb888/s4/hlg/gamma+flag")]


@pytest.mark.parametrize("anchor,other", SECOND_TRIPS, ids=[f"{a} after {b}" for a, b in SECOND_TRIPS])
def test_an_anchor_again_after_another_route(ctx, anchor, other):
    by_name = {c.name: c for c in AL.CASES}
    assert AL.route(by_name[anchor]) != AL.route(by_name[other])
    run(ctx, by_name[other])
    run(ctx, by_name[anchor])
