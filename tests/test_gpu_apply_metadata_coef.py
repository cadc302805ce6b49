"""GPU: the metadata other encoders write (tests/apply_metadata_cases.py) on the applyGainMap kernels that read the base image as JPEG
coefficients -- 4:2:0, 4:2:2 and 4:4:4, the three older entry points and uhdr_hip_apply_gainmap_coef_ex_dev with the gamma-table flag --
and through the one-call decode, which takes the metadata as an argument.  Inputs and bar are those of tests/test_gpu_coef422.py,
tests/test_gpu_coef444.py and tests/test_gpu_coef_gamma.py: coefficients of tests/coef_cases.py, bit for bit against the oracle's IDCT
followed by the oracle's applyGainMap, and against the library's staged route where the image is too large for the oracle (the shape of
tests/test_gpu_coef_tile_trips.py, on which a wave comes round to a second tile)."""
import functools

import numpy as np
import pytest

import apply_metadata_cases as M
from coef_cases import S420, S422, S444, grids, quality_tables, smooth_coefs
from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image
from oracle import loader as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LINEAR, HLG, PQ = M.LINEAR, M.HLG, M.PQ
GT = A.UHDR_HIP_APPLY_GAMMA_TABLE
BT709, BT2100 = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
SAMPLINGS = {"420": (S420, M.Y420), "422": (S422, M.Y422), "444": (S444, M.Y444)}
NAMES = ["hdr-above", "per-channel", "hdr-above-gamma"]
QUAD, PLAIN = "apply_gainmap_gamma_quad", "apply_gainmap"


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def oracle_kind():
    return "ref" if L.ref() is not None else "port"


def to_dev(coefs):
    import torch

    return [torch.from_numpy(c).to(DEV) for c in coefs]


@functools.lru_cache(maxsize=None)
def coef_case(sampling, w, h, quality):
    """(coefficients on libjpeg's grids, three different tables, the oracle's decode of them as an Image of that sampling); built once
    per geometry and left unchanged."""
    factors, fmt = SAMPLINGS[sampling]
    rng = np.random.default_rng(1000 * w + h + int(sampling))
    qts = quality_tables(quality)
    coefs = smooth_coefs(grids(w, h, factors), qts, rng)
    dec = Image(fmt, w, h, BT709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=2)
    for c in range(3):
        full = L.idct_dequant_port(coefs[c], qts[c])
        dec.valid(c)[:] = full[: dec.valid(c).shape[0], : dec.valid(c).shape[1]]
    return coefs, qts, dec


def run_operator(uhdr, sampling, dco, qts, w, h, dgm, md, ct, boost, flags):
    """flags None: the entry point of that sampling as it was before the flags; otherwise the _ex one."""
    dest = Image(M.out_fmt(ct), w, h, align=4, device=DEV)
    if flags is not None:
        uhdr.applyGainMapFromCoefficientsEx(dco, qts, w, h, BT709, dgm, md, ct, M.out_fmt(ct), boost, dest, sampling, flags)
    elif sampling == "444":
        uhdr.applyGainMapFromCoefficients444(dco, qts, w, h, BT709, dgm, md, ct, M.out_fmt(ct), boost, dest)
    else:
        uhdr.applyGainMapFromCoefficients(dco, qts, w, h, BT709, dgm, md, ct, M.out_fmt(ct), boost, dest, sampling=sampling)
    uhdr.ctx.synchronize()
    return dest


# ---- 1. the operators against the oracle --------------------------------------------------------------------------------------------
# 128 x 16: exactly one tile (two tile rows at 4:4:4).  130 x 18: a second tile column with two live pixels and a second tile row with two
# live rows (scales 1 and 2 only).  392 x 200: a partial last tile in both directions.
SIZES = [(128, 16, 95), (130, 18, 85), (392, 200, 70)]


@pytest.mark.parametrize("ct", [LINEAR, HLG, PQ], ids=["linear", "hlg", "pq"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sampling", list(SAMPLINGS))
def test_coefficient_operators_equal_the_oracle(uhdr, sampling, name, ct):
    gamma = name in M.GAMMA_NAMES
    maps = [("y400", 2), ("rgb888", 4), ("rgba8888", 2)] if gamma else [("y400", 1), ("rgb888", 1), ("rgba8888", 2), ("y400", 4)]
    boosts = M.boosts(name)
    ctx = uhdr.ctx
    ran = 0
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_read(None)
    try:
        for w, h, quality in SIZES:
            coefs, qts, dec = coef_case(sampling, w, h, quality)
            dco = to_dev(coefs)
            for kind, scale in maps:
                if w % scale or h % scale:
                    continue
                gm = M.gain_map(kind, w // scale, h // scale)
                md = M.metadata(name, use_base_cg=ran % 2)
                boost = boosts[(0, 2, 4, 5)[ran % 4]]
                want = L.apply_gainmap(oracle_kind(), dec, gm, md, ct, boost)
                got = run_operator(uhdr, sampling, dco, qts, w, h, gm.to(DEV), md, ct, boost, GT if gamma else None).to_host()
                n = int((M.samples(got) != M.samples(want)).sum())
                print(f"{sampling} {name} {w}x{h} {kind} scale={scale} ubc={md.use_base_cg} ct={ct} boost={boost:g}: {n} differing samples")
                assert n == 0 and np.array_equal(got.valid(0), want.valid(0)) and got.raw.cg == want.raw.cg
                ran += 1
        ctx.synchronize()
        tally = {f: ctx.profile_read(f)[0] for f in (PLAIN, QUAD, "idct_dequant")}
        assert tally == {PLAIN: 0 if gamma else ran, QUAD: ran if gamma else 0, "idct_dequant": 0}
    finally:
        ctx.profile_read(None)
        ctx.profile(False)
    assert ran == (8 if gamma else 11)


# ---- 2. a second tile per wave -------------------------------------------------------------------------------------------------------
def staged_whole_grid(uhdr, T, dcoefs, qts, h, sampling, dgm, md, boost, flags):
    """test_gpu_coef_tile_trips.staged with a display boost and flags: idct_dequant x 3 into a device image whose planes hold the whole
    block grid, then applyGainMapEx on its W x h pixels."""
    factors, fmt, _ = T.SAMPLINGS[sampling]
    dims = grids(T.W, h, factors)
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    wp = max(bw * 8 * hmax // f[0] for (bw, _), f in zip(dims, factors))
    hp = max(bh * 8 * vmax // f[1] for (_, bh), f in zip(dims, factors))
    img = Image(fmt, wp, hp, BT709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=16, device=DEV)
    for c in range(3):
        pl = img.plane_tensor(c)
        assert pl.shape[0] >= dims[c][1] * 8 and pl.shape[1] >= dims[c][0] * 8
        uhdr.idct_dequant(dcoefs[c], qts[c], plane=pl, stride=pl.shape[1])
    img.raw.w, img.raw.h = T.W, h
    img.w, img.h = T.W, h
    dest = Image(A.UHDR_IMG_FMT_64bppRGBAHalfFloat, T.W, h, align=4, device=DEV)
    uhdr.applyGainMapEx(img, dgm, md, LINEAR, dest.fmt, boost, dest, flags)
    uhdr.ctx.synchronize()
    return dest


@pytest.mark.parametrize("sampling,name,kind,scale", [("420", "hdr-above", "y400", 2), ("422", "per-channel", "rgb888", 1), ("444", "hdr-above-gamma", "y400", 2)])
def test_waves_take_a_second_tile(uhdr, sampling, name, kind, scale):
    import torch

    import test_gpu_coef_tile_trips as T

    dcoefs, qts, h = T.coef_case(sampling)  # that module's coefficients, built once per session
    rows = T.SAMPLINGS[sampling][2]
    assert -(-T.W // 128) * -(-h // rows) > T.walker_bound(), "no wave can reach a second tile"
    flags = GT if name in M.GAMMA_NAMES else 0
    dgm = M.gain_map(kind, T.W // scale, h // scale).to(DEV)
    md = M.metadata(name, use_base_cg=0)
    dest = run_operator(uhdr, sampling, dcoefs, qts, T.W, h, dgm, md, LINEAR, 3.0, flags if flags else None)
    want = staged_whole_grid(uhdr, T, dcoefs, qts, h, sampling, dgm, md, 3.0, flags)
    assert int(torch.count_nonzero(want.buf)) > want.buf.numel() // 8  # the staged route wrote an image
    n = int(torch.count_nonzero(dest.buf != want.buf))
    print(f"{sampling} {name} {T.W}x{h} {kind} scale={scale}: {n} differing bytes")
    assert n == 0


# ---- 3. the one-call decode ----------------------------------------------------------------------------------------------------------
def map_scan(uhdr, mw, mh, nch, seed):
    """tests/test_gpu_coef422.py's: a gain map as an entropy-coded scan, one component or three at 4:4:4."""
    rng = np.random.default_rng(seed)
    ql, qc = L.quant_table_port(92, False), L.quant_table_port(92, True)
    sampling = S444 if nch == 3 else [(1, 1)]
    dco = to_dev(smooth_coefs(grids(mw, mh, sampling), [ql, qc, qc][:nch], rng))
    return uhdr.jpeg_header(mw, mh, sampling, [ql, qc, qc][:nch]), uhdr.huffman_encode(dco, mw, mh, sampling, 0), dco, (ql, qc)


def decoded_map(uhdr, dco, tables, mw, mh, cg):
    if len(dco) == 3:
        img = uhdr.idct_dequant_rgb(dco, tables[0], tables[1], mw, mh, A.UHDR_IMG_FMT_32bppRGBA8888, 0)
        uhdr.ctx.synchronize()
        img.raw.cg = cg
        return img.to_host()
    plane = uhdr.idct_dequant(dco[0], tables[0])
    uhdr.ctx.synchronize()
    gm = Image(A.UHDR_IMG_FMT_8bppYCbCr400, mw, mh, cg)
    gm.valid(0)[:] = plane.cpu().numpy()[:mh, :mw]
    return gm


@pytest.mark.parametrize("sampling,name,nch,scale", [("420", "hdr-above", 1, 4), ("422", "per-channel", 3, 1), ("444", "per-channel", 1, 2),
                                                     ("444", "hdr-above-gamma", 1, 4), ("420", "hdr-above-gamma", 3, 2)])
def test_one_call_decode(uhdr, sampling, name, nch, scale):
    """uhdr_hip_decode_api1_scans_dev (4:2:0, 4:2:2), _any_dev (4:4:4) and _ex_dev (the gamma-table flag): the metadata goes straight to
    the coefficient kernel.  Against the staged operators -- entropy decode, the map's IDCT, the coefficient operator -- and the oracle."""
    w, h = 384, 176
    factors = SAMPLINGS[sampling][0]
    coefs, qts, dec = coef_case(sampling, w, h, 88)
    dco = to_dev(coefs)
    scan_b = uhdr.huffman_encode(dco, w, h, factors, 0)
    hb = uhdr.jpeg_header(w, h, factors, qts)
    mw, mh = w // scale, h // scale
    hm, scan_m, dmap, tables = map_scan(uhdr, mw, mh, nch, seed=w + nch + scale)
    gamma = name in M.GAMMA_NAMES
    ctx = uhdr.ctx
    for i, (ct, boost) in enumerate(((LINEAR, A.FLT_MAX), (PQ, 3.0), (HLG, 1.2))):
        md = M.metadata(name, use_base_cg=i % 2)
        dest = Image(M.out_fmt(ct), w, h, align=64, device=DEV)
        ctx.synchronize()
        ctx.profile(True)
        ctx.profile_read(None)
        try:
            if gamma:
                uhdr.decodeApi1ScansEx(hb, scan_b, BT709, hm, scan_m, BT2100, md, ct, M.out_fmt(ct), boost, dest, GT)
            elif sampling == "444":
                uhdr.decodeApi1ScansAny(hb, scan_b, BT709, hm, scan_m, BT2100, md, ct, M.out_fmt(ct), boost, dest)
            else:
                uhdr.decodeApi1Scans(hb, scan_b, BT709, hm, scan_m, BT2100, md, ct, M.out_fmt(ct), boost, dest)
            ctx.synchronize()
            # the map's IDCT only: the base image never exists as planes
            assert (ctx.profile_read("idct_dequant")[0], ctx.profile_read(QUAD)[0], ctx.profile_read(PLAIN)[0]) == (1, int(gamma), int(not gamma))
        finally:
            ctx.profile_read(None)
            ctx.profile(False)
        got = dest.to_host()
        back = uhdr.huffman_decode(scan_b, [(bh, bw) for bw, bh in grids(w, h, factors)], w, h, factors, 0)
        assert all(np.array_equal(b.cpu().numpy(), c) for b, c in zip(back, coefs))
        gm = decoded_map(uhdr, dmap, tables, mw, mh, BT2100)
        via_op = run_operator(uhdr, sampling, back, qts, w, h, gm.to(DEV), md, ct, boost, GT if gamma else None).to_host()
        want = L.apply_gainmap(oracle_kind(), dec, gm, md, ct, boost)
        n = int((M.samples(got) != M.samples(want)).sum())
        print(f"{sampling} {name} one call, map {nch} ch scale {scale} ct={ct} boost={boost:g}: {n} differing samples")
        assert np.array_equal(got.valid(0), via_op.valid(0))
        assert n == 0 and np.array_equal(got.valid(0), want.valid(0))
