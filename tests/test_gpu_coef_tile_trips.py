"""GPU: the coefficient-input applyGainMap kernel when a wave comes round to a second tile (for (t = wave; t < ntiles; t += nwaves)):
it then overwrites the LDS tile it has just read.  The other modules never get there: 4K is about 4000 tiles against about 7000
resident waves.

Linear F16 output runs 256-thread workgroups of four waves, and the launcher never asks for more than 8 workgroups per CU, so
32 x CUs bounds the walking waves from above; the shape has more tiles than that (asserted, not assumed).  w = 456: three full tile
columns and a ragged one; h is even and no multiple of the tile height, so the last tile row is ragged too.  The reference is the
library's staged route on the same device -- idct_dequant x 3 into planes, then applyGainMap -- and the whole destination is
compared bit for bit."""
import functools

import numpy as np
import pytest

import coef_cases as K
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth
from libultrahdr_amd.images import Image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat
W = 456
# sampling -> (factors, image format, pixel rows of a tile)
SAMPLINGS = {"420": (K.S420, A.UHDR_IMG_FMT_12bppYCbCr420, 16), "422": (K.S422, A.UHDR_IMG_FMT_16bppYCbCr422, 16),
             "444": (K.S444, A.UHDR_IMG_FMT_24bppYCbCr444, 8)}


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


def walker_bound():
    import torch

    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def height_for(sampling):
    """8 x CUs full tile rows and a ragged one of four tile columns each: 32 x CUs + 4 tiles."""
    rows = SAMPLINGS[sampling][2]
    return rows * (walker_bound() // 4) + rows - 6


@functools.lru_cache(maxsize=None)
def coef_case(sampling):
    """(device coefficients, tables, h): a smooth field through the oracle's FDCT; the last sixteenth of every component's block
    rows -- tiles of the second trip -- holds the full int16 range instead (the 32-bit multiply path).  Built once per sampling and
    left unchanged."""
    import torch

    h = height_for(sampling)
    rng = np.random.default_rng(1000 * W + h)
    dims = K.grids(W, h, SAMPLINGS[sampling][0])
    qts = K.quality_tables(88)
    coefs = K.smooth_coefs(dims, qts, rng)
    for c, wild in zip(coefs, K.wild_coefs(dims, rng)):
        n = c.shape[0] // 16
        c[-n:] = wild[-n:]
    return [torch.from_numpy(c).to(DEV) for c in coefs], qts, h


def staged(uhdr, dcoefs, qts, h, sampling, gm_dev, md):
    """idct_dequant x 3 into a device image whose planes hold the whole block grid, then applyGainMap on its W x h pixels."""
    factors, fmt, _ = SAMPLINGS[sampling]
    dims = K.grids(W, h, factors)
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    wp = max(bw * 8 * hmax // f[0] for (bw, _), f in zip(dims, factors))
    hp = max(bh * 8 * vmax // f[1] for (_, bh), f in zip(dims, factors))
    img = Image(fmt, wp, hp, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=16, device=DEV)
    for c in range(3):
        pl = img.plane_tensor(c)
        assert pl.shape[0] >= dims[c][1] * 8 and pl.shape[1] >= dims[c][0] * 8
        uhdr.idct_dequant(dcoefs[c], qts[c], plane=pl, stride=pl.shape[1])
    img.raw.w, img.raw.h = W, h
    img.w, img.h = W, h
    dest = Image(F16, W, h, align=4, device=DEV)
    uhdr.applyGainMap(img, gm_dev, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest)
    uhdr.ctx.synchronize()
    return dest


@pytest.mark.parametrize("sampling,ch,scale", [("420", 1, 1), ("420", 1, 2), ("422", 3, 1), ("444", 1, 1)])
def test_waves_take_a_second_tile(uhdr, sampling, ch, scale):
    import torch

    dcoefs, qts, h = coef_case(sampling)
    rows = SAMPLINGS[sampling][2]
    tiles = -(-W // 128) * -(-h // rows)
    print(f"{sampling}: {W} x {h}, {tiles} tiles against at most {walker_bound()} walking waves")
    assert tiles > walker_bound(), "no wave can reach a second tile"
    assert h % 2 == 0 and h % rows != 0 and W % 128 != 0
    gm = synth.make_gainmap(W // scale, h // scale, ch, cg=A.UHDR_CG_BT_2100).to(DEV)
    md = synth.default_metadata(use_base_cg=0, per_channel=(ch == 3))
    dest = Image(F16, W, h, align=4, device=DEV)
    if sampling == "444":
        uhdr.applyGainMapFromCoefficients444(dcoefs, qts, W, h, A.UHDR_CG_BT_709, gm, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest)
    else:
        uhdr.applyGainMapFromCoefficients(dcoefs, qts, W, h, A.UHDR_CG_BT_709, gm, md, A.UHDR_CT_LINEAR, F16, A.FLT_MAX, dest, sampling=sampling)
    uhdr.ctx.synchronize()
    want = staged(uhdr, dcoefs, qts, h, sampling, gm, md)
    assert int(torch.count_nonzero(want.buf)) > want.buf.numel() // 8  # the reference wrote an image
    assert torch.equal(dest.buf, want.buf)
