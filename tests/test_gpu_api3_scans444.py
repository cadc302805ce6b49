"""GPU: the one-call API-3 encode (uhdr_hip_encode_api3_scans_dev) on a 4:4:4 SDR intent with the route forced.
UHDR_HIP_API3_ROUTE=fused takes the coefficient kernel (generate_coef.hip on 128 x 8 pixel tiles: no IDCT launch), =staged the planes
route (three IDCT launches + generate_gainmap); the map's scan, the metadata and the description are the same on either and equal the
staged chain of public entry points (tests/test_gpu_api3_scans.py::staged_chain).  The variable is read on every call, so the test sets
it in process.  The HDR intents are kept for this module only and released with it, so that the tests that follow find the device
allocator as the tests before left it."""
import gc

import pytest

import test_gpu_api3_scans as S
from libultrahdr_amd import capi as A

pytestmark = pytest.mark.gpu
BEST, REALTIME = A.UHDR_USAGE_BEST_QUALITY, A.UHDR_USAGE_REALTIME
# (channels, (scale factor, w, h)): three channels at 256 x 144 with S = 1, one channel at 512 x 288 with S = 4
CASES = ((3, S.GEOMETRIES[0]), (1, S.GEOMETRIES[1]))


_hdr = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_data():
    yield
    _hdr.clear()
    gc.collect()


@pytest.fixture(autouse=True)
def _own_hdr_intents(monkeypatch):
    """one_call_dev and staged_chain of the existing module take their HDR intent from its hdr_case: the same images, kept here."""
    make = S.hdr_case.__wrapped__  # the function under that module's lru_cache

    def hdr_case(w, h):
        if (w, h) not in _hdr:
            _hdr[(w, h)] = make(w, h)
        return _hdr[(w, h)]

    monkeypatch.setattr(S, "hdr_case", hdr_case)


@pytest.fixture()
def prof_ctx():
    """A context of its own with the launch profile on: the shared one stays as the other tests expect it."""
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)
    ctx.profile(True)  # uhdr_hip_profile_enable
    try:
        yield ctx
    finally:
        ctx.close()


def routed(monkeypatch, ctx, route, u, w, h):
    """(result of the _dev one-call form with the route forced, IDCT launches it made)."""
    monkeypatch.setenv("UHDR_HIP_API3_ROUTE", route)
    ctx.profile_read(None, reset=True)
    got = S.one_call_dev(u, w, h, "444")
    n_idct = ctx.profile_read("idct_dequant", reset=False)[0]
    n_gen = ctx.profile_read("generate_gainmap", reset=False)[0]
    ctx.profile_read(None, reset=True)
    assert n_gen >= 1, "the profile recorded no generation launch: the launch counts below would say nothing"
    return got, n_idct


@pytest.mark.parametrize("preset", [BEST, REALTIME], ids=["two-pass", "one-pass"])
def test_either_forced_route_gives_the_staged_chains_bytes(monkeypatch, prof_ctx, preset):
    for nch, (scale, w, h) in CASES:
        u = S.uhdr_for(prof_ctx, scale, nch, preset)
        monkeypatch.delenv("UHDR_HIP_API3_ROUTE", raising=False)
        want = S.staged_chain(u, w, h, "444")
        assert want[2][:3] == (A.UHDR_IMG_FMT_24bppRGB888 if nch == 3 else A.UHDR_IMG_FMT_8bppYCbCr400, w // scale, h // scale)
        fused, n_fused = routed(monkeypatch, prof_ctx, "fused", u, w, h)
        staged, n_staged = routed(monkeypatch, prof_ctx, "staged", u, w, h)
        what = f"444 ch={nch} S={scale}"
        assert n_fused == 0, f"{what}: UHDR_HIP_API3_ROUTE=fused made {n_fused} IDCT launches: the coefficient kernel did not run"
        assert n_staged == 3, f"{what}: UHDR_HIP_API3_ROUTE=staged made {n_staged} IDCT launches"
        for name, got in (("fused", fused), ("staged", staged)):
            assert len(got[0]) == len(want[0]) and got[0] == want[0], f"{what} {name}: map scans differ ({len(got[0])} / {len(want[0])} bytes)"
            assert got[1] == want[1], f"{what} {name}: metadata {got[1]} != {want[1]}"
            assert got[2] == want[2], f"{what} {name}: description {got[2]} != {want[2]}"


def test_a_geometry_the_coefficient_operator_declines_goes_through_planes(monkeypatch, prof_ctx):
    """Scale factor 8 is outside the coefficient operator's 1 / 2 / 4 (UNSUPPORTED_FEATURE): with the route forced to fused the call still
    succeeds, through three IDCT launches, and equals the staged chain.  256 x 192 at 8 is a 32 x 24 map, whole 8 x 8 blocks (256 x 144
    would leave 18 rows at 8 and 9 at 16, which the chain refuses as a ragged map whatever the route)."""
    scale, w, h = 8, 256, 192
    for preset in (BEST, REALTIME):
        u = S.uhdr_for(prof_ctx, scale, 1, preset)
        monkeypatch.delenv("UHDR_HIP_API3_ROUTE", raising=False)
        want = S.staged_chain(u, w, h, "444")
        assert want[2][1:3] == (32, 24)
        got, n_idct = routed(monkeypatch, prof_ctx, "fused", u, w, h)
        assert n_idct == 3
        assert got == want
