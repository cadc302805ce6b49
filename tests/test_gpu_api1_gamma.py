"""GPU: the fused API-1 encode with a gain-map gamma other than 1 (uhdr_hip_encode_api1_scans_ex / _ex_dev with
UHDR_HIP_GENERATE_GAMMA_TABLE).  The yardstick is the staged chain run with the same flag -- generateGainMapEx (held to the oracle under the
gamma-1 bar by test_gpu_generate_gamma.py), fdct_quant / fdct_quant_rgb of the map, convertYuv + fdct_quant x 3 of the base image (or the
RGBA8888 route of test_gpu_api1_rgba.py), huffman_encode for the two scans -- and every comparison against it is for equality: both scans
byte for byte, their sizes, the metadata and the gain-map description.  (The scans entry points return no map image: the map's bytes are
compared through the map scan, which codes nothing else.)"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_api1_rgba as R
from libultrahdr_amd import capi as A
from libultrahdr_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RGBA, P3, UNSPEC = R.RGBA, R.P3, R.UNSPEC
HLG = A.UHDR_CT_HLG
REALTIME, BEST = A.UHDR_USAGE_REALTIME, A.UHDR_USAGE_BEST_QUALITY
UNSUP, INVAL = A.UHDR_CODEC_UNSUPPORTED_FEATURE, A.UHDR_CODEC_INVALID_PARAM
FLAG = A.UHDR_HIP_GENERATE_GAMMA_TABLE
GAMMA = 1.571


def _routes(hip_ctx):
    st = A.Stats()
    hip_ctx.lib.uhdr_hip_get_stats(hip_ctx.handle, C.byref(st))
    return np.array([st.generate_channels_tabled, st.generate_channels_per_sample], dtype=np.int64)


def _staged_scans(hip_ctx, u, sdr, ds, dh, enc, qb, qm, flags):
    """(base scan, map scan, metadata, map image) of the staged chain; sdr: the host image ds came from (convertYuv works in place)."""
    w, h = ds.w, ds.h
    md, gm = u.generateGainMapEx(ds, dh, flags)
    if ds.fmt == RGBA:
        img, cdiv, samp = u.convert_raw_input_to_ycbcr(ds, False), 8, R.SAMP444
    else:
        img, cdiv, samp = sdr.to(DEV), 16, R.SAMP420
    if enc != UNSPEC:
        u.convertYuv(img, sdr.raw.cg, enc)
    base = [u.fdct_quant(img.plane_tensor(i), img.raw.stride[i], w // (cdiv if i else 8), h // (cdiv if i else 8), qb[1 if i else 0]) for i in range(3)]
    if gm.raw.fmt == A.UHDR_IMG_FMT_24bppRGB888:
        mapc = list(u.fdct_quant_rgb(gm, qm[0], qm[1]))
    else:
        mapc = [u.fdct_quant(gm.plane_tensor(0), gm.raw.stride[0], gm.w // 8, gm.h // 8, qm[0])]
    eb = u.huffman_encode(base, w, h, samp, 0)
    em = u.huffman_encode(mapc, gm.w, gm.h, [(1, 1)] * len(mapc), 0)
    hip_ctx.synchronize()
    return eb.cpu().numpy().tobytes(), em.cpu().numpy().tobytes(), md, gm


def _check_scans(hip_ctx, u, sdr, hdr, enc=P3, flags=FLAG):
    import torch

    w, h = sdr.w, sdr.h
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    want_b, want_m, md_s, gm_s = _staged_scans(hip_ctx, u, sdr, ds, dh, enc, qb, qm, flags)
    n = w * h * 3 + 4096
    ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    nb, nm, md_d = u.encodeApi1ScansEx(ds, dh, enc, qb, qm, ob, om, flags)
    hip_ctx.synchronize()
    assert (nb, nm) == (len(want_b), len(want_m))
    assert ob[:nb].cpu().numpy().tobytes() == want_b, "base scan (device form)"
    assert om[:nm].cpu().numpy().tobytes() == want_m, "map scan (device form)"
    assert md_d.as_dict() == md_s.as_dict()
    base, mp, md_h, desc = u.encodeApi1ScansEx(sdr, hdr, enc, qb, qm, n, n, flags)
    assert base == want_b, "base scan (host form)"
    assert mp == want_m, "map scan (host form)"
    assert md_h.as_dict() == md_s.as_dict()
    assert (desc.fmt, desc.w, desc.h, desc.cg, desc.ct, desc.range) == (gm_s.raw.fmt, gm_s.w, gm_s.h, hdr.raw.cg, hdr.raw.ct, hdr.raw.range)
    assert list(md_s.gamma) == [np.float32(u.mGamma)] * 3
    return md_s, gm_s


def _pair(w, h, rgba=False):
    sdr = synth.make_sdr_rgba8888(w, h, seed=w + 2 * h, noise=0.05) if rgba else synth.make_sdr_yuv420(w, h, seed=w + 2 * h, noise=0.05)
    return sdr, synth.make_hdr_p010(w, h, seed=w + 3 * h, ct=HLG, noise=0.05)


@pytest.mark.parametrize("w,h", [(144, 48), (208, 112)])
def test_best_quality_three_channels_equals_the_staged_chain(hip_ctx, w, h):
    """Two pass, three channels, scale 1; 208 x 112 has 26 map blocks per row: three full groups of eight and a ragged one.  The range
    kernel builds the ratio -> byte tables from the gamma's thresholds (the table route is counted)."""
    u = R._uhdr(hip_ctx, 1, True, preset=BEST, gamma=GAMMA)
    before = _routes(hip_ctx)
    _check_scans(hip_ctx, u, *_pair(w, h))
    rose = _routes(hip_ctx) - before
    # the staged call, the device form, the host form: three channels each, and the same route in all three (a channel whose range falls
    # between two bucket widths may be declined a table: a correct outcome, but not for every channel)
    assert rose[0] >= 3 and rose.sum() == 9 and rose[0] % 3 == 0, rose


def test_one_pass_one_channel_scale_four_equals_the_staged_chain(hip_ctx):
    u = R._uhdr(hip_ctx, 4, False, preset=REALTIME, gamma=GAMMA)
    md, gm = _check_scans(hip_ctx, u, *_pair(544, 96))
    assert (gm.w, gm.h) == (136, 24) and list(md.min_content_boost) == [1.0] * 3


@pytest.mark.parametrize("preset", [REALTIME, BEST])
def test_rgba8888_sdr_equals_the_staged_chain(hip_ctx, preset):
    u = R._uhdr(hip_ctx, 1, True, preset=preset, gamma=GAMMA)
    _check_scans(hip_ctx, u, *_pair(144, 48, rgba=True))


def test_best_quality_with_a_range_too_dense_for_tables_takes_the_per_sample_thresholds(hip_ctx):
    """min 2.0 / max 2.0002: no channel gets a table, map_blocks_kernel's per-sample tail searches the thresholds."""
    u = R._uhdr(hip_ctx, 1, True, preset=BEST, gamma=GAMMA, minContentBoost=2.0, maxContentBoost=2.0002)
    before = _routes(hip_ctx)
    _check_scans(hip_ctx, u, *_pair(144, 48))
    rose = _routes(hip_ctx) - before
    assert rose[0] == 0 and rose[1] == 9, rose


def test_flags_zero_with_a_gamma_is_refused_with_nothing_written(hip_ctx):
    import torch

    w, h = 144, 48
    sdr, hdr = _pair(w, h)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    n = w * h * 3 + 4096
    for preset in (REALTIME, BEST):
        u = R._uhdr(hip_ctx, 1, True, preset=preset, gamma=GAMMA)
        qbb, qmm, cfg, md = u._qt_pair(qb), u._qt_pair(qm), u.encode_cfg(), A.GainmapMetadata()
        for flags, code, text in ((0, UNSUP, b"needs gain-map gamma 1"), (0x2, INVAL, b"flag"), (FLAG | 0x10, INVAL, b"flag")):
            ob, om = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV), torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
            nb, nm = C.c_size_t(0), C.c_size_t(0)
            with hip_ctx.ordered():
                st = hip_ctx.lib.uhdr_hip_encode_api1_scans_ex_dev(hip_ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                                   C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(ob.data_ptr()), n, C.byref(nb),
                                                                   C.c_void_p(om.data_ptr()), n, C.byref(nm), flags)
            hip_ctx.synchronize()
            assert st.error_code == code and text in st.detail, (flags, st.error_code, st.detail)
            assert bool((ob == 0xA5).all()) and bool((om == 0xA5).all()) and (nb.value, nm.value) == (0, 0)
            hb, hm = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
            st = hip_ctx.lib.uhdr_hip_encode_api1_scans_ex(hip_ctx.handle, C.byref(sdr.raw), C.byref(hdr.raw), C.byref(cfg), P3, C.c_void_p(qbb.ctypes.data),
                                                           C.c_void_p(qmm.ctypes.data), C.byref(md), None, C.c_void_p(hb.ctypes.data), n, C.byref(nb),
                                                           C.c_void_p(hm.ctypes.data), n, C.byref(nm), flags)
            assert st.error_code == code and text in st.detail, (flags, st.error_code, st.detail)
            assert (hb == 0xA5).all() and (hm == 0xA5).all() and (nb.value, nm.value) == (0, 0)


@pytest.mark.parametrize("preset", [REALTIME, BEST])
def test_gamma_one_with_the_flag_is_the_onepass_sibling(hip_ctx, preset):
    import torch

    w, h = 144, 48
    sdr, hdr = _pair(w, h)
    ds, dh = sdr.to(DEV), hdr.to(DEV)
    qb, qm = R._tables()
    u = R._uhdr(hip_ctx, 1, True, preset=preset)
    n = w * h * 3 + 4096
    outs = [torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(4)]
    nb_a, nm_a, md_a = u.encodeApi1ScansEx(ds, dh, P3, qb, qm, outs[0], outs[1], FLAG)
    nb_b, nm_b, md_b = u.encodeApi1ScansOnePass(ds, dh, P3, qb, qm, outs[2], outs[3])
    hip_ctx.synchronize()
    assert (nb_a, nm_a) == (nb_b, nm_b) and nb_a > 0 and nm_a > 0 and md_a.as_dict() == md_b.as_dict()
    assert torch.equal(outs[0][:nb_a], outs[2][:nb_b]) and torch.equal(outs[1][:nm_a], outs[3][:nm_b])
    host_a, host_b = u.encodeApi1ScansEx(sdr, hdr, P3, qb, qm, n, n, FLAG), u.encodeApi1ScansOnePass(sdr, hdr, P3, qb, qm, n, n)
    assert host_a[:2] == host_b[:2] and host_a[2].as_dict() == host_b[2].as_dict()
    host_0 = u.encodeApi1ScansEx(sdr, hdr, P3, qb, qm, n, n, 0)
    assert host_0[:2] == host_b[:2] and host_0[2].as_dict() == host_b[2].as_dict()
