"""The one-call decode to HDR (uhdr_hip_decode_api1_scans_dev: both scans entropy-decoded, the map's IDCT, applyGainMap with the
base image's dequantize + IDCT inside the kernel) against the staged route on the same device-resident scans, at 3840 x 2160:

    fused    UltraHdr.decodeApi1Scans (arguments marshalled once: bindDecodeApi1Scans); for a 4:4:4 base image the same call of
             uhdr_hip_decode_api1_scans_any_dev, marshalled once here
    staged   huffman_decode2 (both scans, concurrently, as the one-call decode does), the map's IDCT, three idct_dequant launches into
             a planar base image, applyGainMap on the planes -- what a caller had to do for a 4:2:2 base image before the
             coefficient-input kernel took that sampling (2 B/px of planes written to HBM and read back; 3 B/px for 4:4:4)

    python tools/hdr_decode_time.py --sampling 422 [--iters 30] [--rounds 3] [--json out.json]
    --sampling 420 | 422 | 444 | both | all    the base image's sampling (both: 4:2:0 and 4:2:2 in one run, all: the three, so that
                                               the 4:2:0 figures are a reference point taken under the same conditions)

Times are HIP events on the context's stream around a loop of calls, each loop behind its own warm-up of the same calls; the two
routes alternate, `rounds` times, and the median round is reported next to the spread.  The entropy stage synchronises with the
host, so an event interval here is a per-call time (host work between the launches included), not a kernel time.  Maps: one
channel at scale 4 (the library's default) and three channels at scale 1 (bench.py's headline); output linear RGBA half float.
The two routes' pixels are compared at the timed size before anything is timed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
S444 = [(1, 1)] * 3
SAMPLING = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": S444}


def grids(w, h, sampling):
    """[(blocks_h, blocks_w)] per component: libjpeg's height_in_blocks / width_in_blocks."""
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-h * vs // vmax) + 7) // 8, (-(-w * hs // hmax) + 7) // 8) for hs, vs in sampling]


def make_scan(u, w, h, sampling, qts, rng, lo, hi):
    """A smooth field + noise per component -> FDCT + quantization and Huffman coding on the device: (scan bytes, header)."""
    import torch

    coefs = []
    for c, (bh, bw) in enumerate(grids(w, h, sampling)):
        yy, xx = np.mgrid[0:bh * 8, 0:bw * 8].astype(np.float32)
        pl = (lo + hi) / 2 + (hi - lo) / 2 * np.sin(xx / (41.0 + 13 * c)) * np.cos(yy / (29.0 + 7 * c)) + rng.normal(0, 3, (bh * 8, bw * 8))
        pl = torch.from_numpy(np.clip(pl, 0, 255).astype(np.uint8)).to("cuda:0")
        coefs.append(u.fdct_quant(pl, bw * 8, bw, bh, qts[c]))
    return u.huffman_encode(coefs, w, h, sampling, 0).clone(), u.jpeg_header(w, h, sampling, qts)


def event_ms(ctx, fn, iters):
    """Per-call milliseconds: events on the context's stream around `iters` calls, behind a warm-up of the same call."""
    import torch

    for _ in range(3):
        fn()
    ctx.synchronize()
    _, stream = ctx._streams()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bind_any(u, base_hdr, base_data, base_cg, map_hdr, map_data, map_cg, md, output_ct, output_format, max_display_boost, dest):
    """UltraHdr.decodeApi1ScansAny with the arguments marshalled once, as bindDecodeApi1Scans does for decodeApi1Scans."""
    import ctypes as C

    from libultrahdr_amd import capi as A

    fn = u.lib.uhdr_hip_decode_api1_scans_any_dev
    args = (u.ctx.handle, C.byref(base_hdr), C.c_void_p(base_data.data_ptr()), int(base_data.numel()), base_cg, C.byref(map_hdr),
            C.c_void_p(map_data.data_ptr()), int(map_data.numel()), map_cg, 0, C.byref(md), output_ct, output_format, max_display_boost, C.byref(dest.raw))
    ordered, check = u.ctx.ordered, A.check

    def run(_keep=(base_hdr, base_data, map_hdr, map_data, md, dest)):
        with ordered():
            check(fn(*args))

    return run


def case(u, ctx, sampling, nch, scale, iters, rounds, rng):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image

    f16 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat
    planar = {"420": A.UHDR_IMG_FMT_12bppYCbCr420, "422": A.UHDR_IMG_FMT_16bppYCbCr422, "444": A.UHDR_IMG_FMT_24bppYCbCr444}[sampling]
    qy, qc = u.quant_table(90, False), u.quant_table(90, True)
    qts = [qy, qc, qc]
    samp = SAMPLING[sampling]
    scan_b, hb = make_scan(u, W, H, samp, qts, rng, 20, 235)
    mw, mh = W // scale, H // scale
    msamp = S444 if nch == 3 else [(1, 1)]
    scan_m, hm = make_scan(u, mw, mh, msamp, qts[:nch], rng, 60, 200)
    md = synth.default_metadata(use_base_cg=0, per_channel=(nch == 3))
    base_cg, map_cg = A.UHDR_CG_BT_709, A.UHDR_CG_BT_2100
    d_fused, d_staged = Image(f16, W, H, align=64, device="cuda:0"), Image(f16, W, H, align=64, device="cuda:0")
    bind = (lambda *a: bind_any(u, *a)) if sampling == "444" else u.bindDecodeApi1Scans  # the first entry point refuses 4:4:4
    fused = bind(hb, scan_b, base_cg, hm, scan_m, map_cg, md, A.UHDR_CT_LINEAR, f16, A.FLT_MAX, d_fused)

    shp_b, shp_m = grids(W, H, samp), grids(mw, mh, msamp)
    base = Image(planar, W, H, base_cg, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=64, device="cuda:0")  # 3840 x 2160: whole blocks
    assert W % 128 == 0 and H % 8 == 0 and (sampling != "420" or H % 16 == 0)
    if nch == 3:
        gm = Image(A.UHDR_IMG_FMT_32bppRGBA8888, mw, mh, map_cg, align=64, device="cuda:0")
    else:
        gm = Image(A.UHDR_IMG_FMT_8bppYCbCr400, mw, (mh + 7) // 8 * 8, map_cg, align=64, device="cuda:0")  # rows of whole blocks
        gm.raw.h = mh

    def staged():
        kb, km = u.huffman_decode2(scan_b, shp_b, W, H, samp, scan_m, shp_m, mw, mh, msamp, 0)
        if nch == 3:
            u.idct_dequant_rgb(km, qy, qc, mw, mh, A.UHDR_IMG_FMT_32bppRGBA8888, 0, dst=gm)
        else:
            pl = gm.plane_tensor(0)
            u.idct_dequant(km[0], qy, plane=pl, stride=pl.shape[1])
        for c in range(3):
            pl = base.plane_tensor(c)
            u.idct_dequant(kb[c], qts[c], plane=pl, stride=pl.shape[1])
        u.applyGainMap(base, gm, md, A.UHDR_CT_LINEAR, f16, A.FLT_MAX, d_staged)

    fused()
    staged()
    ctx.synchronize()
    identical = bool((d_fused.buf == d_staged.buf).all().item())
    tf, ts = [], []
    for _ in range(rounds):  # alternating, each loop behind its own warm-up
        tf.append(event_ms(ctx, fused, iters))
        ts.append(event_ms(ctx, staged, iters))
    f, s = float(np.median(tf)), float(np.median(ts))
    return dict(sampling=sampling, size=f"{W}x{H}", map=f"{nch} channel(s) at scale {scale}", base_scan_bytes=int(scan_b.numel()),
                map_scan_bytes=int(scan_m.numel()), fused_ms=f, staged_ms=s, staged_over_fused=s / f, fused_rounds_ms=tf, staged_rounds_ms=ts,
                identical_pixels=identical)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampling", default="422", choices=("420", "422", "444", "both", "all"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    u = UltraHdr(ctx=ctx)
    rows = []
    for s in {"both": ("420", "422"), "all": ("420", "422", "444")}.get(args.sampling, (args.sampling,)):
        for nch, scale in ((1, 4), (3, 1)):
            rows.append(case(u, ctx, s, nch, scale, args.iters, args.rounds, np.random.default_rng(7)))
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
