"""The fused API-0 front ends at gain-map scale factors 2 and 4 against the staged route, at 3840 x 2176 (the map is whole 8 x 8 blocks at
both scale factors), one pass:

    RGBA1010102 PQ BT.2100   three channels, S = 2        uhdr_hip_encode_api0_fused_scaled_dev
    RGBA1010102 PQ BT.2100   one channel,    S = 4          vs  uhdr_hip_tone_map_dev + uhdr_hip_generate_gainmap_dev
                                                                + uhdr_hip_convert_raw_input_to_ycbcr_dev
    P010 HLG BT.2100         three channels, S = 2        uhdr_hip_encode_api0_p010_fused_scaled_dev
    P010 HLG BT.2100         one channel,    S = 4          vs  uhdr_hip_tone_map_dev + uhdr_hip_generate_gainmap_dev

    python tools/api0_scaled_time.py [--iters 50] [--rounds 5] [--json profiles/api0_scaled_time.json]

Per case, on the same device-resident intent, into preallocated device images, arguments marshalled once:
  (a) launches   the library's own event pair around each launch (uhdr_hip_profile_*): the fused launch against the sum of the staged ones;
  (b) calls      HIP events on the context's stream around a loop of calls: the new _dev call against the staged calls.
The two routes alternate, `rounds` times in one process, each loop behind its own warm-up; the median round is reported next to every
round and the spread (largest - smallest round).  The yardstick is the staged route of the same run: a case meets the bar when the fused
median lies below the staged median by more than the two spreads added.  The outputs of the two routes are compared for equality at the
timed size before anything is timed.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from api0_p010_time import event_ms, kernel_ms  # noqa: E402  (the same two clocks)

W, H = 3840, 2176
CASES = [("RGBA1010102 PQ BT.2100", 3, 2), ("RGBA1010102 PQ BT.2100", 1, 4), ("P010 HLG BT.2100", 3, 2), ("P010 HLG BT.2100", 1, 4)]


def verdict(fused, staged):
    """medians, spreads over the rounds, and the bar: fused median below the staged median by more than the two spreads added"""
    mf, ms = float(np.median(fused)), float(np.median(staged))
    sf, ss = float(max(fused) - min(fused)), float(max(staged) - min(staged))
    return dict(fused_ms=mf, staged_ms=ms, fused_spread_ms=sf, staged_spread_ms=ss, staged_over_fused=ms / mf, meets_bar=bool(ms - mf > sf + ss),
                fused_rounds_ms=list(fused), staged_rounds_ms=list(staged))


def bytes_per_pixel(p010, nch, s):
    """(fused, staged) HBM bytes per pixel the algorithm needs"""
    m = nch / float(s * s)
    if p010:  # tone map 3 + 1.5; generate 1.5 + 3 + map
        return 3 + 1.5 + m, (3 + 1.5) + (1.5 + 3 + m)
    return 4 + 3 + m, (4 + 4) + (4 + 4 + m) + (4 + 3)  # tone map 4 + 4; generate 4 + 4 + map; convert 4 + 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    lib, check, ordered = ctx.lib, A.check, ctx.ordered
    intents = {"RGBA1010102 PQ BT.2100": synth.make_hdr_rgba1010102(W, H, ct=A.UHDR_CT_PQ, cg=A.UHDR_CG_BT_2100).to("cuda:0"),
               "P010 HLG BT.2100": synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100).to("cuda:0")}
    rows = []
    for name, nch, s in CASES:
        dh = intents[name]
        p010 = dh.fmt == A.UHDR_IMG_FMT_24bppYCbCrP010
        u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=s, useMultiChannelGainMap=nch == 3, preset=A.UHDR_USAGE_REALTIME)
        cfg = u.encode_cfg(False, False)
        fmap = A.UHDR_IMG_FMT_24bppRGB888 if nch == 3 else A.UHDR_IMG_FMT_8bppYCbCr400
        fbase = A.UHDR_IMG_FMT_12bppYCbCr420 if p010 else A.UHDR_IMG_FMT_24bppYCbCr444
        dev = dict(align=64, device="cuda:0")
        base_f, base_s = Image(fbase, W, H, **dev), Image(fbase, W, H, **dev)
        gm_f, gm_s = Image(fmap, W // s, H // s, **dev), Image(fmap, W // s, H // s, **dev)
        md_f, md_s = A.GainmapMetadata(), A.GainmapMetadata()
        if p010:
            a_fused = (ctx.handle, C.byref(dh.raw), C.byref(cfg), C.byref(base_f.raw), C.byref(md_f), C.byref(gm_f.raw))
            a_tone = (ctx.handle, C.byref(dh.raw), C.byref(base_s.raw))
            a_gen = (ctx.handle, C.byref(base_s.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm_s.raw))
            families = ("tone_map", "generate_gainmap")

            def fused():
                with ordered():
                    check(lib.uhdr_hip_encode_api0_p010_fused_scaled_dev(*a_fused))

            def staged():
                with ordered():
                    check(lib.uhdr_hip_tone_map_dev(*a_tone))
                    check(lib.uhdr_hip_generate_gainmap_dev(*a_gen))
        else:  # (no RGBA8888 rendition out of the fused call: JpegR::encodeJPEGR does not keep it either)
            sdr_s = Image(A.UHDR_IMG_FMT_32bppRGBA8888, W, H, **dev)
            a_fused = (ctx.handle, C.byref(dh.raw), C.byref(cfg), None, C.byref(base_f.raw), C.byref(md_f), C.byref(gm_f.raw))
            a_tone = (ctx.handle, C.byref(dh.raw), C.byref(sdr_s.raw))
            a_gen = (ctx.handle, C.byref(sdr_s.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm_s.raw))
            a_conv = (ctx.handle, C.byref(sdr_s.raw), 0, C.byref(base_s.raw))
            families = ("tone_map", "generate_gainmap", "convert_raw_input_to_ycbcr")

            def fused():
                with ordered():
                    check(lib.uhdr_hip_encode_api0_fused_scaled_dev(*a_fused))

            def staged():
                with ordered():
                    check(lib.uhdr_hip_tone_map_dev(*a_tone))
                    check(lib.uhdr_hip_generate_gainmap_dev(*a_gen))
                    check(lib.uhdr_hip_convert_raw_input_to_ycbcr_dev(*a_conv))

        fused()
        staged()
        ctx.synchronize()
        identical = (bool((base_f.buf == base_s.buf).all().item()) and bool((gm_f.buf == gm_s.buf).all().item()) and md_f.as_dict() == md_s.as_dict() and
                     (gm_f.raw.w, gm_f.raw.h) == (gm_s.raw.w, gm_s.raw.h) == (W // s, H // s))
        kf, ks, tf, ts = [], [], [], []
        for _ in range(args.rounds):  # alternating, each loop behind its own warm-up
            kf.append(kernel_ms(ctx, fused, args.iters, ("encode_api0_fused",)))
            ks.append(kernel_ms(ctx, staged, args.iters, families))
        for _ in range(args.rounds):
            tf.append(event_ms(ctx, fused, args.iters))
            ts.append(event_ms(ctx, staged, args.iters))
        bf, bs = bytes_per_pixel(p010, nch, s)
        row = dict(size=f"{W}x{H}", intent=name, channels=nch, scale=s, identical_outputs=identical, launches=verdict(kf, ks), calls=verdict(tf, ts),
                   fused_bytes_per_pixel=bf, staged_bytes_per_pixel=bs)
        row["fused_algorithmic_GBps"] = bf * W * H / row["launches"]["fused_ms"] / 1e6
        row["staged_algorithmic_GBps"] = bs * W * H / row["launches"]["staged_ms"] / 1e6
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["identical_outputs"] for r in rows):
        sys.exit("the two routes' outputs differ")


if __name__ == "__main__":
    main()
