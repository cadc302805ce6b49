"""The fused API-1 encode for the one-pass (real-time) preset against the staged route, at 3840 x 2176 (the map is whole 8 x 8 blocks at
scale factor 4 too), everything device resident:

    P010 HLG BT.2100 + YCbCr 4:2:0 BT.709        three channels, S = 1
    P010 HLG BT.2100 + YCbCr 4:2:0 BT.709        one channel,    S = 1
    P010 HLG BT.2100 + YCbCr 4:2:0 BT.709        one channel,    S = 4   (the legacy JpegR() defaults)
    RGBA1010102 PQ BT.2100 + RGBA8888 BT.709     three channels, S = 1

    python tools/api1_onepass_time.py [--iters 50] [--rounds 5] [--json profiles/api1_onepass_time.json]

Per row, on the same device-resident intents, into preallocated device buffers, arguments marshalled once:
  (a) launches   the gain map's side inside the launches (the library's own event pair around each launch, uhdr_hip_profile_*):
                 map_blocks_onepass_kernel inside uhdr_hip_encode_api1_fused_onepass_dev  against  one-pass uhdr_hip_generate_gainmap_dev +
                 uhdr_hip_fdct_quant_dev (one channel) or uhdr_hip_fdct_quant_rgb_dev (three).  The base image's launch is the siblings' own
                 and is on neither side; for this clock it is kept off the auxiliary stream (UHDR_HIP_NO_CHAIN_OVERLAP), so that the
                 map's launch has the device to itself as the staged launches have.
  (b) calls      a host clock around calls that end synchronised: uhdr_hip_encode_api1_scans_onepass_dev  against  the staged route to the
                 same two scans -- generate_gainmap, the map's FDCT, the base image's blocks through the operators (4:2:0: a copy, since
                 convertYuv works in place, convertYuv, 3 x fdct_quant; RGBA8888: convert_raw_input_to_ycbcr, convertYuv, 3 x fdct_quant)
                 and uhdr_hip_huffman_encode2_dev.
  (c) fetch      the 4:2:0 + P010 rows at scale 1 only, same clock as (a), same images: the map's launch with the vector fetch the launcher
                 picks for these rows  against  the same launch through the per-sample instantiation (UHDR_HIP_ONEPASS_NO_VECTOR_FETCH).
The routes alternate, `rounds` times in one process, each loop behind its own warm-up; the median round is reported next to every
round and the spread (largest - smallest round).  The yardstick is the other route of the same run, and the bar is the same for every
pair: the first median lies below the second by more than the two spreads added.  A row's verdict ("meets_bar") is that of (b), the
call: it is what a caller -- and the facade's seam -- replaces.  (a) is reported with its own flag for what it says about the kernel, and
(c) decides whether the vector fetch stays in the library.  Coefficients, metadata and scans of the two routes are compared for equality
at the timed size before anything is timed.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from api0_p010_time import kernel_ms, wall_ms  # noqa: E402  (the same clocks)
from api0_scaled_time import verdict  # noqa: E402  (medians, spreads, the bar)

W, H = 3840, 2176
CASES = [("P010 HLG BT.2100 + YCbCr 4:2:0", 3, 1), ("P010 HLG BT.2100 + YCbCr 4:2:0", 1, 1), ("P010 HLG BT.2100 + YCbCr 4:2:0", 1, 4),
         ("RGBA1010102 PQ BT.2100 + RGBA8888", 3, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    lib, check, ordered = ctx.lib, A.check, ctx.ordered
    dev, enc = "cuda:0", A.UHDR_CG_DISPLAY_P3
    pairs = {CASES[0][0]: (synth.make_sdr_yuv420(W, H), synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100)),
             CASES[3][0]: (synth.make_sdr_rgba8888(W, H), synth.make_hdr_rgba1010102(W, H, ct=A.UHDR_CT_PQ, cg=A.UHDR_CG_BT_2100))}
    rows = []
    for name, nch, s in CASES:
        sdr, hdr = pairs[name]
        rgba = sdr.fmt == A.UHDR_IMG_FMT_32bppRGBA8888
        ds, dh = sdr.to(dev), hdr.to(dev)
        u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=s, useMultiChannelGainMap=nch == 3, preset=A.UHDR_USAGE_REALTIME)
        cfg = u.encode_cfg()
        mw, mh = W // s, H // s
        cdiv = 8 if rgba else 16
        qb = (u.quant_table(95, False), u.quant_table(95, True))
        qm = (u.quant_table(85, False), u.quant_table(85, True))
        qbb, qmm = u._qt_pair(qb), u._qt_pair(qm)
        qt = lambda t: (C.c_uint16 * 64)(*[int(v) for v in t])
        q_bl, q_bc, q_ml, q_mc = qt(qb[0]), qt(qb[1]), qt(qm[0]), qt(qm[1])
        coefs = lambda bh, bw: torch.empty((bh, bw, 64), dtype=torch.int16, device=dev)
        mk_base = lambda: [coefs(H // 8, W // 8), coefs(H // cdiv, W // cdiv), coefs(H // cdiv, W // cdiv)]
        base_f, base_s = mk_base(), mk_base()
        map_f, map_s = [coefs(mh // 8, mw // 8) for _ in range(nch)], [coefs(mh // 8, mw // 8) for _ in range(nch)]
        blocks = A.Api1Blocks()
        for i in range(3):
            blocks.base_coef[i] = base_f[i].data_ptr()
            blocks.map_coef[i] = map_f[i].data_ptr() if i < nch else None
        md_f, md_s = A.GainmapMetadata(), A.GainmapMetadata()
        gm = Image(A.UHDR_IMG_FMT_24bppRGB888 if nch == 3 else A.UHDR_IMG_FMT_8bppYCbCr400, mw, mh, align=64, device=dev)
        work = Image(A.UHDR_IMG_FMT_24bppYCbCr444 if rgba else A.UHDR_IMG_FMT_12bppYCbCr420, W, H, sdr.raw.cg, sdr.raw.ct, sdr.raw.range, align=64, device=dev)
        a_fused = (ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), enc, C.c_void_p(qbb.ctypes.data), C.c_void_p(qmm.ctypes.data),
                   C.byref(blocks), C.byref(md_f), None)
        a_gen = (ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm.raw))

        def fused():
            with ordered():
                check(lib.uhdr_hip_encode_api1_fused_onepass_dev(*a_fused))

        def staged_map():
            with ordered():
                check(lib.uhdr_hip_generate_gainmap_dev(*a_gen))
                if nch == 3:
                    check(lib.uhdr_hip_fdct_quant_rgb_dev(ctx.handle, C.byref(gm.raw), q_ml, q_mc, *[C.c_void_p(m.data_ptr()) for m in map_s]))
                else:
                    check(lib.uhdr_hip_fdct_quant_dev(ctx.handle, C.c_void_p(gm.raw.planes[0]), gm.raw.stride[0], mw // 8, mh // 8, q_ml, C.c_void_p(map_s[0].data_ptr())))

        def staged_base():
            with ordered():
                if rgba:
                    check(lib.uhdr_hip_convert_raw_input_to_ycbcr_dev(ctx.handle, C.byref(ds.raw), 0, C.byref(work.raw)))
                else:
                    check(lib.uhdr_hip_copy_raw_image_dev(ctx.handle, C.byref(ds.raw), C.byref(work.raw)))
                check(lib.uhdr_hip_convert_yuv_dev(ctx.handle, C.byref(work.raw), sdr.raw.cg, enc))
                for i in range(3):
                    d = cdiv if i else 8
                    check(lib.uhdr_hip_fdct_quant_dev(ctx.handle, C.c_void_p(work.raw.planes[i]), work.raw.stride[i], W // d, H // d, q_bc if i else q_bl,
                                                      C.c_void_p(base_s[i].data_ptr())))

        fused()
        staged_map()
        staged_base()
        ctx.synchronize()
        identical = all(torch.equal(a, b) for a, b in zip(base_f + map_f, base_s + map_s)) and md_f.as_dict() == md_s.as_dict()

        # (b) to the two scans, device buffers
        cap = W * H * 3 + (1 << 16)
        ob, om = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        one, chain = {}, {}
        samp_b = [(1, 1)] * 3 if rgba else [(2, 2), (1, 1), (1, 1)]

        def one_call():
            one["r"] = u.encodeApi1ScansOnePass(ds, dh, enc, qb, qm, ob, om)

        def staged_scans():
            staged_map()
            staged_base()
            sb, sm = u.huffman_encode2(base_s, W, H, samp_b, map_s, mw, mh, [(1, 1)] * nch, outs=outs)
            chain["r"] = (int(sb.numel()), int(sm.numel()))

        one_call()
        staged_scans()
        ctx.synchronize()
        nb, nm = one["r"][0], one["r"][1]
        identical = identical and (nb, nm) == chain["r"] and torch.equal(ob[:nb], outs[0][:nb]) and torch.equal(om[:nm], outs[1][:nm])
        identical = identical and one["r"][2].as_dict() == md_s.as_dict()

        vector_fetch = not rgba and s == 1  # 4:2:0 + P010 at scale 1 on 64-aligned rows: the launcher picks the vector fetch
        kf, ks, kg, tf, ts = [], [], [], [], []
        for _ in range(args.rounds):  # alternating, each loop behind its own warm-up
            os.environ["UHDR_HIP_NO_CHAIN_OVERLAP"] = "1"  # the map's launch alone on the device, as the staged launches are
            kf.append(kernel_ms(ctx, fused, args.iters, ("map_blocks_onepass",)))
            if vector_fetch:  # (c) the same launch through the per-sample instantiation
                os.environ["UHDR_HIP_ONEPASS_NO_VECTOR_FETCH"] = "1"
                kg.append(kernel_ms(ctx, fused, args.iters, ("map_blocks_onepass",)))
                del os.environ["UHDR_HIP_ONEPASS_NO_VECTOR_FETCH"]
            del os.environ["UHDR_HIP_NO_CHAIN_OVERLAP"]
            ks.append(kernel_ms(ctx, staged_map, args.iters, ("generate_gainmap", "fdct_quant")))
        it = max(3, args.iters // 5)
        for _ in range(args.rounds):
            tf.append(wall_ms(ctx, one_call, it))
            ts.append(wall_ms(ctx, staged_scans, it))
        row = dict(size=f"{W}x{H}", intents=name, channels=nch, scale=s, identical_outputs=bool(identical), base_scan_bytes=nb, map_scan_bytes=nm,
                   launches=verdict(kf, ks), calls=verdict(tf, ts))
        row["meets_bar"] = row["calls"]["meets_bar"]  # the row's verdict: the call is what a caller, and the facade's seam, replaces
        if vector_fetch:
            v = verdict(kf, kg)
            row["vector_fetch"] = dict(vector_ms=v["fused_ms"], per_sample_ms=v["staged_ms"], vector_spread_ms=v["fused_spread_ms"],
                                       per_sample_spread_ms=v["staged_spread_ms"], per_sample_over_vector=v["staged_over_fused"], meets_bar=v["meets_bar"],
                                       vector_rounds_ms=v["fused_rounds_ms"], per_sample_rounds_ms=v["staged_rounds_ms"])
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
