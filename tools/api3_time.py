"""The API-3 encode from JPEG coefficients against the staged route, device resident, at 3840 x 2176 and 1920 x 1080 with a P010 HLG
BT.2100 intent and a BT.709 SDR intent in coefficient / compressed form:

    4:2:0, 4:2:2 and 4:4:4 SDR intents   x   three channels at S = 1, one channel at S = 4   x   both presets

    python tools/api3_time.py [--iters 20] [--rounds 5] [--json profiles/api3_time.json]

Per row, on the same device-resident data, into preallocated device buffers:
  (a) operators  inside the launches (the library's own event pair around each launch, uhdr_hip_profile_*):
                 uhdr_hip_generate_gainmap_coef_dev / _coef422_dev / _coef444_dev  against  3 x uhdr_hip_idct_dequant_dev + uhdr_hip_generate_gainmap_dev.
                 One pass: that is the first launch alone on either side.  Two pass: both sides carry the same range kernel and pass 2
                 behind their first launch, so the difference is the first launches'.
  (b) calls      a host clock around calls that end synchronised: uhdr_hip_encode_api3_scans_dev with UHDR_HIP_API3_ROUTE=fused  against
                 the staged chain of public entry points -- uhdr_hip_huffman_decode_dev, 3 x uhdr_hip_idct_dequant_dev,
                 uhdr_hip_generate_gainmap_dev (sdr_is_601), uhdr_hip_fdct_quant_dev / _rgb_dev, uhdr_hip_huffman_encode_dev -- and, as a
                 third column, against the same one call with UHDR_HIP_API3_ROUTE=staged (the planes route inside the call).
                 1920 x 1080 at S = 4 has a 480 x 270 map, which is not whole 8 x 8 blocks: the one-call form declines it and the row has
                 column (a) only.
The routes alternate, `rounds` times in one process, each loop behind its own warm-up; the median round is reported next to every round
and the spread (largest - smallest round).  The bar is the same for every pair: the first median lies below the second by more than the
two spreads added.  A row's verdict ("meets_bar") is that of (b) against the staged chain of public entry points: the default route of a
sampling is `fused` only if every row of that sampling that has a (b) meets it.  The third column carries its own flag.  Map scans and metadata of the routes are compared for equality at the timed
size before anything is timed.
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

SIZES = [(3840, 2176), (1920, 1080)]
SAMPLINGS = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1), (1, 1), (1, 1)]}
COEF_ENTRY = {"420": "uhdr_hip_generate_gainmap_coef_dev", "422": "uhdr_hip_generate_gainmap_coef422_dev", "444": "uhdr_hip_generate_gainmap_coef444_dev"}


def grids(w, h, sampling):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8) for hs, vs in sampling]


class Route:
    def __init__(self, route):
        self.route = route

    def __enter__(self):
        os.environ["UHDR_HIP_API3_ROUTE"] = self.route

    def __exit__(self, *exc):
        os.environ.pop("UHDR_HIP_API3_ROUTE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
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
    dev = "cuda:0"
    fmts = {"420": A.UHDR_IMG_FMT_12bppYCbCr420, "422": A.UHDR_IMG_FMT_16bppYCbCr422, "444": A.UHDR_IMG_FMT_24bppYCbCr444}
    rows = []
    for (W, H) in SIZES:
        wp, hp = (W + 15) // 16 * 16, (H + 15) // 16 * 16
        dh = synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100).to(dev)
        for sampling in SAMPLINGS:
            u0 = UltraHdr(ctx=ctx)
            qts = [u0.quant_table(92, False), u0.quant_table(92, True), u0.quant_table(92, True)]
            # the SDR intent: a synthetic image on the padded grid -> its coefficients on libjpeg's grids for W x H -> its scan
            src = synth.make_sdr_planar(fmts[sampling], wp, hp).to(dev)
            dims = grids(W, H, SAMPLINGS[sampling])
            dco = []
            for c, (bw, bh) in enumerate(dims):
                pl = src.plane_tensor(c)
                dco.append(u0.fdct_quant(pl, pl.shape[1], bw, bh, qts[c]))
            scan = u0.huffman_encode(dco, W, H, SAMPLINGS[sampling], 0).clone()
            hdr_j = UltraHdr.jpeg_header(W, H, SAMPLINGS[sampling], qts)
            ctx.synchronize()
            for (nch, s) in ((3, 1), (1, 4)):
                for preset in (A.UHDR_USAGE_BEST_QUALITY, A.UHDR_USAGE_REALTIME):
                    u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=s, useMultiChannelGainMap=nch == 3, preset=preset)
                    cfg = u.encode_cfg(True, True)
                    mw, mh = W // s, H // s
                    qm = (u.quant_table(85, False), u.quant_table(85, True))
                    qt = lambda t: (C.c_uint16 * 64)(*[int(v) for v in t])
                    q_ml, q_mc, q_sdr = qt(qm[0]), qt(qm[1]), [qt(t) for t in qts]
                    mfmt = A.UHDR_IMG_FMT_24bppRGB888 if nch == 3 else A.UHDR_IMG_FMT_8bppYCbCr400
                    gm_f, gm_s = Image(mfmt, mw, mh, align=64, device=dev), Image(mfmt, mw, mh, align=64, device=dev)
                    planes = Image(fmts[sampling], wp, hp, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=64, device=dev)
                    planes.raw.w, planes.raw.h = W, H
                    md_f, md_s = A.GainmapMetadata(), A.GainmapMetadata()
                    jc = A.JpegCoefficients()
                    for i in range(3):
                        jc.coef[i] = dco[i].data_ptr()
                        jc.blocks_h[i], jc.blocks_w[i] = int(dco[i].shape[0]), int(dco[i].shape[1])
                        for k in range(64):
                            jc.qtable[i][k] = int(qts[i][k])
                    fn_coef = getattr(lib, COEF_ENTRY[sampling])

                    def op_fused():
                        with ordered():
                            check(fn_coef(ctx.handle, C.byref(jc), W, H, A.UHDR_CG_BT_709, C.byref(dh.raw), C.byref(cfg), C.byref(md_f), C.byref(gm_f.raw)))

                    def op_staged(coefs=dco):
                        with ordered():
                            for i in range(3):
                                check(lib.uhdr_hip_idct_dequant_dev(ctx.handle, C.c_void_p(coefs[i].data_ptr()), dims[i][0], dims[i][1], q_sdr[i],
                                                                    C.c_void_p(planes.raw.planes[i]), planes.raw.stride[i]))
                            check(lib.uhdr_hip_generate_gainmap_dev(ctx.handle, C.byref(planes.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm_s.raw)))

                    op_fused()
                    op_staged()
                    ctx.synchronize()
                    identical = md_f.as_dict() == md_s.as_dict() and torch.equal(gm_f.buf, gm_s.buf)
                    row = dict(size=f"{W}x{H}", sampling=sampling, channels=nch, scale=s, preset="two-pass" if preset == A.UHDR_USAGE_BEST_QUALITY else "one-pass")
                    kf, ks = [], []
                    for _ in range(args.rounds):  # alternating, each loop behind its own warm-up
                        kf.append(kernel_ms(ctx, op_fused, args.iters, ("generate_gainmap",)))
                        ks.append(kernel_ms(ctx, op_staged, args.iters, ("idct_dequant", "generate_gainmap")))
                    row["operators"] = verdict(kf, ks)

                    if mw % 8 == 0 and mh % 8 == 0:  # (b) the whole call
                        cap = mw * mh * nch + (1 << 16)
                        out_f, out_r, out_s = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
                        back = [torch.empty_like(t) for t in dco]
                        mapc = [torch.empty((mh // 8, mw // 8, 64), dtype=torch.int16, device=dev) for _ in range(nch)]
                        res = {}

                        def one_call(route, out):
                            with Route(route):
                                res[route] = u.encodeApi3Scans(hdr_j, scan, A.UHDR_CG_BT_709, dh, qm, out)

                        def chain():
                            sc = u._scan(back, W, H, SAMPLINGS[sampling], 0)
                            with ordered():
                                check(lib.uhdr_hip_huffman_decode_dev(ctx.handle, C.byref(sc), None, C.c_void_p(scan.data_ptr()), scan.numel()))
                            op_staged(back)
                            with ordered():
                                if nch == 3:
                                    check(lib.uhdr_hip_fdct_quant_rgb_dev(ctx.handle, C.byref(gm_s.raw), q_ml, q_mc, *[C.c_void_p(m.data_ptr()) for m in mapc]))
                                else:
                                    check(lib.uhdr_hip_fdct_quant_dev(ctx.handle, C.c_void_p(gm_s.raw.planes[0]), gm_s.raw.stride[0], mw // 8, mh // 8, q_ml,
                                                                      C.c_void_p(mapc[0].data_ptr())))
                            res["chain"] = int(u.huffman_encode(mapc, mw, mh, [(1, 1)] * nch, 0, out=out_s).numel())

                        one_call("fused", out_f)
                        one_call("staged", out_r)
                        chain()
                        ctx.synchronize()
                        n = res["chain"]
                        identical = identical and res["fused"][0] == res["staged"][0] == n and torch.equal(out_f[:n], out_s[:n]) and torch.equal(out_r[:n], out_s[:n])
                        identical = identical and res["fused"][1].as_dict() == res["staged"][1].as_dict() == md_s.as_dict()
                        tf, tr, tc = [], [], []
                        it = max(3, args.iters // 2)
                        for _ in range(args.rounds):
                            tf.append(wall_ms(ctx, lambda: one_call("fused", out_f), it))
                            tr.append(wall_ms(ctx, lambda: one_call("staged", out_r), it))
                            tc.append(wall_ms(ctx, chain, it))
                        row["map_scan_bytes"] = n
                        row["calls"] = verdict(tf, tc)
                        v = verdict(tf, tr)
                        row["calls_vs_staged_route"] = dict(staged_route_ms=v["staged_ms"], staged_route_spread_ms=v["staged_spread_ms"], staged_route_over_fused=v["staged_over_fused"],
                                                            meets_bar=v["meets_bar"], staged_route_rounds_ms=v["staged_rounds_ms"])
                        row["meets_bar"] = row["calls"]["meets_bar"]
                    else:
                        row["calls"] = None
                        row["meets_bar"] = None
                    row["identical_outputs"] = bool(identical)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    ctx.close()
    defaults = {}
    for sampling in SAMPLINGS:
        have = [r["meets_bar"] for r in rows if r["sampling"] == sampling and r["meets_bar"] is not None]
        defaults[sampling] = "fused" if have and all(have) else "staged"
    print(json.dumps(dict(default_route=defaults)), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(rows=rows, default_route=defaults), f, indent=1)
    if not all(r["identical_outputs"] for r in rows):
        sys.exit("the routes' outputs differ")


if __name__ == "__main__":
    main()
