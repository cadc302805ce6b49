"""The fused API-1 encode for RGBA8888 SDR intents off the block grid (UHDR_HIP_ENCODE_RGBA_EDGES on uhdr_hip_encode_api1_scans_edges /
_edges_dev) against the staged public chain the refusal without the flag sends a caller to, RGBA8888 BT.709 + an RGBA1010102 PQ or a half-float
linear BT.2100 HDR intent: 1920 x 1080 at scale factors 1, 2 and 4 (maps 1920 x 1080, 960 x 540, 480 x 270) with both HDR formats,
1170 x 2532 at 1 and 4000 x 3000 at 4 (map 1000 x 750) with RGBA1010102; both presets; three channels at scale factor 1 (the C API's
defaults), one channel above it (the legacy JpegR() defaults):

    python tools/api1_rgba_edges_time.py [--iters 10] [--rounds 5] [--json profiles/api1_rgba_edges_time.json]
    python tools/api1_rgba_edges_time.py --staged-only --lib <libuhdr_hip.so of another commit> --merge-into profiles/api1_rgba_edges_time.json

Per row, a host clock around calls that end synchronised, on the same intents:
  staged   host planes through the per-stage operators: uhdr_hip_convert_raw_input_to_ycbcr (a fresh zero-filled YCbCr 4:4:4 image),
           uhdr_hip_convert_yuv, uhdr_hip_jpeg_encode_image on its planes (the base scan), uhdr_hip_generate_gainmap,
           uhdr_hip_jpeg_encode_image on the map
  host     uhdr_hip_encode_api1_scans_edges with the flag on the same host intents, into host buffers
  dev      uhdr_hip_encode_api1_scans_edges_dev with the flag on device-resident copies of the intents, into preallocated device buffers
(`host` against `staged` compares equal interfaces.  `dev` against `staged` does not: the dev call starts and ends in HBM while the staged
chain carries host planes between its stages, so most of that factor is PCIe and host work.)
The routes alternate, `rounds` times in one process, each loop behind its own warm-up; the median round is reported next to every round
and the spread (largest - smallest round).  The bar: the new call's median lies below the staged median by more than the two spreads
added ("meets_bar"); "loses" says the opposite with the same margin.  The scans and the metadata of the routes are compared for equality at
the timed size before anything is timed (the staged map goes through a zero-filled device image for that comparison, as
tests/test_gpu_api1_rgba_edges.py has it).
--staged-only times the staged chain alone -- it needs nothing of this feature, so with --lib it runs on the library of the parent commit --
and --merge-into adds its medians to the rows of an existing result file as "staged_parent".
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from api0_p010_time import wall_ms  # noqa: E402  (the same clock)
from api0_scaled_time import verdict  # noqa: E402  (medians, spreads, the bar)

# (w, h, scale factor, HDR kind)
ROWS = [(1920, 1080, s, k) for s in (1, 2, 4) for k in ("rgba1010102", "half float")] + [(1170, 2532, 1, "rgba1010102"), (4000, 3000, 4, "rgba1010102")]
SAMP444 = [(1, 1)] * 3
EDGES = 0x4  # UHDR_HIP_ENCODE_RGBA_EDGES (spelled out: --staged-only also runs against a library and mirror without it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--staged-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libuhdr_hip.so to load (with --staged-only: the parent commit's)")
    ap.add_argument("--merge-into", default=None, help="with --staged-only: add the medians to this result file's rows as staged_parent")
    args = ap.parse_args()

    import torch

    from libultrahdr_amd import capi as A

    if args.lib:
        A.LIB_PATH = os.path.abspath(args.lib)
    from libultrahdr_amd import synth
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    dev, enc = "cuda:0", A.UHDR_CG_DISPLAY_P3
    cdiv = lambda a, b: -(-a // b)
    rows = []
    for w, h, s, kind in ROWS:
        sdr = synth.make_sdr_rgba8888(w, h, align=1)
        if kind == "half float":
            hdr = synth.make_hdr_rgba_f16(w, h, specials=False, align=1)
        else:
            hdr = synth.make_hdr_rgba1010102(w, h, ct=A.UHDR_CT_PQ, align=1)
        ds, dh = sdr.to(dev), hdr.to(dev)
        nch = 3 if s == 1 else 1
        for preset, pname in ((A.UHDR_USAGE_BEST_QUALITY, "best quality"), (A.UHDR_USAGE_REALTIME, "real time")):
            u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=s, useMultiChannelGainMap=nch == 3, preset=preset)
            qb = (u.quant_table(95, False), u.quant_table(95, True))
            qm = (u.quant_table(85, False), u.quant_table(85, True))
            mw, mh = w // s, h // s
            cap_b = 3 * cdiv(w, 8) * cdiv(h, 8) * 64 + (1 << 16)  # one byte per coefficient of the blocks there are
            cap_m = cdiv(mw, 8) * cdiv(mh, 8) * 64 * nch + (1 << 16)
            got = {}

            def map_scan(gm):
                if nch == 3:
                    return u.jpeg_encode_image(gm.plane(0).reshape(gm.h, gm.raw.stride[0], 3), gm.w, gm.h, [(1, 1)] * 3, qm[0], qm[1], rgb_channels=3)
                return u.jpeg_encode_image([gm.plane(0)], gm.w, gm.h, [(1, 1)], qm[0], qm[1])

            def base_scan():
                ycc = u.convert_raw_input_to_ycbcr(sdr, False)
                u.convertYuv(ycc, sdr.raw.cg, enc)
                return u.jpeg_encode_image([ycc.plane(i) for i in range(3)], w, h, SAMP444, qb[0], qb[1])

            def staged():
                base = base_scan()
                md, gm = u.generateGainMap(sdr, hdr)
                got["staged"] = (base, map_scan(gm), md)

            row = dict(size=f"{w}x{h}", scale=s, channels=nch, hdr=kind, preset=pname, map=f"{mw}x{mh}")
            if args.staged_only:
                ts = [wall_ms(ctx, staged, args.iters) for _ in range(args.rounds)]
                row.update(staged_ms=statistics.median(ts), staged_spread_ms=max(ts) - min(ts), staged_rounds_ms=ts)
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue

            ob, om = torch.empty(cap_b, dtype=torch.uint8, device=dev), torch.empty(cap_m, dtype=torch.uint8, device=dev)

            def host():
                got["host"] = u.encodeApi1ScansEdges(sdr, hdr, enc, qb, qm, cap_b, cap_m, EDGES)

            def on_dev():
                got["dev"] = u.encodeApi1ScansEdges(ds, dh, enc, qb, qm, ob, om, EDGES)

            # equality first: the staged map through a zero-filled device image
            md_s, gm_s = u.generateGainMap(ds, dh)
            ctx.synchronize()
            want_b, want_m = base_scan(), map_scan(gm_s.to_host())
            host()
            on_dev()
            ctx.synchronize()
            nb, nm, md_d = got["dev"]
            identical = got["host"][0] == want_b and got["host"][1] == want_m and got["host"][2].as_dict() == md_s.as_dict()
            identical = identical and ob[:nb].cpu().numpy().tobytes() == want_b and om[:nm].cpu().numpy().tobytes() == want_m
            identical = identical and md_d.as_dict() == md_s.as_dict()

            ts, th, td = [], [], []
            for _ in range(args.rounds):  # alternating, each loop behind its own warm-up
                ts.append(wall_ms(ctx, staged, args.iters))
                th.append(wall_ms(ctx, host, args.iters))
                td.append(wall_ms(ctx, on_dev, args.iters))
            row.update(identical_outputs=bool(identical), base_scan_bytes=len(want_b), map_scan_bytes=len(want_m), host=verdict(th, ts), dev=verdict(td, ts))
            for k in ("host", "dev"):
                v = row[k]
                v["loses"] = bool(v["fused_ms"] - v["staged_ms"] > v["fused_spread_ms"] + v["staged_spread_ms"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    if args.staged_only and args.merge_into:
        with open(args.merge_into) as f:
            target = json.load(f)
        key = lambda r: (r["size"], r["scale"], r["hdr"], r["preset"])
        parent = {key(r): r for r in rows}
        for r in target:
            p = parent[key(r)]
            r["staged_parent"] = dict(staged_ms=p["staged_ms"], staged_spread_ms=p["staged_spread_ms"], staged_rounds_ms=p["staged_rounds_ms"])
        with open(args.merge_into, "w") as f:
            json.dump(target, f, indent=1)
    elif args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not args.staged_only and not all(r["identical_outputs"] for r in rows):
        sys.exit("the routes' outputs differ")


if __name__ == "__main__":
    main()
