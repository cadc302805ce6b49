"""The fused API-1 encode for frames that are not whole MCUs (uhdr_hip_encode_api1_scans_edges / _edges_dev) against the staged public chain
the whole-MCU entry points' refusal sends a caller to today, at 1920 x 1080 and 1080 x 1920 (h or w % 16 == 8; the scale-4 map is 480 x 270 /
270 x 480, not whole blocks), P010 HLG BT.2100 + YCbCr 4:2:0 BT.709, both presets, three channels at scale factor 1 (the C API's defaults)
and one channel at scale factor 4 (the legacy JpegR() defaults):

    python tools/api1_edges_time.py [--iters 10] [--rounds 5] [--json profiles/api1_edges_time.json]

Per row, a host clock around calls that end synchronised, on the same intents:
  staged   host planes through the per-stage operators: a copy of the SDR intent (convertYuv works in place), uhdr_hip_convert_yuv,
           uhdr_hip_jpeg_encode_image on its planes (the base scan), uhdr_hip_generate_gainmap, uhdr_hip_jpeg_encode_image on the map
  host     uhdr_hip_encode_api1_scans_edges on the same host intents, into host buffers
  dev      uhdr_hip_encode_api1_scans_edges_dev on device-resident copies of the intents, into preallocated device buffers
(`host` against `staged` compares equal interfaces.  `dev` against `staged` does not: the dev call starts and ends in HBM while the staged chain
carries host planes between its stages -- uhdr_hip_jpeg_encode_image takes host planes only --, so most of that factor is PCIe and host work.)
The routes alternate, `rounds` times in one process, each loop behind its own warm-up; the median round is reported next to every round
and the spread (largest - smallest round).  The bar is the same for both pairs: the new call's median lies below the staged median by more
than the two spreads added ("meets_bar"); "loses" says the opposite with the same margin.  The scans and the metadata of the routes are
compared for equality at the timed size before anything is timed (the staged map goes through a zero-filled device image for that
comparison, as tests/test_gpu_api1_edges.py has it).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from api0_p010_time import wall_ms  # noqa: E402  (the same clock)
from api0_scaled_time import verdict  # noqa: E402  (medians, spreads, the bar)

SIZES = [(1920, 1080), (1080, 1920)]
CONFIGS = [(1, 3), (4, 1)]  # (scale factor, channels)
SAMP420 = [(2, 2), (1, 1), (1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    dev, enc = "cuda:0", A.UHDR_CG_DISPLAY_P3
    rows = []
    for w, h in SIZES:
        sdr = synth.make_sdr_yuv420(w, h)
        hdr = synth.make_hdr_p010(w, h, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100)
        ds, dh = sdr.to(dev), hdr.to(dev)
        for s, nch in CONFIGS:
            for preset, pname in ((A.UHDR_USAGE_BEST_QUALITY, "best quality"), (A.UHDR_USAGE_REALTIME, "real time")):
                u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=s, useMultiChannelGainMap=nch == 3, preset=preset)
                qb = (u.quant_table(95, False), u.quant_table(95, True))
                qm = (u.quant_table(85, False), u.quant_table(85, True))
                mw, mh = w // s, h // s
                cdiv = lambda a, b: -(-a // b)
                cap_b = (cdiv(w, 8) * cdiv(h, 8) + 2 * cdiv(w, 16) * cdiv(h, 16)) * 64 + (1 << 16)  # one byte per coefficient of the blocks there are
                cap_m = cdiv(mw, 8) * cdiv(mh, 8) * 64 * nch + (1 << 16)
                ob, om = torch.empty(cap_b, dtype=torch.uint8, device=dev), torch.empty(cap_m, dtype=torch.uint8, device=dev)
                got = {}

                def map_scan(gm):
                    if nch == 3:
                        return u.jpeg_encode_image(gm.plane(0).reshape(gm.h, gm.raw.stride[0], 3), gm.w, gm.h, [(1, 1)] * 3, qm[0], qm[1], rgb_channels=3)
                    return u.jpeg_encode_image([gm.plane(0)], gm.w, gm.h, [(1, 1)], qm[0], qm[1])

                def base_scan():
                    conv = sdr.clone()
                    u.convertYuv(conv, sdr.raw.cg, enc)
                    return u.jpeg_encode_image([conv.plane(i) for i in range(3)], w, h, SAMP420, qb[0], qb[1])

                def staged():
                    base = base_scan()
                    md, gm = u.generateGainMap(sdr, hdr)
                    got["staged"] = (base, map_scan(gm), md)

                def host():
                    got["host"] = u.encodeApi1ScansEdges(sdr, hdr, enc, qb, qm, cap_b, cap_m, 0)

                def on_dev():
                    got["dev"] = u.encodeApi1ScansEdges(ds, dh, enc, qb, qm, ob, om, 0)

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
                row = dict(size=f"{w}x{h}", scale=s, channels=nch, preset=pname, map=f"{mw}x{mh}", identical_outputs=bool(identical),
                           base_scan_bytes=len(want_b), map_scan_bytes=len(want_m), host=verdict(th, ts), dev=verdict(td, ts))
                for k in ("host", "dev"):
                    v = row[k]
                    v["loses"] = bool(v["fused_ms"] - v["staged_ms"] > v["fused_spread_ms"] + v["staged_spread_ms"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["identical_outputs"] for r in rows):
        sys.exit("the routes' outputs differ")


if __name__ == "__main__":
    main()
