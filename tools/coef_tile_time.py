"""Launches the two kernels that take an image as JPEG coefficient blocks (the coefficient-tile stage of csrc/coef_tile.h), for a
kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -o t -- python tools/coef_tile_time.py [--iters 65]

At 3840 x 2160, device resident, `iters` launches each behind two warm-up launches:
  applyGainMapFromCoefficients, linear F16 output, a one-channel map at scale factor 4, for 4:2:0, 4:2:2 and 4:4:4 bases;
  generateGainMapFromCoefficients from a P010 HLG intent, a one-channel map at scale factor 4, for 4:2:0, 4:2:2 and 4:4:4 SDR intents
  and both presets (best quality: two passes; real time: one).
The coefficients are small random values with flat tables (every dequantised value below 2^13: the 24-bit multiply path, as for any
image that came out of an 8-bit forward DCT).  To trace two builds in turn, exchange libultrahdr_amd/lib/libuhdr_hip.so between
runs, each run its own process; tools/read_prof.py summarises the databases."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
SAMPLINGS = {"420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)], "444": [(1, 1)] * 3}


def grids(w, h, sampling):
    hmax, vmax = max(s[0] for s in sampling), max(s[1] for s in sampling)
    return [((-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8) for hs, vs in sampling]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=65)
    args = ap.parse_args()

    import numpy as np
    import torch

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    dev = "cuda:0"
    f16 = A.UHDR_IMG_FMT_64bppRGBAHalfFloat
    gen = torch.Generator(device=dev).manual_seed(7)
    qts = [np.full(64, 16, dtype=np.uint16)] * 3
    coefs = {s: [torch.randint(-24, 25, (bh, bw, 64), dtype=torch.int16, device=dev, generator=gen) for bw, bh in grids(W, H, f)]
             for s, f in SAMPLINGS.items()}
    torch.cuda.synchronize()

    u = UltraHdr(ctx=ctx)
    gm = synth.make_gainmap(W // 4, H // 4, 1, cg=A.UHDR_CG_BT_2100).to(dev)
    md = synth.default_metadata()
    dest = Image(f16, W, H, align=64, device=dev)
    for s in ("420", "422", "444"):
        for _ in range(args.iters + 2):
            if s == "444":
                u.applyGainMapFromCoefficients444(coefs[s], qts, W, H, A.UHDR_CG_BT_709, gm, md, A.UHDR_CT_LINEAR, f16, A.FLT_MAX, dest)
            else:
                u.applyGainMapFromCoefficients(coefs[s], qts, W, H, A.UHDR_CG_BT_709, gm, md, A.UHDR_CT_LINEAR, f16, A.FLT_MAX, dest, sampling=s)
        ctx.synchronize()
        print(f"apply {s}: {args.iters + 2} launches")

    hdr = synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100).to(dev)
    for preset, name in ((A.UHDR_USAGE_BEST_QUALITY, "best"), (A.UHDR_USAGE_REALTIME, "realtime")):
        e = UltraHdr(ctx=ctx, preset=preset)
        for s in ("420", "422", "444"):
            out = None
            for _ in range(args.iters + 2):
                _, out = e.generateGainMapFromCoefficients(coefs[s], qts, W, H, A.UHDR_CG_BT_709, hdr, s, gm=out)
            ctx.synchronize()
            print(f"generate {s} {name}: {args.iters + 2} launches")
    ctx.close()


if __name__ == "__main__":
    main()
