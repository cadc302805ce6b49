"""The fused API-0 front end for P010 intents against the staged route, at 3840 x 2160, HLG / BT.2100 P010, one pass, three channels:

    device call   uhdr_hip_encode_api0_p010_fused_dev                         (one kernel: 3 B/px in, 1.5 + 3 out)
            vs    uhdr_hip_tone_map_dev + uhdr_hip_generate_gainmap_dev       (two kernels: 12 B/px in all)
                  on the same device-resident intent, into preallocated device images, arguments marshalled once
    one call      uhdr_hip_encode_api0_scans_any on the host intent           (upload, fused kernel, FDCTs, both scans coded, bytes down)
            vs    the same chain through the existing entry points: upload of the intent, tone map, gain map, three
                  uhdr_hip_fdct_quant_dev + uhdr_hip_fdct_quant_rgb_dev, uhdr_hip_huffman_encode2_dev, download of the bytes

    python tools/api0_p010_time.py [--iters 50] [--rounds 5] [--json out.json]

Device calls: HIP events on the context's stream around a loop of calls, each loop behind its own warm-up of the same calls, and
next to that the library's own per-launch event times (uhdr_hip_profile_*: the kernels without the gaps between their launches),
taken in loops of their own.  One-call routes: a host clock around calls that end synchronised (the bytes are on the host).  The
two routes of a pair alternate, `rounds` times; the median round is reported next to every round.  Outputs of the two routes are
compared at the timed size before anything is timed.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160


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


def kernel_ms(ctx, fn, iters, families):
    """Per-call milliseconds inside the launches of `families` (the library's events around each launch)."""
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.profile(True)
    for f in families:
        ctx.profile_read(f)
    for _ in range(iters):
        fn()
    ctx.synchronize()
    total = sum(ctx.profile_read(f)[1] for f in families)
    ctx.profile(False)
    return total / iters


def wall_ms(ctx, fn, iters):
    for _ in range(2):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


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
    u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=1, useMultiChannelGainMap=True, preset=A.UHDR_USAGE_REALTIME)
    lib, check, ordered = ctx.lib, A.check, ctx.ordered
    hdr = synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG, cg=A.UHDR_CG_BT_2100)
    dh = hdr.to("cuda:0")
    cfg = u.encode_cfg(False, False)
    f420, frgb = A.UHDR_IMG_FMT_12bppYCbCr420, A.UHDR_IMG_FMT_24bppRGB888
    base_f, gm_f = Image(f420, W, H, align=64, device="cuda:0"), Image(frgb, W, H, align=64, device="cuda:0")
    base_s, gm_s = Image(f420, W, H, align=64, device="cuda:0"), Image(frgb, W, H, align=64, device="cuda:0")
    md_f, md_s = A.GainmapMetadata(), A.GainmapMetadata()
    a_fused = (ctx.handle, C.byref(dh.raw), C.byref(cfg), C.byref(base_f.raw), C.byref(md_f), C.byref(gm_f.raw))
    a_tone = (ctx.handle, C.byref(dh.raw), C.byref(base_s.raw))
    a_gen = (ctx.handle, C.byref(base_s.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm_s.raw))

    def fused():
        with ordered():
            check(lib.uhdr_hip_encode_api0_p010_fused_dev(*a_fused))

    def staged():
        with ordered():
            check(lib.uhdr_hip_tone_map_dev(*a_tone))
            check(lib.uhdr_hip_generate_gainmap_dev(*a_gen))

    fused()
    staged()
    ctx.synchronize()
    identical = bool((base_f.buf == base_s.buf).all().item()) and bool((gm_f.buf == gm_s.buf).all().item()) and md_f.as_dict() == md_s.as_dict()
    tf, ts, kf, ks = [], [], [], []
    for _ in range(args.rounds):  # alternating, each loop behind its own warm-up
        tf.append(event_ms(ctx, fused, args.iters))
        ts.append(event_ms(ctx, staged, args.iters))
    for _ in range(args.rounds):
        kf.append(kernel_ms(ctx, fused, args.iters, ("encode_api0_fused",)))
        ks.append(kernel_ms(ctx, staged, args.iters, ("tone_map", "generate_gainmap")))
    med = lambda v: float(np.median(v))
    px = W * H
    row_dev = dict(what="device call", size=f"{W}x{H}", intent="P010 HLG BT.2100 limited range", map="3 channels, one pass", identical_outputs=identical,
                   fused_call_ms=med(tf), staged_call_ms=med(ts), staged_over_fused_call=med(ts) / med(tf), fused_call_rounds_ms=tf, staged_call_rounds_ms=ts,
                   fused_kernel_ms=med(kf), staged_kernels_ms=med(ks), staged_over_fused_kernels=med(ks) / med(kf), fused_kernel_rounds_ms=kf,
                   staged_kernels_rounds_ms=ks, fused_algorithmic_GBps=7.5 * px / med(kf) / 1e6, staged_algorithmic_GBps=12.0 * px / med(ks) / 1e6)
    print(json.dumps(row_dev), flush=True)

    # ---- host intent -> the two scans on the host ----
    qb = (u.quant_table(95, False), u.quant_table(95, True))
    qm = (u.quant_table(85, False), u.quant_table(85, True))
    cap = W * H * 3 + (1 << 16)
    one = {}

    def one_call():
        one["r"] = u.encodeApi0ScansAny(hdr, qb, qm, cap, cap)

    up = Image(A.UHDR_IMG_FMT_24bppYCbCrP010, W, H, hdr.raw.cg, hdr.raw.ct, hdr.raw.range, align=64, device="cuda:0")
    src = torch.from_numpy(hdr.buf)
    coef_b = [torch.empty((H // 8, W // 8, 64), dtype=torch.int16, device="cuda:0")] + [torch.empty((H // 16, W // 16, 64), dtype=torch.int16, device="cuda:0") for _ in range(2)]
    outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    a_tone2 = (ctx.handle, C.byref(up.raw), C.byref(base_s.raw))
    a_gen2 = (ctx.handle, C.byref(base_s.raw), C.byref(up.raw), C.byref(cfg), C.byref(md_s), C.byref(gm_s.raw))
    chain = {}

    def staged_chain():
        up.buf.copy_(src)  # the intent goes up once here too (pageable memory, as the entry point's caller has it)
        with ordered():
            check(lib.uhdr_hip_tone_map_dev(*a_tone2))
            check(lib.uhdr_hip_generate_gainmap_dev(*a_gen2))
        for i in range(3):
            pl = base_s.plane_tensor(i)
            u.fdct_quant(pl, pl.shape[1], (W if i == 0 else W // 2) // 8, (H if i == 0 else H // 2) // 8, qb[0 if i == 0 else 1], coef=coef_b[i])
        coef_m = u.fdct_quant_rgb(gm_s, qm[0], qm[1])
        sb, sm = u.huffman_encode2(coef_b, W, H, [(2, 2), (1, 1), (1, 1)], coef_m, W, H, [(1, 1)] * 3, outs=outs)
        chain["r"] = (sb.cpu().numpy().tobytes(), sm.cpu().numpy().tobytes())

    one_call()
    staged_chain()
    same = one["r"][0] == chain["r"][0] and one["r"][1] == chain["r"][1]
    it = max(3, args.iters // 5)
    to, tc = [], []
    for _ in range(args.rounds):
        to.append(wall_ms(ctx, one_call, it))
        tc.append(wall_ms(ctx, staged_chain, it))
    row_one = dict(what="host intent -> two scans on the host", size=f"{W}x{H}", identical_scans=same, base_scan_bytes=len(one["r"][0]),
                   map_scan_bytes=len(one["r"][1]), one_call_ms=med(to), staged_chain_ms=med(tc), staged_over_one_call=med(tc) / med(to),
                   one_call_rounds_ms=to, staged_chain_rounds_ms=tc)
    print(json.dumps(row_one), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump([row_dev, row_one], f, indent=1)


if __name__ == "__main__":
    main()
