"""The fused API-1 encode for RGBA8888 SDR intents against the staged route, RGBA1010102 PQ BT.2100 + RGBA8888 BT.709, two passes,
three channels, everything device resident: scale factor 1 at 3840 x 2160 and scale factor 4 at 3840 x 2176 (2160 / 4 = 540 map rows
are not whole 8 x 8 blocks, which the fused chain leaves to the operators; see SCALES):

    (a) base stage   base_blocks_rgba_kernel inside uhdr_hip_encode_api1_fused_any_dev     (one launch: 4 B/px in, 6 out)
               vs    uhdr_hip_convert_raw_input_to_ycbcr_dev + uhdr_hip_convert_yuv_dev + 3 x uhdr_hip_fdct_quant_dev   (22 B/px)
                     both inside the launches: the library's own events around each launch (uhdr_hip_profile_*)
    (b) device call  uhdr_hip_encode_api1_fused_any_dev
               vs    uhdr_hip_generate_gainmap_dev + the three staged base stages + uhdr_hip_fdct_quant_rgb_dev, on the same images
    (c) one call     uhdr_hip_encode_api1_scans_any_dev, wall time
               vs    the staged stages + uhdr_hip_huffman_encode2_dev

    python tools/api1_rgba_time.py [--iters 50] [--rounds 5] [--json out.json]

(a): the fused chain records its RGBA base launch under a profile family of its own, "base_blocks_rgba" (one entry per call, asserted),
apart from the map's blocks ("fdct_quant"); it runs on the auxiliary stream under the gain-map passes, as it does in use.  (b): HIP events on the context's stream around a loop of
calls.  (c): a host clock around calls that end synchronised.  Every loop runs behind its own warm-up of the same calls; the two
routes of a pair alternate, `rounds` times; the median round is reported next to every round, and `spread` is the larger of the
two routes' max - min over the rounds.  The acceptance flags say whether the fused median is at most the staged median plus that
spread.  Outputs of the two routes are compared at the timed size before anything is timed.
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
# scale factor -> height: 2160 / 4 = 540 map rows are not whole 8 x 8 blocks, which the fused chain (4:2:0 and RGBA alike) leaves to the
# operators; scale factor 4 is timed at the nearest height whose map is (2176 / 4 = 544)
SCALES = [(1, H), (4, 2176)]


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


def launches_ms(ctx, fn, iters, families):
    """family -> the durations (ms) of its launches over `iters` calls, in launch order, behind a warm-up."""
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_read(None)
    for _ in range(iters):
        fn()
    ctx.synchronize()
    out = {f: ctx.profile_read_list(f) for f in families}
    ctx.profile_read(None)
    ctx.profile(False)
    return out


def wall_ms(ctx, fn, iters):
    for _ in range(2):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def med(v):
    return float(np.median(v))


def spread(a, b):
    return float(max(max(a) - min(a), max(b) - min(b)))


def run_scale(ctx, scale, sdr, hdr, args):
    W, H = sdr.w, sdr.h
    import torch

    from libultrahdr_amd import capi as A
    from libultrahdr_amd.images import Image
    from libultrahdr_amd.ultrahdr import UltraHdr

    dev = "cuda:0"
    u = UltraHdr(ctx=ctx, mapDimensionScaleFactor=scale, useMultiChannelGainMap=True, preset=A.UHDR_USAGE_BEST_QUALITY)
    lib, check, ordered = ctx.lib, A.check, ctx.ordered
    ds, dh = sdr.to(dev), hdr.to(dev)
    mw, mh = W // scale, H // scale
    cfg = u.encode_cfg()
    enc = A.UHDR_CG_DISPLAY_P3
    qb = (u.quant_table(95, False), u.quant_table(95, True))
    qm = (u.quant_table(85, False), u.quant_table(85, True))
    qbb, qmm = u._qt_pair(qb), u._qt_pair(qm)
    qt = lambda t: (C.c_uint16 * 64)(*[int(v) for v in t])
    q_bl, q_bc, q_ml, q_mc = qt(qb[0]), qt(qb[1]), qt(qm[0]), qt(qm[1])
    coefs = lambda bh, bw, n: [torch.empty((bh, bw, 64), dtype=torch.int16, device=dev) for _ in range(n)]
    base_f, map_f = coefs(H // 8, W // 8, 3), coefs(mh // 8, mw // 8, 3)
    base_s, map_s = coefs(H // 8, W // 8, 3), coefs(mh // 8, mw // 8, 3)
    blocks = A.Api1Blocks()
    for i in range(3):
        blocks.base_coef[i], blocks.map_coef[i] = base_f[i].data_ptr(), map_f[i].data_ptr()
    md_f, md_s = A.GainmapMetadata(), A.GainmapMetadata()
    ycc = Image(A.UHDR_IMG_FMT_24bppYCbCr444, W, H, align=64, device=dev)
    gm = Image(A.UHDR_IMG_FMT_24bppRGB888, mw, mh, align=64, device=dev)
    a_fused = (ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), enc, C.c_void_p(qbb.ctypes.data), C.c_void_p(qmm.ctypes.data),
               C.byref(blocks), C.byref(md_f), None)
    a_gen = (ctx.handle, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md_s), C.byref(gm.raw))

    def fused():
        with ordered():
            check(lib.uhdr_hip_encode_api1_fused_any_dev(*a_fused))

    def staged_base():
        with ordered():
            check(lib.uhdr_hip_convert_raw_input_to_ycbcr_dev(ctx.handle, C.byref(ds.raw), 0, C.byref(ycc.raw)))
            check(lib.uhdr_hip_convert_yuv_dev(ctx.handle, C.byref(ycc.raw), sdr.raw.cg, enc))
            for i in range(3):
                check(lib.uhdr_hip_fdct_quant_dev(ctx.handle, C.c_void_p(ycc.raw.planes[i]), ycc.raw.stride[i], W // 8, H // 8, q_bc if i else q_bl,
                                                  C.c_void_p(base_s[i].data_ptr())))

    def staged():
        with ordered():
            check(lib.uhdr_hip_generate_gainmap_dev(*a_gen))
        staged_base()
        with ordered():
            check(lib.uhdr_hip_fdct_quant_rgb_dev(ctx.handle, C.byref(gm.raw), q_ml, q_mc, *[C.c_void_p(m.data_ptr()) for m in map_s]))

    fused()
    staged()
    ctx.synchronize()
    identical = all(torch.equal(a, b) for a, b in zip(base_f + map_f, base_s + map_s)) and md_f.as_dict() == md_s.as_dict()

    # (a) inside the launches
    fam_staged = ("convert_raw_input_to_ycbcr", "convert_yuv", "fdct_quant")
    kf, ks, per_stage = [], [], {f: [] for f in fam_staged}
    for _ in range(args.rounds):
        each = launches_ms(ctx, fused, args.iters, ("base_blocks_rgba", "fdct_quant"))
        assert len(each["base_blocks_rgba"]) == args.iters and len(each["fdct_quant"]) == args.iters, {k: len(v) for k, v in each.items()}
        kf.append(sum(each["base_blocks_rgba"]) / args.iters)
        st = launches_ms(ctx, staged_base, args.iters, fam_staged)
        assert len(st["fdct_quant"]) == 3 * args.iters and len(st["convert_yuv"]) == args.iters, {k: len(v) for k, v in st.items()}
        for f in fam_staged:
            per_stage[f].append(sum(st[f]) / args.iters)
        ks.append(sum(sum(st[f]) for f in fam_staged) / args.iters)
    px = W * H
    row_a = dict(what="(a) base stage inside the launches", scale=scale, size=f"{W}x{H}", identical_outputs=identical, fused_base_launch_ms=med(kf), staged_three_stages_ms=med(ks),
                 staged_over_fused=med(ks) / med(kf), spread_ms=spread(kf, ks), fused_not_slower=med(kf) <= med(ks) + spread(kf, ks),
                 fused_rounds_ms=kf, staged_rounds_ms=ks, staged_per_stage_ms={f: med(v) for f, v in per_stage.items()},
                 fused_algorithmic_GBps=10.0 * px / med(kf) / 1e6, staged_algorithmic_GBps=22.0 * px / med(ks) / 1e6)
    print(json.dumps(row_a), flush=True)

    # (b) the device call
    tf, ts = [], []
    for _ in range(args.rounds):
        tf.append(event_ms(ctx, fused, args.iters))
        ts.append(event_ms(ctx, staged, args.iters))
    row_b = dict(what="(b) device call", scale=scale, size=f"{W}x{H}", fused_call_ms=med(tf), staged_chain_ms=med(ts), staged_over_fused=med(ts) / med(tf), spread_ms=spread(tf, ts),
                 fused_not_slower=med(tf) <= med(ts) + spread(tf, ts), fused_rounds_ms=tf, staged_rounds_ms=ts)
    print(json.dumps(row_b), flush=True)

    # (c) to the two scans, device buffers
    cap = W * H * 3 + (1 << 16)
    ob, om = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    one, chain = {}, {}

    def one_call():
        one["r"] = u.encodeApi1ScansAny(ds, dh, enc, qb, qm, ob, om)

    def staged_scans():
        staged()
        sb, sm = u.huffman_encode2(base_s, W, H, [(1, 1)] * 3, map_s, mw, mh, [(1, 1)] * 3, outs=outs)
        chain["r"] = (int(sb.numel()), int(sm.numel()))

    one_call()
    staged_scans()
    ctx.synchronize()
    nb, nm = one["r"][0], one["r"][1]
    same = (nb, nm) == chain["r"] and torch.equal(ob[:nb], outs[0][:nb]) and torch.equal(om[:nm], outs[1][:nm])
    it = max(3, args.iters // 5)
    to, tc = [], []
    for _ in range(args.rounds):
        to.append(wall_ms(ctx, one_call, it))
        tc.append(wall_ms(ctx, staged_scans, it))
    row_c = dict(what="(c) device intents -> two scans in device buffers, wall", scale=scale, size=f"{W}x{H}", identical_scans=same, base_scan_bytes=nb, map_scan_bytes=nm,
                 one_call_ms=med(to), staged_chain_ms=med(tc), staged_over_one_call=med(tc) / med(to), spread_ms=spread(to, tc), one_call_rounds_ms=to,
                 staged_chain_rounds_ms=tc)
    print(json.dumps(row_c), flush=True)
    return [row_a, row_b, row_c]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.ultrahdr import Context

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    rows = []
    for scale, h in SCALES:
        sdr = synth.make_sdr_rgba8888(W, h, cg=A.UHDR_CG_BT_709)
        hdr = synth.make_hdr_rgba1010102(W, h, ct=A.UHDR_CT_PQ, cg=A.UHDR_CG_BT_2100)
        rows += run_scale(ctx, scale, sdr, hdr, args)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(sizes=[f"{W}x{h} at scale factor {s}" for s, h in SCALES], intents="RGBA1010102 PQ BT.2100 + RGBA8888 BT.709", map="3 channels, two passes", iters=args.iters,
                           rounds=args.rounds, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
