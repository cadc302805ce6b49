"""generateGainMap with a gain-map gamma other than 1, 3840 x 2160 4:2:0 + P010, gamma 1.571: the threshold-table route
(UHDR_HIP_GENERATE_GAMMA_TABLE: uhdr_hip_generate_gainmap_ex_dev, uhdr_hip_encode_api1_scans_ex_dev) against the pow-per-sample route of
the older entry points, which this build leaves as they were.

    python tools/generate_gamma_time.py [--calls 20] [--rounds 5] [--json profiles/generate_gamma_time.json]

    generate   table: uhdr_hip_generate_gainmap_ex_dev with the flag      pow: uhdr_hip_generate_gainmap_dev
               one pass and two pass, one and three channels, scale 1 and 4; the library's own event pairs around its launches
               (uhdr_hip_profile_enable, family generate_gainmap), summed per call
    api1       table: uhdr_hip_encode_api1_scans_ex_dev with the flag     pow: the staged chain the refusal sends a caller to --
               uhdr_hip_generate_gainmap_dev, fdct_quant x 3 of the base image, fdct_quant / fdct_quant_rgb of the map, huffman_encode x 2 --
               both through the Python binding, wall clock from call to synchronize (no base-image colour conversion on either side)

`calls` calls per candidate and round after three warm-up calls, the candidates alternating, `rounds` rounds: the median of the rounds'
medians and their spread (max - min).  `rule_holds`: the table route's median is below the other's by more than the two spreads added --
only such a row is a gain.  Before a generate row is timed the two maps are compared: they may differ by one code.  The host's time to
build the thresholds of a new gamma is recorded first (uhdr_hip_gamma_code_eval, before any call needs them)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA = 1.571
W, H = 3840, 2160


def spread_rule(rows_new, rows_old):
    new, old = float(np.median(rows_new)), float(np.median(rows_old))
    s_new, s_old = float(max(rows_new) - min(rows_new)), float(max(rows_old) - min(rows_old))
    return dict(table_us=new * 1e3, table_spread_us=s_new * 1e3, pow_us=old * 1e3, pow_spread_us=s_old * 1e3, margin_us=(old - new) * 1e3,
                spreads_added_us=(s_new + s_old) * 1e3, rule_holds=bool(old - new > s_new + s_old), table_rounds_us=[x * 1e3 for x in rows_new],
                pow_rounds_us=[x * 1e3 for x in rows_old])


def read_family(ctx, family, capacity=65536):
    buf = (C.c_double * capacity)()
    n = ctx.lib.uhdr_hip_profile_read_list(ctx.handle, family.encode() if family else None, buf, capacity, 1)
    return list(buf[: min(n, capacity)])


def timed_events(ctx, fn, calls):
    """-> the median over `calls` calls of the summed milliseconds of a call's generate_gainmap launches."""
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.lib.uhdr_hip_profile_enable(ctx.handle, 1)
    read_family(ctx, None)
    for _ in range(calls):
        fn()
    ctx.synchronize()
    v = read_family(ctx, "generate_gainmap")
    left = read_family(ctx, None)
    ctx.lib.uhdr_hip_profile_enable(ctx.handle, 0)
    assert v and len(v) % calls == 0 and not left, (len(v), calls, len(left))
    return float(np.median(np.asarray(v).reshape(calls, -1).sum(1)))


def timed_wall(ctx, fn, calls):
    for _ in range(3):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def uhdr_for(ctx, preset, multi, scale):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=ctx, mapDimensionScaleFactor=scale, useMultiChannelGainMap=bool(multi), gamma=GAMMA, preset=preset)


def generate_case(ctx, ds, dh, preset, multi, scale, calls, rounds):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd.images import Image

    u = uhdr_for(ctx, preset, multi, scale)
    cfg = u.encode_cfg()
    fmt = A.UHDR_IMG_FMT_24bppRGB888 if multi else A.UHDR_IMG_FMT_8bppYCbCr400
    g_new, g_old = (Image(fmt, W // scale, H // scale, align=64, device="cuda:0") for _ in range(2))
    md = A.GainmapMetadata()
    lib, h = ctx.lib, ctx.handle
    run_new = lambda: A.check(lib.uhdr_hip_generate_gainmap_ex_dev(h, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md), C.byref(g_new.raw),
                                                                   A.UHDR_HIP_GENERATE_GAMMA_TABLE))
    run_old = lambda: A.check(lib.uhdr_hip_generate_gainmap_dev(h, C.byref(ds.raw), C.byref(dh.raw), C.byref(cfg), C.byref(md), C.byref(g_old.raw)))
    run_new(), run_old()
    ctx.synchronize()
    d = np.abs(g_new.to_host().valid(0).astype(np.int32) - g_old.to_host().valid(0).astype(np.int32))
    rows_new, rows_old = [], []
    for _ in range(rounds):  # alternating
        rows_new.append(timed_events(ctx, run_new, calls))
        rows_old.append(timed_events(ctx, run_old, calls))
    out = dict(what="generate_gainmap", preset="one pass" if preset == A.UHDR_USAGE_REALTIME else "two pass", channels=3 if multi else 1, scale=scale,
               maps_max_code_diff=int(d.max()), maps_fraction_differing=float((d != 0).mean()))
    out.update(spread_rule(rows_new, rows_old))
    return out


def api1_case(ctx, ds, dh, preset, multi, scale, calls, rounds):
    import torch

    from libultrahdr_amd import capi as A
    from oracle import loader as L

    u = uhdr_for(ctx, preset, multi, scale)
    qb, qm = (L.quant_table_port(95, False), L.quant_table_port(95, True)), (L.quant_table_port(90, False), L.quant_table_port(90, True))
    n = W * H * 3 + 4096
    ob, om = torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0")
    enc = A.UHDR_CG_UNSPECIFIED
    run_new = lambda: u.encodeApi1ScansEx(ds, dh, enc, qb, qm, ob, om, A.UHDR_HIP_GENERATE_GAMMA_TABLE)

    def run_old():
        md, gm = u.generateGainMap(ds, dh)
        base = [u.fdct_quant(ds.plane_tensor(i), ds.raw.stride[i], W // (16 if i else 8), H // (16 if i else 8), qb[1 if i else 0]) for i in range(3)]
        mapc = list(u.fdct_quant_rgb(gm, qm[0], qm[1])) if multi else [u.fdct_quant(gm.plane_tensor(0), gm.raw.stride[0], gm.w // 8, gm.h // 8, qm[0])]
        u.huffman_encode(base, W, H, [(2, 2), (1, 1), (1, 1)], 0)
        u.huffman_encode(mapc, gm.w, gm.h, [(1, 1)] * len(mapc), 0)

    rows_new, rows_old = [], []
    for _ in range(rounds):
        rows_new.append(timed_wall(ctx, run_new, calls))
        rows_old.append(timed_wall(ctx, run_old, calls))
    out = dict(what="encode_api1_scans", preset="one pass" if preset == A.UHDR_USAGE_REALTIME else "two pass", channels=3 if multi else 1, scale=scale)
    out.update(spread_rule(rows_new, rows_old))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.ultrahdr import Context

    info = (C.c_uint32 * 4)()
    rc = A.load().uhdr_hip_gamma_code_eval(C.c_float(GAMMA), 1, None, None, 0, info, None)
    result = {"gamma": GAMMA, "frame": f"{W}x{H} 4:2:0 + P010", "tables_verified_exact": bool(rc == 0 and info[0] == 1), "tables_build_us": int(info[2]),
              "two_pass_smallest_threshold_gap_ulps": int(info[3]), "cases": []}
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}), flush=True)
    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    ds, dh = synth.make_sdr_yuv420(W, H).to("cuda:0"), synth.make_hdr_p010(W, H, ct=A.UHDR_CT_HLG).to("cuda:0")
    RT, BQ = A.UHDR_USAGE_REALTIME, A.UHDR_USAGE_BEST_QUALITY
    for preset in (RT, BQ):
        for multi in (0, 1):
            for scale in (1, 4):
                r = generate_case(ctx, ds, dh, preset, multi, scale, args.calls, args.rounds)
                result["cases"].append(r)
                print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds_us")}), flush=True)
    for preset, multi, scale in ((BQ, 1, 1), (RT, 1, 1), (RT, 0, 1)):  # (a scale-4 map of this frame is 960 x 540: not whole blocks, the chain declines it)
        r = api1_case(ctx, ds, dh, preset, multi, scale, max(5, args.calls // 2), args.rounds)
        result["cases"].append(r)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds_us")}), flush=True)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
