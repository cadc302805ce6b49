"""applyGainMap for a gain map of another aspect ratio than the base image (uhdr_hip_apply_gainmap_any_dev), 3840 x 2160 4:2:0 base:
the two routes against each other, and the old entry point on a same-aspect map of equal size for orientation.

    staged   uhdr_hip_resize_image_dev into scratch of the context, then the usual launch at scale 1 (UHDR_HIP_APPLY_RESIZE=staged);
             also its two launches on their own: the resize alone, and the old entry point on an already resized map
    fused    the resized byte computed per output pixel inside the applyGainMap kernel (UHDR_HIP_APPLY_RESIZE=fused)
    same     uhdr_hip_apply_gainmap_dev on a 16:9 map of the same width (what a file without the mismatch costs)

    python tools/resized_map_time.py [--iters 50] [--rounds 5] [--json profiles/resized_map_time.json] [--no-facade]

Maps: 960 x 720 Y400 and 1920 x 1440 RGBA8888 (4:3 under 16:9); outputs linear RGBA half float and PQ RGBA1010102.  Times are HIP
events on the context's stream around a loop of calls, each loop behind its own warm-up of the same calls; the candidates alternate,
`rounds` times; the median round is reported with the spread (max - min over the rounds).  A loop whose kernels are shorter than the
host's time to issue a call (about 40 us from Python) measures the host; `launches` therefore adds the library's own event pairs around
each kernel (resize launch, apply launch), median and spread of 20 calls.  Next to them the algorithmic bytes per output
pixel of both routes.  The two routes' pixels are compared at the timed size before anything is timed.  `default_is` names the route
the library takes when the environment does not say, and `rule_holds` whether, in that case, it is not slower than the other route by
more than the two spreads added.  Last, not gated: the facade's uhdr_decode of a 4K file of this kind (API-4, 960 x 720 Y400 map) with
and without UHDR_HIP_SEAM_RESIZED_MAP -- without it the applyGainMap of such a file runs on the host cores.
"""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160


def event_ms(ctx, fn, iters):
    """Per-call milliseconds: events on the context's stream around `iters` calls, behind a warm-up of the same call."""
    import torch

    for _ in range(5):
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


def random_map(fmt, w, h, rng, cg):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd.images import Image

    img = Image(fmt, w, h, cg, align=64)
    if fmt == A.UHDR_IMG_FMT_8bppYCbCr400:
        img.valid(0)[:] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    else:
        img.valid(0)[:] = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) | (np.uint32(255) << 24)
    return img


def case(u, ctx, map_fmt, mw, mh, out_ct, iters, rounds, rng):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image

    out_fmt = A.UHDR_IMG_FMT_64bppRGBAHalfFloat if out_ct == A.UHDR_CT_LINEAR else A.UHDR_IMG_FMT_32bppRGBA1010102
    y400 = map_fmt == A.UHDR_IMG_FMT_8bppYCbCr400
    bpp = 1 if y400 else 4
    base = synth.make_sdr_yuv420(W, H).to("cuda:0")
    gm = random_map(map_fmt, mw, mh, rng, A.UHDR_CG_BT_2100).to("cuda:0")
    same = random_map(map_fmt, mw, mw * H // W, rng, A.UHDR_CG_BT_2100).to("cuda:0")
    md = synth.default_metadata(use_base_cg=0, per_channel=not y400)
    d = {k: Image(out_fmt, W, H, align=64, device="cuda:0") for k in ("staged", "fused", "apply", "same")}
    resized = Image(map_fmt, W, H, A.UHDR_CG_BT_2100, align=64, device="cuda:0")

    def any_route(route, dest):
        def run():
            os.environ["UHDR_HIP_APPLY_RESIZE"] = route
            u.applyGainMapAny(base, gm, md, out_ct, out_fmt, A.FLT_MAX, dest)
        return run

    runs = {
        "staged": any_route("staged", d["staged"]),
        "fused": any_route("fused", d["fused"]),
        "staged_resize_only": lambda: u.resizeImage(gm, W, H, dst=resized),
        "staged_apply_only": lambda: u.applyGainMap(base, resized, md, out_ct, out_fmt, A.FLT_MAX, d["apply"]),
        "same_aspect_old_entry": lambda: u.applyGainMap(base, same, md, out_ct, out_fmt, A.FLT_MAX, d["same"]),
    }
    for fn in runs.values():
        fn()
    ctx.synchronize()
    identical = bool((d["staged"].buf == d["fused"].buf).all().item() and (d["staged"].buf == d["apply"].buf).all().item())
    rows = {k: [] for k in runs}
    for _ in range(rounds):  # alternating, each loop behind its own warm-up
        for k, fn in runs.items():
            rows[k].append(event_ms(ctx, fn, iters))
    # the launches on their own: the library's event pairs around each kernel (uhdr_hip_profile_enable), 20 calls per candidate --
    # a call whose kernels take less than the host needs to issue it shows the host's time in the loops above
    kernel_us = {}
    for k in ("staged", "fused", "same_aspect_old_entry"):
        ctx.synchronize()
        ctx.profile(True)
        ctx.profile_read_list(None)
        for _ in range(20):
            runs[k]()
        ctx.synchronize()
        rz, ap = ctx.profile_read_list("resize_image", reset=False), ctx.profile_read_list("apply_gainmap")
        ctx.profile(False)
        kernel_us[k] = {"apply_gainmap_launch_us": float(np.median(ap)) * 1e3, "apply_gainmap_launch_spread_us": float(max(ap) - min(ap)) * 1e3}
        if rz:
            kernel_us[k].update(resize_image_launch_us=float(np.median(rz)) * 1e3, resize_image_launch_spread_us=float(max(rz) - min(rz)) * 1e3)
    os.environ.pop("UHDR_HIP_APPLY_RESIZE", None)
    out = dict(base=f"{W}x{H} 4:2:0", map=f"{mw}x{mh} {'Y400' if y400 else 'RGBA8888'}", output="linear f16" if out_ct == A.UHDR_CT_LINEAR else "pq 1010102",
               identical_pixels=identical)
    for k, v in rows.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_spread_ms"] = float(max(v) - min(v))
        out[k + "_rounds_ms"] = v
    out["launches"] = kernel_us
    px = W * H
    io_bytes = 1.5 + (8 if out_ct == A.UHDR_CT_LINEAR else 4)
    map_b = mw * mh * bpp / px
    out["algorithmic_bytes_per_pixel"] = {"fused": io_bytes + map_b, "staged": io_bytes + map_b + 2 * bpp,
                                          "note": "base 1.5 + output + the map once; staged adds the resized map written and read back"}
    return out


def facade_rows(n=5):
    """uhdr_decode of a 4K API-4 file whose 960 x 720 Y400 map lies under a 3840 x 2160 base, acceleration on, with and without the switch."""
    import ctypes as C

    from PIL import Image as PImage

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import facade as FA
    from libultrahdr_amd import synth

    lib = FA.load()
    lib.uhdr_enc_set_compressed_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_compressed_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.c_int]
    lib.uhdr_enc_set_gainmap_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_gainmap_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.POINTER(A.GainmapMetadata)]

    def jpeg(a, **kw):
        buf = io.BytesIO()
        PImage.fromarray(a).save(buf, format="JPEG", **kw)
        return buf.getvalue()

    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([64 + xx * 180 // W, 64 + yy * 180 // H, 64 + (xx + yy) * 61 % 180], -1)
    base = jpeg(np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8), quality=90, subsampling=2)
    yy, xx = np.mgrid[0:720, 0:960]
    gm = jpeg(np.clip((xx + yy) // 7 % 256 + rng.integers(-4, 5, (720, 960)), 0, 255).astype(np.uint8), quality=95)
    md = synth.default_metadata(use_base_cg=1)
    keep = []

    def ci(data):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        keep.append(buf)
        return FA.CompressedImage(C.cast(buf, C.c_void_p), len(data), len(data), A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE)

    b, g = ci(base), ci(gm)
    h = lib.uhdr_create_encoder()
    try:
        FA._chk(lib.uhdr_enc_set_compressed_image(h, C.byref(b), FA.UHDR_BASE_IMG))
        FA._chk(lib.uhdr_enc_set_gainmap_image(h, C.byref(g), C.byref(md)))
        FA._chk(lib.uhdr_encode(h))
        o = lib.uhdr_get_encoded_stream(h).contents
        jpegr = C.string_at(o.data, o.data_sz)
    finally:
        lib.uhdr_release_encoder(h)
    out = {"file": f"API-4, {W}x{H} 4:2:0 base, 960x720 Y400 map, {len(jpegr)} bytes", "output": "linear f16", "decodes": n}
    px = {}
    for name, switch in (("without_switch", False), ("with_switch", True)):
        os.environ.pop("UHDR_HIP_SEAM_RESIZED_MAP", None)
        if switch:
            os.environ["UHDR_HIP_SEAM_RESIZED_MAP"] = "1"
        t = []
        for k in range(n + 2):  # two warm-up decodes
            px[name] = FA.decode(jpegr, A.UHDR_CT_LINEAR, A.UHDR_IMG_FMT_64bppRGBAHalfFloat, gpu=True)
            if k >= 2:
                t.append(FA.last_call_seconds * 1e3)
        out[name + "_ms"] = float(np.median(t))
        out[name + "_spread_ms"] = float(max(t) - min(t))
        out[name + "_calls_ms"] = t
    os.environ.pop("UHDR_HIP_SEAM_RESIZED_MAP", None)
    out["identical_pixels"] = bool(np.array_equal(px["without_switch"], px["with_switch"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-facade", action="store_true")
    args = ap.parse_args()
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import facade as FA
    from libultrahdr_amd.ultrahdr import Context, UltraHdr

    ctx = Context(0)  # raises without a GPU: there is nothing to time on a CPU
    u = UltraHdr(ctx=ctx)
    os.environ.pop("UHDR_HIP_APPLY_RESIZE", None)
    rows = []
    for fmt, mw, mh in ((A.UHDR_IMG_FMT_8bppYCbCr400, 960, 720), (A.UHDR_IMG_FMT_32bppRGBA8888, 1920, 1440)):
        for ct in (A.UHDR_CT_LINEAR, A.UHDR_CT_PQ):
            r = case(u, ctx, fmt, mw, mh, ct, args.iters, args.rounds, np.random.default_rng(7))
            rows.append(r)
            print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds_ms")}), flush=True)
    ctx.close()
    result = {"cases": rows}
    for r in rows:
        lo, hi = ("staged", "fused") if r["staged_ms"] <= r["fused_ms"] else ("fused", "staged")
        r["faster"] = lo
        r["margin_ms"] = r[hi + "_ms"] - r[lo + "_ms"]
        r["spreads_added_ms"] = r["staged_spread_ms"] + r["fused_spread_ms"]
    if not args.no_facade and FA.available():
        result["facade_uhdr_decode_4k"] = facade_rows()
        print(json.dumps({k: v for k, v in result["facade_uhdr_decode_4k"].items() if not k.endswith("_calls_ms")}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
