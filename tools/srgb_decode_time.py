"""The 4:2:0 / 4:2:2 -> RGB decode on the device (uhdr_hip_idct_upsample_rgb_dev, uhdr_hip_idct_upsample_rgb422_dev: one kernel
template in jpeg_upsample.hip, idct_upsample_rgb_kernel<BPP, VARIANT, VSAMP>) at 4K and 8K, next to the 4:4:4 idct_dequant_rgb_kernel, the
whole-file entry (uhdr_hip_jpeg_decode_rgb / _rgb_any), and uhdr_decode to SRGB / RGBA8888 through the drop-in libuhdr.so with
and without GPU acceleration.

    python tools/srgb_decode_time.py [--iters 50] [--json out.json]        per-call times (see below) + the facade decode
    python tools/srgb_decode_time.py --kernel-trace DIR                     kernel times: one rocprofv3 --kernel-trace child
                                                                            process per size, durations read from its database
    --sampling 420 | 422 | both                                             which subsampled decode(s) to run (default 420;
                                                                            a trace with both puts the two kernels in one run)
    --sizes 4K 8K                                                           sizes of the per-call / trace runs

Per-call times are torch events around a loop of Python calls of the entry (ctypes tables, the stream handshake and, for
variant 0, the two chroma IDCT launches included): a bound on what a caller pays, not a kernel time.  Kernel times come from
the trace; the fraction of 8 TB/s is taken on algorithmic bytes: 3 B/px of int16 coefficients in (1.5 samples per pixel) +
4 (3) B/px out for 4:2:0, 4 B/px in (2 samples per pixel) for 4:2:2, 6 B/px in for 4:4:4.  Variant 0's kernel time is the
upsampling kernel plus its two chroma idct_dequant_kernel launches (1 B/px more through HBM for 4:2:0, 2 B/px for 4:2:2, not
counted as algorithmic); a trace with both samplings cannot tell whose launches those are and takes their average per launch
apart by grid size.
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def _time(fn, iters):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


SIZES = {"4K": (3840, 2160), "8K": (7680, 4320)}


def _inputs(w, h, rng, sampling="420"):
    import torch

    from oracle import loader as L

    cgrid = ((h + 15) // 16, (w + 15) // 16) if sampling == "420" else ((h + 7) // 8, ((w + 1) // 2 + 7) // 8)
    grids = [((h + 7) // 8, (w + 7) // 8), cgrid, cgrid]
    coefs = []
    for bh, bw in grids:
        c = rng.integers(-3, 4, (bh, bw, 64)).astype(np.int16)
        c[..., 0] = rng.integers(-60, 61, (bh, bw))
        coefs.append(torch.from_numpy(c).to("cuda:0"))
    c444 = [torch.from_numpy(rng.integers(-3, 4, (grids[0][0], grids[0][1], 64)).astype(np.int16)).to("cuda:0") for _ in range(3)]
    qts = [L.quant_table_port(90, False), L.quant_table_port(90, True), L.quant_table_port(90, True)]
    return coefs, c444, qts


def _samplings(arg):
    return ("420", "422") if arg == "both" else (arg,)


def _per_call(u, sizes, iters, rng, sampling="420"):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd.images import Image

    rows = []
    for name in sizes:
        w, h = SIZES[name]
        ins = {s: _inputs(w, h, rng, s) for s in _samplings(sampling)}
        c444, qts = next(iter(ins.values()))[1:]
        for ch, fmt in ((4, A.UHDR_IMG_FMT_32bppRGBA8888), (3, A.UHDR_IMG_FMT_24bppRGB888)):
            dst = Image(fmt, w, h, align=64, device="cuda:0")
            for s, (coefs, _, _) in ins.items():
                fn, entry = (u.idct_upsample_rgb, "uhdr_hip_idct_upsample_rgb_dev") if s == "420" else (u.idct_upsample_rgb422, "uhdr_hip_idct_upsample_rgb422_dev")
                for variant in (0, 1):
                    t = _time(lambda: fn(coefs, qts, w, h, fmt, variant, dst=dst), iters)
                    rows.append(dict(entry=f"{entry} v{variant}", size=name, channels=ch, per_call_us=t * 1e6))
            t = _time(lambda: u.idct_dequant_rgb(c444, qts[0], qts[1], w, h, fmt, 0, dst=dst), iters)
            rows.append(dict(entry="uhdr_hip_idct_dequant_rgb_dev (4:4:4)", size=name, channels=ch, per_call_us=t * 1e6))
    return rows


def _api3_jpegr(hdr, sdr_jpeg):
    """uhdr_encode of a raw HDR intent + a compressed SDR intent (API-3) through the drop-in, GPU acceleration off: the JpegR
    keeps sdr_jpeg's scan as its base image."""
    import ctypes as C

    from libultrahdr_amd import capi as A
    from libultrahdr_amd import facade as FA

    lib = FA.load()
    lib.uhdr_enc_set_compressed_image.restype = A.ErrorInfo
    lib.uhdr_enc_set_compressed_image.argtypes = [C.c_void_p, C.POINTER(FA.CompressedImage), C.c_int]
    buf = (C.c_uint8 * len(sdr_jpeg)).from_buffer_copy(sdr_jpeg)
    ci = FA.CompressedImage(C.cast(buf, C.c_void_p), len(sdr_jpeg), len(sdr_jpeg), A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE)
    h = lib.uhdr_create_encoder()
    try:
        FA._chk(lib.uhdr_enc_set_raw_image(h, C.byref(hdr.raw), FA.UHDR_HDR_IMG))
        FA._chk(lib.uhdr_enc_set_compressed_image(h, C.byref(ci), FA.UHDR_SDR_IMG))
        FA._chk(lib.uhdr_encode(h))
        o = lib.uhdr_get_encoded_stream(h).contents
        return C.string_at(o.data, o.data_sz)
    finally:
        lib.uhdr_release_encoder(h)


def _whole_file_and_facade(u, rng, sampling="420"):
    """4K: the whole-file entry against Pillow's libjpeg-turbo on the host, and uhdr_decode to SRGB / RGBA8888 through the
    facade with and without GPU acceleration (the facade links IJG 9: its CPU route is that libjpeg).  4:2:2: the JpegR is an
    API-3 encode around the Pillow-written file, so its base image is that file's 4:2:2 scan."""
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import facade as FA
    from libultrahdr_amd import synth

    rows = []
    w, h = SIZES["4K"]
    try:
        from PIL import Image as PImage

        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 97 % 256)], -1).astype(np.uint8)
        a = np.clip(a.astype(np.int32) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        PImage.fromarray(a, "RGB").save(buf, format="JPEG", quality=95, subsampling=2 if sampling == "420" else 1)
        jpeg = buf.getvalue()
        out = np.empty((h, w, 4), np.uint8)
        decode = u.jpeg_decode_rgb if sampling == "420" else u.jpeg_decode_rgb_any
        for _ in range(3):
            decode(jpeg, 4, 0, out=out)
        n = 20
        t0 = time.perf_counter()
        for _ in range(n):
            decode(jpeg, 4, 0, out=out)
        t_gpu = (time.perf_counter() - t0) / n
        t0 = time.perf_counter()
        for _ in range(n):
            cpu = np.asarray(PImage.open(io.BytesIO(jpeg)).convert("RGBA"))
        t_cpu = (time.perf_counter() - t0) / n
        entry = "uhdr_hip_jpeg_decode_rgb" if sampling == "420" else "uhdr_hip_jpeg_decode_rgb_any"
        rows.append(dict(entry=f"{entry} (variant 0) vs Pillow's libjpeg-turbo on the host, one 4:{sampling[1]}:{sampling[2]} file", size="4K",
                         gpu_ms=t_gpu * 1e3, pillow_ms=t_cpu * 1e3, bytes=len(jpeg), identical=bool(np.array_equal(out, cpu))))
    except ImportError:
        if sampling == "422":
            raise SystemExit("--sampling 422 needs Pillow to write the 4:2:2 file")
    if os.path.isfile(FA.PATH):
        sdr = synth.make_sdr_yuv420(w, h)
        hdr = synth.make_hdr_p010(w, h, ct=A.UHDR_CT_HLG)
        jpegr = FA.encode(hdr, sdr, gpu=True) if sampling == "420" else _api3_jpegr(hdr, jpeg)
        res = {}
        for gpu in (False, True):
            ts = []
            for _ in range(6):
                px = FA.decode(jpegr, A.UHDR_CT_SRGB, A.UHDR_IMG_FMT_32bppRGBA8888, gpu=gpu)
                ts.append(FA.last_call_seconds)
            res[gpu] = (float(np.median(ts[1:])), px)
        st = A.seam_stats()
        A.seam_stats(reset=True)
        rows.append(dict(entry=f"facade uhdr_decode -> SRGB / RGBA8888 ({'API-1' if sampling == '420' else 'API-3'} JpegR, 4:{sampling[1]}:{sampling[2]} base, "
                               "median of 5 after one warm-up)", size="4K",
                         gpu_ms=res[True][0] * 1e3, cpu_ms=res[False][0] * 1e3, identical=bool(np.array_equal(res[True][1], res[False][1])),
                         device_route_calls=st.get("jpeg_decode_rgb", {}).get("device", 0)))
    return rows


def _kernel_trace(outdir, iters, sampling="420", sizes=tuple(SIZES)):
    """One rocprofv3 --kernel-trace child per size (this script with --launch-only); kernel durations from its database."""
    import glob
    import sqlite3
    import subprocess

    rows = []
    for name in sizes:
        w, h = SIZES[name]
        d = os.path.join(outdir, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "k", "--", sys.executable, os.path.abspath(__file__), "--launch-only", name,
               "--iters", str(iters), "--sampling", sampling]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit(f"rocprofv3 run for {name} ended with {p.returncode}:\n{p.stderr[-2000:]}")
        db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        con = sqlite3.connect(db[0])
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type='table'")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        seq = list(con.execute(f"select s.kernel_name, d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"))
        con.close()
        # per kernel symbol: the durations of its launches; a variant-0 launch also carries the two chroma idct_dequant_kernel
        # launches enqueued right before it (the same kernel serves both samplings, so they are told apart by position)
        runs, pending = {}, []
        for kname, ns in seq:
            if "idct_dequant_kernel" in kname:
                pending.append(ns)
                continue
            if "idct_upsample_rgb" in kname and len(pending) >= 2:
                ns += pending[-1] + pending[-2]
            pending = []
            runs.setdefault(kname, []).append(ns)

        def find(kname, *targs):
            """The launches (ns each) of the kernel `kname` with these template arguments; the symbol table may hold demangled
            or mangled names (<4, 0> / ILi4ELi0EE)."""
            dem = "<" + ", ".join(str(t) for t in targs) + ">"
            man = "I" + "".join(f"Li{t}E" for t in targs) + "E"
            hits = [v for n, v in runs.items() if kname in n and (dem in n or man in n)]
            return hits[0] if hits else None

        def row(label, v, ch, in_bytes):
            v = np.asarray(v[3:] if len(v) > 3 else v, dtype=np.float64)  # the first three launches are _time's warm-up
            ns = float(v.mean())
            return dict(kernel=label, size=name, channels=ch, launches=int(v.size), kernel_us=ns / 1e3, min_us=float(v.min()) / 1e3,
                        std_us=float(v.std()) / 1e3, ns_per_mpx=ns / (w * h / 1e6), alg_bytes_per_px=in_bytes + ch,
                        frac_8tbs=(in_bytes + ch) * w * h / (ns * 1e-9) / PEAK)

        # the rows keep the labels of the time when 4:2:2 had a kernel of its own (profiles/srgb422_decode_times.json); a
        # library of that time is still found by those names, so that it can be timed next to a current one
        for ch in (4, 3):
            for kname, vsamp, in_bytes in (("idct_upsample_rgb_kernel", 2, 3), ("idct_upsample_rgb422_kernel", 1, 4)):
                for variant in (0, 1):
                    v = find("idct_upsample_rgb_kernel", ch, variant, vsamp) or find(kname, ch, variant)
                    if v is not None:
                        rows.append(row(f"{kname}<{ch},{variant}>" + (" + 2 x idct_dequant_kernel" if variant == 0 else ""), v, ch, in_bytes))
            v = find("idct_dequant_rgb_kernel", ch)
            if v is not None:
                rows.append(row(f"idct_dequant_rgb_kernel<{ch}> (4:4:4)", v, ch, 6))
        if not any(r["size"] == name for r in rows):
            raise SystemExit(f"no decode kernels found in the {name} trace; kernels seen: {sorted(runs)}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    ap.add_argument("--launch-only", default=None, choices=sorted(SIZES))
    ap.add_argument("--sampling", default="420", choices=("420", "422", "both"))
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=sorted(SIZES))
    args = ap.parse_args()
    if args.kernel_trace:
        rows = _kernel_trace(args.kernel_trace, args.iters, args.sampling, args.sizes)
    else:
        from libultrahdr_amd.ultrahdr import Context, UltraHdr

        ctx = Context(0)
        u = UltraHdr(ctx=ctx)
        rng = np.random.default_rng(1)
        if args.launch_only:
            _per_call(u, [args.launch_only], args.iters, rng, args.sampling)
            ctx.close()
            return
        rows = _per_call(u, args.sizes, args.iters, rng, args.sampling)
        for s in _samplings(args.sampling):
            rows += _whole_file_and_facade(u, rng, s)
        ctx.close()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
