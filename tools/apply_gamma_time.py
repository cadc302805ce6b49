"""applyGainMap with a gain-map gamma other than 1 at a map scale other than 1, 3840 x 2160 4:2:0 base, gamma 1.571: the threshold-table
route (UHDR_HIP_APPLY_GAMMA_TABLE: uhdr_hip_apply_gainmap_ex_dev, uhdr_hip_apply_gainmap_coef_ex_dev) against the pow-per-sample route
of the older entry points.

    python tools/apply_gamma_time.py [--parent-lib PATH] [--calls 20] [--rounds 5] [--json profiles/apply_gamma_time.json]

    table      planes input:       uhdr_hip_apply_gainmap_ex_dev with the flag                      (this build)
               coefficient input:  uhdr_hip_apply_gainmap_coef_ex_dev with the flag                 (this build)
    pow        planes input:       uhdr_hip_apply_gainmap_dev                                       (the yardstick library)
               coefficient input:  3 x uhdr_hip_idct_dequant_dev + uhdr_hip_apply_gainmap_dev       (the yardstick library)

The yardstick library is --parent-lib (a libuhdr_hip.so built from the parent commit, loaded beside this build's in the same process)
or, without it, this build's own older entry points, which launch the same kernels.  Maps: Y400 at scale 4 and RGB888 at scale 2;
outputs linear RGBA half float and PQ RGBA1010102.  Times are the library's own event pairs around each launch
(uhdr_hip_profile_enable), `calls` calls per candidate and round, the candidates alternating, `rounds` rounds: the median of the rounds'
medians and their spread (max - min).  `rule_holds`: the table route's median is below the yardstick's by more than the two spreads
added.  Before anything is timed the two routes' outputs are compared: they may differ by one output code on at most 0.1 % of the
samples (the pow route's allowance against the reference; the table route is the reference's, tests/test_gpu_apply_gamma.py).  For
orientation, not gated: the same geometry at gamma 1 on this build, and an 7680 x 4320 base under a Y400 map at scale 4 as a fraction
of 8 TB/s.  The host's time to build one threshold table is recorded first (uhdr_hip_gamma_index_eval, before any call needs it).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA = 1.571
NEEDED = ("uhdr_hip_create", "uhdr_hip_destroy", "uhdr_hip_synchronize", "uhdr_hip_profile_enable", "uhdr_hip_profile_read_list",
          "uhdr_hip_apply_gainmap_dev", "uhdr_hip_idct_dequant_dev")


class Lib:
    """A libuhdr_hip.so and one context of it on its own stream; launches are timed by the library's event pairs."""

    def __init__(self, path):
        from libultrahdr_amd import capi as A

        self.A = A
        self.lib = A.load() if path is None else C.CDLL(path)
        if path is not None:
            for name in NEEDED:
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = A._SIGS[name]
        err = A.ErrorInfo()
        self.handle = self.lib.uhdr_hip_create(0, C.byref(err))
        if not self.handle:
            raise A.UhdrError(err.error_code, err.detail.decode("utf-8", "replace"))

    def sync(self):
        self.A.check(self.lib.uhdr_hip_synchronize(self.handle))

    def timed(self, fn, calls, families):
        """-> per call, the summed milliseconds of the launches of `families` ({family: launches per call})."""
        for _ in range(3):
            fn()
        self.sync()
        self.lib.uhdr_hip_profile_enable(self.handle, 1)
        self.read(None)
        for _ in range(calls):
            fn()
        self.sync()
        per_call = np.zeros(calls)
        for fam, k in families.items():
            v = self.read(fam)
            assert len(v) == calls * k, (fam, len(v), calls * k)
            per_call += np.asarray(v).reshape(calls, k).sum(1)
        left = self.read(None)
        assert not left, f"launches outside {list(families)}: {len(left)}"
        self.lib.uhdr_hip_profile_enable(self.handle, 0)
        return float(np.median(per_call))

    def read(self, family, capacity=65536):
        buf = (C.c_double * capacity)()
        n = self.lib.uhdr_hip_profile_read_list(self.handle, family.encode() if family else None, buf, capacity, 1)
        return list(buf[: min(n, capacity)])

    def close(self):
        self.lib.uhdr_hip_destroy(self.handle)


def random_map(fmt, w, h, rng, cg):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd.images import Image

    img = Image(fmt, w, h, cg, align=64)
    v = img.valid(0)
    v[:] = rng.integers(0, 256, v.shape, dtype=np.uint8)
    return img


def coef_inputs(w, h, rng):
    """Coefficient arrays of a 4:2:0 frame on libjpeg's grids (a DC level and a few low frequencies per block) and three tables."""
    import torch

    from oracle import loader as L

    qts = [L.quant_table_port(90, False), L.quant_table_port(90, True), L.quant_table_port(85, True)]
    coefs = []
    for cw, ch in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        bw, bh = (cw + 7) // 8, (ch + 7) // 8
        c = np.zeros((bh, bw, 64), dtype=np.int16)
        c[:, :, 0] = rng.integers(-40, 41, (bh, bw))
        for k in (1, 8, 9, 2, 16):
            c[:, :, k] = rng.integers(-6, 7, (bh, bw))
        coefs.append(torch.from_numpy(c).to("cuda:0"))
    return coefs, qts


def spread_rule(rows_new, rows_old):
    new, old = float(np.median(rows_new)), float(np.median(rows_old))
    s_new, s_old = float(max(rows_new) - min(rows_new)), float(max(rows_old) - min(rows_old))
    return dict(table_us=new * 1e3, table_spread_us=s_new * 1e3, pow_us=old * 1e3, pow_spread_us=s_old * 1e3, margin_us=(old - new) * 1e3,
                spreads_added_us=(s_new + s_old) * 1e3, rule_holds=bool(old - new > s_new + s_old), table_rounds_us=[x * 1e3 for x in rows_new],
                pow_rounds_us=[x * 1e3 for x in rows_old])


def allowance(a, b, linear):
    """Differences between two outputs in output codes: (max, fraction of samples that differ)."""
    if linear:
        x, y = a.view(np.uint16).astype(np.int64), b.view(np.uint16).astype(np.int64)
    else:
        x = np.stack([(a.astype(np.int64) >> s) & 0x3FF for s in (0, 10, 20)], -1)
        y = np.stack([(b.astype(np.int64) >> s) & 0x3FF for s in (0, 10, 20)], -1)
    d = np.abs(x - y)
    return int(d.max()), float((d != 0).mean())


def case(new, old, w, h, three, scale, out_ct, calls, rounds, rng, coef):
    from libultrahdr_amd import capi as A
    from libultrahdr_amd import synth
    from libultrahdr_amd.images import Image

    linear = out_ct == A.UHDR_CT_LINEAR
    out_fmt = A.UHDR_IMG_FMT_64bppRGBAHalfFloat if linear else A.UHDR_IMG_FMT_32bppRGBA1010102
    gm = random_map(A.UHDR_IMG_FMT_24bppRGB888 if three else A.UHDR_IMG_FMT_8bppYCbCr400, w // scale, h // scale, rng, A.UHDR_CG_BT_2100).to("cuda:0")
    md = synth.default_metadata(use_base_cg=0, per_channel=three, gamma=GAMMA)
    md1 = synth.default_metadata(use_base_cg=0, per_channel=three)
    d_new, d_old, d_one = (Image(out_fmt, w, h, align=64, device="cuda:0") for _ in range(3))
    GT = A.UHDR_HIP_APPLY_GAMMA_TABLE
    chk = A.check
    if coef is None:
        base = synth.make_sdr_yuv420(w, h).to("cuda:0")
        run_new = lambda: chk(new.lib.uhdr_hip_apply_gainmap_ex_dev(new.handle, C.byref(base.raw), C.byref(gm.raw), C.byref(md), out_ct, out_fmt, A.FLT_MAX,
                                                                    C.byref(d_new.raw), 0, 0, GT))
        run_old = lambda: chk(old.lib.uhdr_hip_apply_gainmap_dev(old.handle, C.byref(base.raw), C.byref(gm.raw), C.byref(md), out_ct, out_fmt, A.FLT_MAX,
                                                                 C.byref(d_old.raw), 0, 0))
        run_one = lambda: chk(new.lib.uhdr_hip_apply_gainmap_ex_dev(new.handle, C.byref(base.raw), C.byref(gm.raw), C.byref(md1), out_ct, out_fmt, A.FLT_MAX,
                                                                    C.byref(d_one.raw), 0, 0, GT))
        fam_old = {"apply_gainmap": 1}
    else:
        coefs, qts = coef
        jc = A.JpegCoefficients()
        for i in range(3):
            jc.coef[i] = coefs[i].data_ptr()
            jc.blocks_h[i], jc.blocks_w[i] = int(coefs[i].shape[0]), int(coefs[i].shape[1])
            for k in range(64):
                jc.qtable[i][k] = int(qts[i][k])
        planes = Image(A.UHDR_IMG_FMT_12bppYCbCr420, w, h, A.UHDR_CG_BT_709, A.UHDR_CT_SRGB, A.UHDR_CR_FULL_RANGE, align=64, device="cuda:0")
        qt = [(C.c_uint16 * 64)(*[int(v) for v in q]) for q in qts]
        for i in range(3):  # the IDCT writes whole blocks: the planes must hold them
            rows, stride, _ = planes.layout[i]
            assert rows == jc.blocks_h[i] * 8 and stride >= jc.blocks_w[i] * 8

        def run_old():
            for i in range(3):
                chk(old.lib.uhdr_hip_idct_dequant_dev(old.handle, C.c_void_p(coefs[i].data_ptr()), jc.blocks_w[i], jc.blocks_h[i], qt[i],
                                                      C.c_void_p(planes.raw.planes[i]), planes.raw.stride[i]))
            chk(old.lib.uhdr_hip_apply_gainmap_dev(old.handle, C.byref(planes.raw), C.byref(gm.raw), C.byref(md), out_ct, out_fmt, A.FLT_MAX, C.byref(d_old.raw), 0, 0))

        run_new = lambda: chk(new.lib.uhdr_hip_apply_gainmap_coef_ex_dev(new.handle, C.byref(jc), 420, w, h, A.UHDR_CG_BT_709, C.byref(gm.raw), C.byref(md), out_ct,
                                                                         out_fmt, A.FLT_MAX, C.byref(d_new.raw), GT))
        run_one = lambda: chk(new.lib.uhdr_hip_apply_gainmap_coef_ex_dev(new.handle, C.byref(jc), 420, w, h, A.UHDR_CG_BT_709, C.byref(gm.raw), C.byref(md1), out_ct,
                                                                         out_fmt, A.FLT_MAX, C.byref(d_one.raw), GT))
        fam_old = {"idct_dequant": 3, "apply_gainmap": 1}
    run_new(), run_old()
    new.sync(), old.sync()
    dmax, dfrac = allowance(d_new.to_host().valid(0), d_old.to_host().valid(0), linear)
    within = dmax <= 1 and dfrac <= 0.001
    rows_new, rows_old, rows_one = [], [], []
    for _ in range(rounds):  # alternating
        rows_new.append(new.timed(run_new, calls, {"apply_gainmap_gamma_quad": 1}))
        rows_old.append(old.timed(run_old, calls, fam_old))
        rows_one.append(new.timed(run_one, calls, {"apply_gainmap": 1}))
    out = dict(base=f"{w}x{h} 4:2:0", input="coefficients" if coef is not None else "planes", map=f"{'RGB888' if three else 'Y400'} at scale {scale}",
               output="linear f16" if linear else "pq 1010102", outputs_max_code_diff=dmax, outputs_fraction_differing=dfrac, outputs_within_allowance=within)
    out.update(spread_rule(rows_new, rows_old))
    out["gamma_1_same_geometry_us"] = float(np.median(rows_one)) * 1e3
    in_b = (3.0 if coef is not None else 1.5) + (3 if three else 1) / (scale * scale)
    out["bytes_per_pixel"] = in_b + (8 if linear else 4)
    out["table_fraction_of_8TBs"] = out["bytes_per_pixel"] * w * h / (out["table_us"] * 1e-6) / 8e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from libultrahdr_amd import capi as A

    info = (C.c_uint32 * 4)()
    rc = A.load().uhdr_hip_gamma_index_eval(C.c_float(GAMMA), None, None, 0, info, None)
    result = {"gamma": GAMMA, "table_verified_exact": bool(rc == 0 and info[0] == 1), "table_build_us": int(info[2]),
              "yardstick": "parent library" if args.parent_lib else "this build's older entry points", "cases": []}
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}), flush=True)
    new = Lib(None)  # raises without a GPU: there is nothing to time on a CPU
    old = Lib(args.parent_lib) if args.parent_lib else new
    rng = np.random.default_rng(7)
    coef = coef_inputs(3840, 2160, rng)
    for use_coef in (None, coef):
        for three, scale in ((False, 4), (True, 2)):
            for ct in (A.UHDR_CT_LINEAR, A.UHDR_CT_PQ):
                r = case(new, old, 3840, 2160, three, scale, ct, args.calls, args.rounds, rng, use_coef)
                result["cases"].append(r)
                print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds_us")}), flush=True)
    r = case(new, old, 7680, 4320, False, 4, A.UHDR_CT_LINEAR, args.calls, args.rounds, rng, None)
    result["orientation_8k"] = r
    print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds_us")}), flush=True)
    if old is not new:
        old.close()
    new.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
