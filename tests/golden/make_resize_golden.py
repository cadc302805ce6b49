"""Writes tests/golden/resize_image_ref.npz: for every case of tests/test_resize_port.py the inputs, the metadata and what the REAL
reference's applyGainMap returns for a gain map of another aspect ratio than the base image (its resize_image runs inside).  Needs the
reference built under oracle/_ref; run once, from the repository root:  python tests/golden/make_resize_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import resize_cases as K  # noqa: E402
from test_resize_port import CASES, OUTPUTS, METADATA, case_inputs, case_key  # noqa: E402
from oracle import loader as L  # noqa: E402


def main():
    assert L.ref() is not None, "oracle/_ref is not built"
    out = {"metadata": np.array([METADATA["max_boost"], METADATA["min_boost"], METADATA["gamma"]], np.float64)}
    for geom, fmt_name in CASES:
        base, gm = case_inputs(geom, fmt_name)
        key = case_key(geom, fmt_name)
        out[K.geom_id(geom) + "/base"] = base.valid(0).copy()  # one base image per geometry
        out[key + "/map"] = gm.valid(0).copy()
        for ct_name, ct in OUTPUTS.items():
            out[key + "/" + ct_name] = L.apply_gainmap("ref", base, gm, METADATA["md"](), ct).valid(0).copy()
    path = os.path.join(HERE, "resize_image_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
