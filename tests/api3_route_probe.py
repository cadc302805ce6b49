"""Child process of tests/test_gpu_api3_scans.py::test_both_routes_give_the_same_bytes: runs the one-call API-3 encode under whatever
UHDR_HIP_API3_ROUTE the parent set and prints one JSON line -- per case the SHA-256 and the length of the map scan, the metadata
and the gain-map description."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_api3_scans as M  # noqa: E402

if __name__ == "__main__":
    print(json.dumps(M.probe()))
