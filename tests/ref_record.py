"""Recorded answers of the real reference (oracle/_ref) for the CPU tests that compare the C port against it.

Where oracle/_ref is built, the wrapped calls run live and what they return -- reduced to JSON by `fingerprint` -- must
equal what the test's entry in tests/golden/<file> holds; elsewhere the entry is replayed through `replay`, so the
comparison runs on every machine.  With UHDR_RECORD_REF_ANSWERS=1 (and oracle/_ref built) the entries are rewritten."""
import json
import os

import pytest

from libultrahdr_amd import capi as A
from oracle import loader as L

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = bool(os.environ.get("UHDR_RECORD_REF_ANSWERS"))


def answers(request, monkeypatch, golden_name, owner, names, fingerprint, replay, is_ref=lambda *a, **kw: True):
    """Generator for a fixture: wraps owner.<name> for each name; calls for which is_ref(*args) holds are the reference's.
    fingerprint(name, args, result) -> JSON item; replay(name, item) -> the result a test sees, live or not.  An A.UhdrError
    the reference raises is kept as {"error": code} and raised again on replay."""
    path = os.path.join(GOLDEN_DIR, golden_name)
    with open(path) as f:
        golden = json.load(f)
    key = request.node.name
    live = L.ref() is not None
    if RECORD and not live:
        pytest.fail("UHDR_RECORD_REF_ANSWERS needs oracle/_ref")
    recorded = golden.get(key)
    assert RECORD or recorded is not None, f"{key} is not in {path}"
    calls = []

    def wrap(name):
        real = getattr(owner, name)

        def fn(*a, **kw):
            if not is_ref(*a, **kw):
                return real(*a, **kw)
            if not live:
                assert len(calls) < len(recorded), f"{key}: more reference calls than recorded"
                item = recorded[len(calls)]
                calls.append(item)
                if isinstance(item, dict) and "error" in item:
                    raise A.UhdrError(item["error"], "recorded reference answer")
                return replay(name, item)
            try:
                out = real(*a, **kw)
            except A.UhdrError as e:
                calls.append({"error": e.code})
                raise
            calls.append(fingerprint(name, a, out))
            return replay(name, calls[-1])

        monkeypatch.setattr(owner, name, fn)

    for name in names:
        wrap(name)
    yield
    if RECORD:
        with open(path) as f:
            golden = json.load(f)
        golden[key] = calls
        with open(path, "w") as f:
            json.dump(golden, f, indent=0, sort_keys=True)
            f.write("\n")
    else:
        assert calls == recorded, f"{key}: the reference's answers differ from the record"
