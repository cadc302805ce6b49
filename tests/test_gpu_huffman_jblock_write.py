"""GPU: write form 3 of the self-synchronising Huffman decoder (csrc/huffman_decode_sync.hip: write_span2<true>, dc_partial3_kernel,
dc_apply3_kernel) -- scans whose components are all sampled 1x1 are stored straight into the JBLOCK arrays (natural order, zero-filled
by pass 0), and the DC prediction happens in place; no scan-order scratch, no placing pass.

The cases are the small noise-textured scans of tests/test_gpu_huffman_straggler.py (256 x 256, subsequence size pinned, one lockstep
level) and its protocol: the decode gives back the coefficients that were coded, exactly, and the library's debug output
(UHDR_HIP_HUFF_DEBUG) says which route ran -- the kernel-times line names the write form of every hypothesis attempt, the rounds print
a line of their own.  Output tensors are filled with a non-zero pattern first wherever the test allocates them itself: a block whose
coded coefficients are all zero comes out right only if the zero fill reached it.

  1. form 3 for 4:4:4 and one-component scans, q95 / q100, whole subsequences (512 bits) and four pieces (1024 bits);
  2. the same scans with UHDR_HIP_HUFF_WRITE=2: form 2, as before;
  3. a 248 x 216 4:4:4 scan: 31 x 27 blocks, 2511 blocks in all -- the last DC chunk (256 scan positions) is partial, rows of odd length;
  4. a last subsequence shorter than 64 bits;
  5. q100 full-scale noise: the pinned hypothesis attempt (form 3) loses the true path and stores garbage, the rounds (form 1) repeat the
     decode into arrays that must have been zeroed again;
  6. 4:2:0 and 4:2:2 keep form 2;
  7. three separately allocated component tensors with guard tensors between them: three fill regions, nothing outside them touched.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from oracle import loader as L
from test_gpu_huffman_straggler import SAMPLINGS, _case, _dev, _parallel, decode_with_stragglers

pytestmark = pytest.mark.gpu

FORM_LINE = re.compile(r"hypothesis decode kernels \(write form (\d)\)")
ROUNDS_LINE = re.compile(r"rounds decode of \d+ bytes, \d+ subsequences of \d+ bits \(write form (\d)\): (\w+)")


@pytest.fixture(scope="module")
def uhdr(hip_ctx):
    from libultrahdr_amd.ultrahdr import UltraHdr

    return UltraHdr(ctx=hip_ctx)


class _Tee:
    """capfd for decode_with_stragglers, keeping what it reads (the helper prints only the attempt lines)."""

    def __init__(self, capfd):
        self.capfd, self.err = capfd, ""

    def readouterr(self):
        r = self.capfd.readouterr()
        self.err += r.err
        return r

    def disabled(self):
        return self.capfd.disabled()


def _forms(err):
    return [int(m.group(1)) for m in FORM_LINE.finditer(err)]


def _decode_into(uhdr, scan, outs, w, h, sampling):
    """uhdr.huffman_decode into tensors the caller allocated."""
    data = _dev(scan)
    sc = uhdr._scan(outs, w, h, sampling, 0)
    uhdr._call(True, uhdr.lib.uhdr_hip_huffman_decode_dev, uhdr.ctx.handle, C.byref(sc), None, C.c_void_p(data.data_ptr()), data.numel())


def _pin(monkeypatch, sub_bits):
    monkeypatch.setenv("UHDR_HIP_HUFF_DEBUG", "1")
    monkeypatch.setenv("UHDR_HIP_HUFF_SUB_BITS", str(sub_bits))
    monkeypatch.setenv("UHDR_HIP_HUFF_MAIN_LEVELS", "1")


@pytest.mark.parametrize("sub_bits", [512, 1024])  # one piece / four pieces, start states from the notes
@pytest.mark.parametrize("quality", [95, 100])
@pytest.mark.parametrize("name", ["444", "400"])
def test_form3_gives_back_the_coefficients(uhdr, monkeypatch, capfd, name, quality, sub_bits):
    tee = _Tee(capfd)
    decode_with_stragglers(uhdr, monkeypatch, tee, name, quality, sub_bits, 1)  # (asserts equality and exactly one attempt)
    assert _forms(tee.err) == [3], tee.err


@pytest.mark.parametrize("sub_bits", [512, 1024])
@pytest.mark.parametrize("quality", [95, 100])
@pytest.mark.parametrize("name", ["444", "400"])
def test_form2_still_works(uhdr, monkeypatch, capfd, name, quality, sub_bits):
    monkeypatch.setenv("UHDR_HIP_HUFF_WRITE", "2")
    tee = _Tee(capfd)
    decode_with_stragglers(uhdr, monkeypatch, tee, name, quality, sub_bits, 1)
    assert _forms(tee.err) == [2], tee.err


OW, OH = 248, 216  # 31 x 27 blocks


@functools.lru_cache(maxsize=None)
def _odd_case():
    rng = np.random.default_rng(4711)
    bw, bh = OW // 8, OH // 8
    coefs = []
    for c in range(3):
        yy, xx = np.mgrid[0:OH, 0:OW]
        amp = 0.3 + 7.0 * (0.5 + 0.5 * np.sin(xx / 23.0 + c) * np.cos(yy / 17.0)) ** 2
        pl = 128 + 70 * np.sin(xx / (29.0 + 5 * c)) * np.cos(yy / (21.0 + 3 * c)) + rng.normal(0, 1, (OH, OW)) * amp
        qt = L.quant_table_port(95, c > 0)
        coefs.append(L.fdct_quant_port(np.ascontiguousarray(np.clip(np.rint(pl), 0, 255).astype(np.uint8)), OW, bw, bh, qt))
    scan = L.huffman_encode_port(coefs, OW, OH, SAMPLINGS["444"], 0)
    assert len(scan) >= 4096, len(scan)  # the parallel route's threshold
    assert (bw * bh * 3) % 256 != 0 and bw % 2 == 1 and bh % 2 == 1
    return coefs, scan


def test_odd_block_grid(uhdr, monkeypatch, capfd):
    """31 x 27 blocks: JBLOCK numbers cross row ends at odd places, and the last DC chunk holds 207 of 256 scan positions."""
    import torch

    coefs, scan = _odd_case()
    _pin(monkeypatch, 512)
    outs = [torch.full(c.shape, 0x5a5a, dtype=torch.int16, device="cuda:0") for c in coefs]
    capfd.readouterr()
    before = _parallel(uhdr)
    _decode_into(uhdr, scan, outs, OW, OH, SAMPLINGS["444"])
    err = capfd.readouterr().err
    assert _parallel(uhdr) == before + 1
    assert _forms(err) == [3], err
    for c in range(3):
        assert np.array_equal(outs[c].cpu().numpy(), coefs[c]), c


def test_short_last_subsequence(uhdr, monkeypatch, capfd):
    tee = _Tee(capfd)
    decode_with_stragglers(uhdr, monkeypatch, tee, "444", 95, 512, 1, short_tail=True)
    assert _forms(tee.err) == [3], tee.err


def test_lost_first_attempt_leaves_nothing_behind(uhdr, monkeypatch, capfd):
    """q100, full-scale noise: the pinned attempt loses the true path (tests/test_gpu_huffman_straggler.py's docstring), so its write pass
    ran from wrong start states and stored garbage into the component arrays.  The rounds that follow store into zero-initialised
    arrays: every term the lost attempt touched, the many that are coded as zero among them, must be what was coded."""
    import torch

    coefs, scan = _case("444", 100, False, 1.0)
    _pin(monkeypatch, 512)
    outs = [torch.full(c.shape, 0x5a5a, dtype=torch.int16, device="cuda:0") for c in coefs]
    capfd.readouterr()
    before = _parallel(uhdr)
    _decode_into(uhdr, scan, outs, 256, 256, SAMPLINGS["444"])
    err = capfd.readouterr().err
    attempts = [ln for ln in err.splitlines() if "paths handed to the straggler waves" in ln or ROUNDS_LINE.search(ln)]
    with capfd.disabled():
        print("\n" + " | ".join(attempts))
    assert len(attempts) == 2, err
    assert "true path LOST" in attempts[0], attempts[0]
    assert _forms(err) == [3], err
    m = ROUNDS_LINE.search(attempts[1])
    assert m and m.group(2) == "settled", attempts[1]
    assert _parallel(uhdr) == before + 1
    for c in range(3):
        assert np.array_equal(outs[c].cpu().numpy(), coefs[c]), c


@pytest.mark.parametrize("name", ["420", "422"])
def test_subsampled_scans_keep_form2(uhdr, monkeypatch, capfd, name):
    tee = _Tee(capfd)
    decode_with_stragglers(uhdr, monkeypatch, tee, name, 95, 512, 1)
    assert _forms(tee.err) == [2], tee.err


def test_three_separate_allocations(uhdr, monkeypatch, capfd):
    """The component arrays need not be contiguous: three tensors with guard tensors in between (and in front and behind), which the
    decode must leave as they are."""
    import torch

    coefs, scan = _case("444", 95)
    _pin(monkeypatch, 512)
    outs, guards = [], [torch.full((1000,), 0x1234, dtype=torch.int16, device="cuda:0")]
    for c in coefs:
        outs.append(torch.full(c.shape, 0x5a5a, dtype=torch.int16, device="cuda:0"))
        guards.append(torch.full((1000 + 8 * len(guards),), 0x1234, dtype=torch.int16, device="cuda:0"))
    assert len({o.data_ptr() for o in outs}) == 3 and all(o.data_ptr() % 16 == 0 for o in outs)
    assert outs[1].data_ptr() != outs[0].data_ptr() + outs[0].numel() * 2 or outs[2].data_ptr() != outs[1].data_ptr() + outs[1].numel() * 2
    capfd.readouterr()
    _decode_into(uhdr, scan, outs, 256, 256, SAMPLINGS["444"])
    err = capfd.readouterr().err
    assert _forms(err) == [3], err
    for c in range(3):
        assert np.array_equal(outs[c].cpu().numpy(), coefs[c]), c
    for g in guards:
        assert bool((g == 0x1234).all())
