"""Images as views inside sentinel frames: a plain helper module (no pytest fixtures) for tests/test_route_lattice.py and
tests/test_apply_lattice.py (CPU) and tests/test_gpu_route_lattice.py / tests/test_gpu_apply_lattice.py / tests/test_gpu_tile_loops.py
(device).

framed() builds an image of a given format and size whose planes each live in a buffer of their own, filled with GUARD (0xA5):
guard rows above and below, the caller's stride per plane (in samples, as uhdr_raw_image_t counts them: pixels for the packed
formats) and the caller's byte offset of each plane's base from a 256-byte boundary.  The valid samples come from a host Image
(its top-left w x h samples, so a crop of a larger image works) or stay GUARD for a destination.  assert_frame_intact() then checks
that nothing but the samples an operator may write has changed: the guard rows, the bytes in front of the base, the stride
padding behind each row -- and, for an in-place operator, the samples the reference leaves untouched."""
import ctypes as C
from collections import namedtuple

import numpy as np

from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image, bytes_per_sample, plane_layout

GUARD = 0xA5
GUARD_ROWS = 2

# one plane inside its buffer, everything in bytes: the buffer's size, the offset of the base (sample (0, 0)), rows, the row pitch,
# the valid bytes of a row, the bytes of a sample
Plane = namedtuple("Plane", "nbytes base rows pitch width bps")

_DTYPE = {1: np.uint8, 2: np.uint16, 3: np.uint8, 4: np.uint32, 8: np.uint64}


def plane_samples(fmt, w, h):
    """[(rows, valid samples per row)] of the planes a w x h image of this format has."""
    return [(pl[0], pl[2]) for pl in plane_layout(fmt, w, h, 1) if pl is not None]


def frame_layout(fmt, w, h, strides, offsets, guard_rows=GUARD_ROWS):
    """[Plane] for strides (samples per row, per plane) and offsets (bytes of each base past a 256-byte boundary)."""
    bps = bytes_per_sample(fmt)
    geom = plane_samples(fmt, w, h)
    assert len(strides) == len(offsets) == len(geom), (fmt, strides, offsets)
    out = []
    for (rows, width), stride, off in zip(geom, strides, offsets):
        assert stride >= width, f"stride {stride} is less than the {width} samples of a row"
        assert 0 <= off < 256 and off % (1 if bps == 3 else bps) == 0, f"offset {off} does not keep {bps}-byte samples aligned"
        pitch = stride * bps
        lead = -(-(guard_rows * pitch) // 256) * 256  # whole guard rows in front of the base, and the base on a 256-byte boundary + off
        out.append(Plane(lead + off + (rows + guard_rows) * pitch, lead + off, rows, pitch, width * bps, bps))
    return out


def _rows(buf, pl, rows=None, width=None):
    """The (rows, width bytes) window of a plane inside its flat uint8 buffer, as a writable strided view."""
    rows, width = pl.rows if rows is None else rows, pl.width if width is None else width
    return np.lib.stride_tricks.as_strided(buf[pl.base:], shape=(rows, width), strides=(pl.pitch, 1), writeable=True)


class Frame:
    """raw: the uhdr_raw_image_t to hand to the C ABI.  planes: [Plane].  initial: the buffers as they were built (host copies)."""

    def __init__(self, fmt, w, h, planes, strides, initial, device):
        self.fmt, self.w, self.h, self.planes, self.strides, self.initial, self.device = fmt, w, h, planes, list(strides), initial, device
        self.bufs = []
        self.raw = A.RawImage()
        self.raw.fmt, self.raw.w, self.raw.h = fmt, w, h
        for i, (pl, host) in enumerate(zip(planes, initial)):
            if device is None:
                store = np.empty(pl.nbytes + 256, dtype=np.uint8)
                shift = (-store.ctypes.data) % 256
                view = store[shift: shift + pl.nbytes]
                view[:] = host
                ptr = view.ctypes.data
            else:
                import torch

                store = torch.empty(pl.nbytes + 256, dtype=torch.uint8, device=device)
                shift = (-store.data_ptr()) % 256
                view = store[shift: shift + pl.nbytes]
                view.copy_(torch.from_numpy(host))
                ptr = view.data_ptr()
            assert ptr % 256 == 0
            self.bufs.append(view)
            self.raw.planes[i] = ptr + pl.base
            self.raw.stride[i] = strides[i]
        if device is not None:
            import torch

            torch.cuda.current_stream(self.bufs[0].device).synchronize()  # the library works on a stream of its own

    def sync_meta_from_raw(self):  # what the wrappers of libultrahdr_amd/ultrahdr.py call on a destination
        pass

    def desc(self):
        """The descriptor fields a call may rewrite."""
        r = self.raw
        return (r.fmt, r.cg, r.ct, r.range, r.w, r.h)

    def download(self):
        return [b.copy() if self.device is None else b.cpu().numpy() for b in self.bufs]

    def valid(self, w=None, h=None, bufs=None):
        """The valid samples per plane as 2-D arrays (uint8 columns for RGB888), read back from the buffers; w, h: of a smaller image
        of the same format at the same base (the part an operator on an odd-sized 4:2:0 image writes, say)."""
        bufs = self.download() if bufs is None else bufs
        geom = plane_samples(self.fmt, self.w if w is None else w, self.h if h is None else h)
        out = []
        for buf, pl, (rows, width) in zip(bufs, self.planes, geom):
            win = np.ascontiguousarray(_rows(buf, pl, rows, width * pl.bps))
            out.append(win.view(_DTYPE[pl.bps]))
        return out


def framed(fmt, w, h, strides, offsets, src=None, device="cuda:0", guard_rows=GUARD_ROWS, cg=None, ct=None, rng=None):
    """A Frame of a w x h image of `fmt`; src: the host Image (same format, at least w x h) whose samples fill it, None for a
    destination (all GUARD).  The colour description comes from src unless given."""
    planes = frame_layout(fmt, w, h, strides, offsets, guard_rows)
    initial = [np.full(pl.nbytes, GUARD, dtype=np.uint8) for pl in planes]
    if src is not None:
        assert src.fmt == fmt and src.w >= w and src.h >= h and src.device is None
        present = [i for i, pl in enumerate(src.layout) if pl is not None]
        for buf, pl, i in zip(initial, planes, present):
            rows_src = src.plane(i).view(np.uint8).reshape(src.layout[i][0], -1)
            _rows(buf, pl)[:] = rows_src[: pl.rows, : pl.width]
    fr = Frame(fmt, w, h, planes, strides, initial, device)
    fr.raw.cg = (src.raw.cg if src is not None else A.UHDR_CG_UNSPECIFIED) if cg is None else cg
    fr.raw.ct = (src.raw.ct if src is not None else A.UHDR_CT_UNSPECIFIED) if ct is None else ct
    fr.raw.range = (src.raw.range if src is not None else A.UHDR_CR_UNSPECIFIED) if rng is None else rng
    return fr


def tight(fmt, w, h, src):
    """A host Image of the top-left w x h samples of src with the smallest even strides (what the oracle is run on; even, because
    the interleaved chroma rows of an odd-width P010 image hold w + 1 samples)."""
    out = Image(fmt, w, h, src.raw.cg, src.raw.ct, src.raw.range, align=2)
    present = [i for i, pl in enumerate(src.layout) if pl is not None]
    for i, (rows, width) in zip(present, plane_samples(fmt, w, h)):
        k = 3 if bytes_per_sample(fmt) == 3 else 1
        out.plane(i)[:rows, : width * k] = src.plane(i)[:rows, : width * k]
    return out


def stripe(frame, row0, rows):
    """The uhdr_raw_image_t of rows [row0, row0 + rows) of a Frame: a view inside the same buffers, as a caller that shards an image
    by rows hands it over (row0 and rows even for a format with subsampled chroma rows)."""
    r = A.RawImage()
    C.memmove(C.byref(r), C.byref(frame.raw), C.sizeof(A.RawImage))
    r.h = rows
    for i, pl in enumerate(frame.planes):
        k = frame.h // pl.rows if pl.rows else 1  # luma rows per row of this plane
        assert row0 % k == 0 and rows % k == 0 and row0 + rows <= frame.h, (row0, rows, k)
        r.planes[i] = frame.raw.planes[i] + (row0 // k) * pl.pitch
    return r


def assert_frame_intact(frame, written=None, what="", rows=None):
    """Every byte of every buffer of `frame` still holds what it was built with, except the samples an operator may write: all
    valid samples (written=None, a destination), none (written=(), an input), or the top-left (w, h) image of the same format
    (an in-place operator that leaves the last column / row of an odd-sized subsampled image alone).  Outside the valid samples
    that means GUARD: the guard rows, the bytes in front of the base, the padding behind each row.  rows=(row0, n): the writable
    samples are those of rows [row0, row0 + n) only (a destination handed over as a stripe()), at their full width."""
    now = frame.download()
    first = [0] * len(frame.planes)
    if rows is not None:
        assert written is None
        geom = plane_samples(frame.fmt, frame.w, rows[1])
        first = [rows[0] // (frame.h // pl.rows) * pl.pitch for pl in frame.planes]
    elif written is None:
        geom = plane_samples(frame.fmt, frame.w, frame.h)
    elif len(written) == 0:
        geom = [(0, 0)] * len(frame.planes)
    else:
        geom = plane_samples(frame.fmt, *written)
    for i, (buf, was, pl, (rows, width)) in enumerate(zip(now, frame.initial, frame.planes, geom)):
        keep = np.ones(pl.nbytes, dtype=bool)
        if rows and width:
            _rows(keep[first[i]:], pl, rows, width * pl.bps)[:] = False
        bad = np.flatnonzero(keep & (buf != was))
        if bad.size:
            off = int(bad[0]) - pl.base
            raise AssertionError(f"{what}: plane {i}: {bad.size} bytes outside the writable samples changed; the first at byte {off} from the base "
                                 f"(row {off // pl.pitch if off >= 0 else off / pl.pitch:.0f}, byte {off % pl.pitch} of a {pl.pitch}-byte pitch, "
                                 f"{pl.width} valid): 0x{int(was[bad[0]]):02x} -> 0x{int(buf[bad[0]]):02x}")


def view_inside_frame(frame):
    """CPU check of the construction itself: every plane's view, guard rows included, lies inside its buffer, and the base sits at
    its offset from a 256-byte boundary."""
    for i, pl in enumerate(frame.planes):
        if pl.base < GUARD_ROWS * pl.pitch or pl.base + (pl.rows - 1) * pl.pitch + pl.width + GUARD_ROWS * pl.pitch > pl.nbytes:
            return False
        ptr = frame.raw.planes[i]
        first = frame.bufs[i].ctypes.data if frame.device is None else frame.bufs[i].data_ptr()
        if ptr != first + pl.base or first % 256:
            return False
    return True
