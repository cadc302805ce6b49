"""numpy restatement of the reference's resize_image (lib/src/editorhelper.cpp:88-146) for the three gain-map formats, the same kind
of thing as upsample_port.py: what uhdr_hip_resize_image and the resizing sampler of the applyGainMap kernel must reproduce byte for
byte.  Pinned to the real reference by tests/test_resize_port.py.

For destination pixel (x, y):
    ori_x = x * (src_w / dst_w), ori_y = y * (src_h / dst_h)                      float64
    p0 = (floor(ori_x), floor(ori_y)) clipped to the source; p1 right of p0, p2 below p0, p3 right of p2, clipped to the last
    column / row
    t = ori_x - p0.x; the vertical position takes no part in the weights
    w0 = (1-t)(1-t)(1-t), w1 = 3t(1-t)(1-t), w2 = 3tt(1-t), w3 = ttt              float64, products left to right
    v = float32(((w0*p0 + w1*p1) + w2*p2) + w3*p3)                               samples float32, widened
    byte = trunc(clip(v * 255.0f + 0.5f, 0, 255))                                float32; alpha 255 for RGBA8888
A sample is get_pixel's float32: byte * (1 / 255.0f) for Y400 (getYuv400Pixel), byte / 255.0f for RGB888 and RGBA8888
(getRgb888Pixel, getRgba8888Pixel) -- the two differ in the last bit for some bytes."""
import numpy as np

from libultrahdr_amd import capi as A
from libultrahdr_amd.images import Image

_F32 = np.float32
_BPP = {A.UHDR_IMG_FMT_8bppYCbCr400: 1, A.UHDR_IMG_FMT_24bppRGB888: 3, A.UHDR_IMG_FMT_32bppRGBA8888: 4}


def sample_table(fmt):
    """get_pixel's float32 for every byte of a map of this format."""
    b = np.arange(256, dtype=_F32)
    return b * (_F32(1) / _F32(255)) if fmt == A.UHDR_IMG_FMT_8bppYCbCr400 else b / _F32(255)


def resize_channels(src, fmt, dst_w, dst_h, y0=0, rows=None):
    """src: uint8 [src_h, src_w, nch] -> uint8 [rows, dst_w, nch], rows y0 .. y0 + rows of the dst_w x dst_h result."""
    src_h, src_w = src.shape[:2]
    rows = dst_h - y0 if rows is None else rows
    scale_x, scale_y = np.float64(src_w) / np.float64(dst_w), np.float64(src_h) / np.float64(dst_h)
    ori_x = np.arange(dst_w, dtype=np.float64) * scale_x
    ori_y = np.arange(y0, y0 + rows, dtype=np.float64) * scale_y
    x0 = np.clip(np.floor(ori_x).astype(np.int64), 0, src_w - 1)
    yl = np.clip(np.floor(ori_y).astype(np.int64), 0, src_h - 1)
    x1, yh = np.minimum(x0 + 1, src_w - 1), np.minimum(yl + 1, src_h - 1)
    t = ori_x - x0
    u = 1 - t
    w0, w1, w2, w3 = u * u * u, 3 * t * u * u, 3 * t * t * u, t * t * t
    f = sample_table(fmt)[src].astype(np.float64)  # [src_h, src_w, nch]
    wv = lambda w: w[None, :, None]
    p0, p1 = f[yl][:, x0], f[yl][:, x1]
    p2, p3 = f[yh][:, x0], f[yh][:, x1]
    v = (((wv(w0) * p0 + wv(w1) * p1) + wv(w2) * p2) + wv(w3) * p3).astype(_F32)
    v = v * _F32(255)
    v = v + _F32(0.5)
    return np.clip(v, _F32(0), _F32(255)).astype(np.int32).astype(np.uint8)


def channels_of(img: Image):
    """The colour channels of a host Y400 / RGB888 / RGBA8888 image: uint8 [h, w, nch]."""
    bpp = _BPP[img.fmt]
    v = img.valid(0)
    if bpp == 1:
        return v[:, :, None].copy()
    if bpp == 3:
        return v.reshape(img.h, img.w, 3).copy()
    return np.ascontiguousarray(v).view(np.uint8).reshape(img.h, img.w, 4)[:, :, :3].copy()


def put_channels(img: Image, ch):
    bpp = _BPP[img.fmt]
    if bpp == 1:
        img.valid(0)[:] = ch[:, :, 0]
    elif bpp == 3:
        img.valid(0)[:] = ch.reshape(img.h, img.w * 3)
    else:
        c = ch.astype(np.uint32)
        img.valid(0)[:] = c[:, :, 0] | (c[:, :, 1] << 8) | (c[:, :, 2] << 16) | (np.uint32(255) << 24)


def resize_image(src: Image, dst_w, dst_h, align=64) -> Image:
    """resize_image(src, dst_w, dst_h) on a host image: a new image of the same format and colour aspects."""
    dst = Image(src.fmt, dst_w, dst_h, src.raw.cg, src.raw.ct, src.raw.range, align)
    put_channels(dst, resize_channels(channels_of(src), src.fmt, dst_w, dst_h))
    return dst


def needs_resize(base_w, base_h, map_w, map_h):
    """The reference's decision (jpegr.cpp:1653-1658) in float32, as written there."""
    pa = _F32(base_w) / _F32(base_h)
    ga = _F32(map_w) / _F32(map_h)
    return bool(np.abs(pa - ga) / pa > _F32(0.01))
