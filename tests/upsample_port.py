"""Checker code (numpy) for the 4:2:0 -> RGB decode: how each libjpeg family rebuilds the chroma planes.

variant 0, libjpeg-turbo 3.1 (jdsample.c): every chroma block goes through the 8x8 islow IDCT; h2v2_fancy_upsample
then makes each chroma sample 2x2 output samples.  Vertical step colsum = 3 * near + far (far: the chroma row above for
the upper output row, below for the lower one); horizontal step (3 * this + left + 8) >> 4 and (3 * this + right + 7)
>> 4.  The context rows and columns replicate the last REAL chroma row / column (ceil(h/2) - 1, ceil(w/2) - 1), which is
the same as clamping the neighbour's index.  turbo takes plain 2x2 replication (h2v2_upsample) when ceil(w/2) <= 2.

variant 1, IJG libjpeg 9 (jdmaster.c / jidctint.c): with do_fancy_upsampling the chroma is not upsampled at all; each
8x8 chroma block is rebuilt as 16x16 samples by the scaled islow IDCT jpeg_idct_16x16 and the upsampler is 1:1.  Its
arithmetic is integer (CONST_BITS 13, PASS1_BITS 2) on INT32 = long: pass 1 is exact in 64 bits and its results are
stored as int; pass 2's range-limit index keeps bits 18..27, which any wrap-around arithmetic reproduces.

Both families convert with ycc_rgb_convert (oracle.loader.jpeg_ycc_to_rgb_port, variant 0 / 1)."""
import numpy as np

from oracle import loader as L


def _fix(x: float) -> int:
    return int(x * (1 << 13) + 0.5)


def _idct16_1d(x, pass1: bool):
    """One 16-point pass of jpeg_idct_16x16 on a list of 8 int64 arrays -> 16 int64 arrays before the final shift."""
    if pass1:
        tmp0 = (x[0] << 13) + (1 << 10)
    else:
        tmp0 = (x[0] + ((512 << 5) + (1 << 4))) << 13  # RANGE_CENTER << (PASS1_BITS + 3), rounding 1 << (PASS1_BITS + 2)
    z1 = x[4]
    tmp1 = z1 * _fix(1.306562965)
    tmp2 = z1 * _fix(0.541196100)
    tmp10, tmp11, tmp12, tmp13 = tmp0 + tmp1, tmp0 - tmp1, tmp0 + tmp2, tmp0 - tmp2
    z1, z2 = x[2], x[6]
    z3 = z1 - z2
    z4 = z3 * _fix(0.275899379)
    z3 = z3 * _fix(1.387039845)
    tmp0 = z3 + z2 * _fix(2.562915447)
    tmp1 = z4 + z1 * _fix(0.899976223)
    tmp2 = z3 - z1 * _fix(0.601344887)
    tmp3 = z4 - z2 * _fix(0.509795579)
    tmp20, tmp27 = tmp10 + tmp0, tmp10 - tmp0
    tmp21, tmp26 = tmp12 + tmp1, tmp12 - tmp1
    tmp22, tmp25 = tmp13 + tmp2, tmp13 - tmp2
    tmp23, tmp24 = tmp11 + tmp3, tmp11 - tmp3
    z1, z2, z3, z4 = x[1], x[3], x[5], x[7]
    tmp11 = z1 + z3
    tmp1 = (z1 + z2) * _fix(1.353318001)
    tmp2 = tmp11 * _fix(1.247225013)
    tmp3 = (z1 + z4) * _fix(1.093201867)
    tmp10 = (z1 - z4) * _fix(0.897167586)
    tmp11 = tmp11 * _fix(0.666655658)
    tmp12 = (z1 - z2) * _fix(0.410524528)
    tmp0 = tmp1 + tmp2 + tmp3 - z1 * _fix(2.286341144)
    tmp13 = tmp10 + tmp11 + tmp12 - z1 * _fix(1.835730603)
    z1 = (z2 + z3) * _fix(0.138617169)
    tmp1 = tmp1 + z1 + z2 * _fix(0.071888074)
    tmp2 = tmp2 + z1 - z3 * _fix(1.125726048)
    z1 = (z3 - z2) * _fix(1.407403738)
    tmp11 = tmp11 + z1 - z3 * _fix(0.766367282)
    tmp12 = tmp12 + z1 + z2 * _fix(1.971951411)
    z2 = z2 + z4
    z1 = z2 * -_fix(0.666655658)
    tmp1 = tmp1 + z1
    tmp3 = tmp3 + z1 + z4 * _fix(1.065388962)
    z2 = z2 * -_fix(1.247225013)
    tmp10 = tmp10 + z2 + z4 * _fix(3.141271809)
    tmp12 = tmp12 + z2
    z2 = (z3 + z4) * -_fix(1.353318001)
    tmp2 = tmp2 + z2
    tmp3 = tmp3 + z2
    z2 = (z4 - z3) * _fix(0.410524528)
    tmp10 = tmp10 + z2
    tmp11 = tmp11 + z2
    out = [None] * 16
    for k, (e, o) in enumerate(((tmp20, tmp0), (tmp21, tmp1), (tmp22, tmp2), (tmp23, tmp3),
                                (tmp24, tmp10), (tmp25, tmp11), (tmp26, tmp12), (tmp27, tmp13))):
        out[k], out[15 - k] = e + o, e - o
    return out


def idct16_ijg9(coef: np.ndarray, qt) -> np.ndarray:
    """(bh, bw, 64) int16 JBLOCKs -> (bh*16, bw*16) uint8 plane: IJG 9's jpeg_idct_16x16 of every block."""
    bh, bw = coef.shape[:2]
    v = coef.reshape(-1, 8, 8).astype(np.int64) * np.asarray(qt, dtype=np.int64).reshape(8, 8)
    ws = np.zeros((v.shape[0], 16, 8), dtype=np.int64)
    for c in range(8):
        o = _idct16_1d([v[:, k, c] for k in range(8)], True)
        for r in range(16):
            ws[:, r, c] = (o[r] >> 11).astype(np.int32)  # workspace is int
    out = np.zeros((v.shape[0], 16, 16), dtype=np.uint8)
    for r in range(16):
        o = _idct16_1d([ws[:, r, k] for k in range(8)], False)
        for k in range(16):
            t = (o[k] >> 18) & 1023
            out[:, r, k] = np.clip(t - 384, 0, 255)
    return out.reshape(bh, bw, 16, 16).transpose(0, 2, 1, 3).reshape(bh * 16, bw * 16)


def h2v2_turbo(c: np.ndarray, w: int, h: int) -> np.ndarray:
    """Real chroma samples (ceil(h/2), ceil(w/2)) uint8 -> (h, w) uint8, libjpeg-turbo's 4:2:0 upsampling."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    c = c[:ch, :cw].astype(np.int32)
    if cw <= 2:  # h2v2_upsample
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w].astype(np.uint8)
    rows = np.arange(2 * ch)
    near = c[rows >> 1]
    far = c[np.clip((rows >> 1) + np.where(rows & 1, 1, -1), 0, ch - 1)]
    colsum = 3 * near + far
    left = colsum[:, np.clip(np.arange(cw) - 1, 0, cw - 1)]
    right = colsum[:, np.clip(np.arange(cw) + 1, 0, cw - 1)]
    out = np.empty((2 * ch, 2 * cw), dtype=np.int32)
    out[:, 0::2] = (3 * colsum + left + 8) >> 4
    out[:, 1::2] = (3 * colsum + right + 7) >> 4
    return out[:h, :w].astype(np.uint8)


def decode420_rgb(coefs, qts, w: int, h: int, variant: int, channels: int = 3) -> np.ndarray:
    """coefs: [Y, Cb, Cr] (bh, bw, 64) int16 (libjpeg's width_in_blocks grids or larger); qts: 3 natural-order tables
    -> (h, w, channels) uint8, what the libjpeg family `variant` returns for JCS_RGB / JCS_EXT_RGBA."""
    y = L.idct_dequant_port(coefs[0], qts[0])[:h, :w]
    if variant == 0:
        cb, cr = [h2v2_turbo(L.idct_dequant_port(coefs[i], qts[i]), w, h) for i in (1, 2)]
    else:
        cb, cr = [idct16_ijg9(coefs[i], qts[i])[:h, :w] for i in (1, 2)]
    planes = [np.ascontiguousarray(p) for p in (y, cb, cr)]
    return L.jpeg_ycc_to_rgb_port(*planes, out_bpp=channels, variant=variant).reshape(h, w, channels)
