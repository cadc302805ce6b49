"""Checker code (numpy) for the 4:2:2 -> RGB decode: how each libjpeg family rebuilds the chroma planes of a 2x1 / 1x1 / 1x1
file.  The companion of tests/upsample_port.py (4:2:0), which supplies the 16-point pass.

variant 0, libjpeg-turbo 3.1 (jdsample.c): every chroma block goes through the 8x8 islow IDCT; h2v1_fancy_upsample then
makes each chroma sample two output samples of the same row, (3 * this + left + 1) >> 2 and (3 * this + right + 2) >> 2.
The first output of a row is c[0] and the last c[cw - 1], cw = ceil(w/2): the same as clamping the neighbour's index to the
real samples.  No vertical mixing.  turbo takes plain replication (h2v1_upsample) when cw <= 2.

variant 1, IJG libjpeg 9 (jdmaster.c / jidctint.c): with do_fancy_upsampling the chroma is not upsampled at all; each 8x8
chroma block is rebuilt as 16 wide x 8 high samples by jpeg_idct_16x8 and the upsampler is 1:1.  Pass 1 over the columns is
the ordinary 8-point islow pass (CONST_BITS 13, PASS1_BITS 2) on INT32 = long, exact in 64 bits, its results stored as
int; pass 2 over each of the 8 rows is the 16-point pass of jpeg_idct_16x16 (upsample_port._idct16_1d, pass1=False), whose
range-limit index keeps bits 18..27.

Both families convert with ycc_rgb_convert (oracle.loader.jpeg_ycc_to_rgb_port, variant 0 / 1)."""
import numpy as np

from oracle import loader as L
from upsample_port import _idct16_1d

FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865 = 2446, 3196, 4433, 6270
FIX_0_899976223, FIX_1_175875602, FIX_1_501321110, FIX_1_847759065 = 7373, 9633, 12299, 15137
FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026 = 16069, 16819, 20995, 25172


def _idct8_columns(x):
    """jidctint.c's 8-point islow column pass on a list of 8 int64 arrays -> 8 int64 arrays before the shift by 11."""
    z2, z3 = x[0] << 13, x[4] << 13
    z2 = z2 + (1 << 10)  # the fudge factor of the final descale
    tmp0, tmp1 = z2 + z3, z2 - z3
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * FIX_0_541196100
    tmp2 = z1 + z2 * FIX_0_765366865
    tmp3 = z1 - z3 * FIX_1_847759065
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp2, tmp0 - tmp2, tmp1 + tmp3, tmp1 - tmp3
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z2 = tmp0 + tmp2
    z3 = tmp1 + tmp3
    z1 = (z2 + z3) * FIX_1_175875602
    z2 = z2 * -FIX_1_961570560 + z1
    z3 = z3 * -FIX_0_390180644 + z1
    z1 = (tmp0 + tmp3) * -FIX_0_899976223
    tmp0 = tmp0 * FIX_0_298631336 + z1 + z2
    tmp3 = tmp3 * FIX_1_501321110 + z1 + z3
    z1 = (tmp1 + tmp2) * -FIX_2_562915447
    tmp1 = tmp1 * FIX_2_053119869 + z1 + z3
    tmp2 = tmp2 * FIX_3_072711026 + z1 + z2
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def idct16x8_ijg9(coef: np.ndarray, qt) -> np.ndarray:
    """(bh, bw, 64) int16 JBLOCKs -> (bh*8, bw*16) uint8 plane: IJG 9's jpeg_idct_16x8 of every block."""
    bh, bw = coef.shape[:2]
    v = coef.reshape(-1, 8, 8).astype(np.int64) * np.asarray(qt, dtype=np.int64).reshape(8, 8)
    ws = np.zeros((v.shape[0], 8, 8), dtype=np.int64)
    for c in range(8):
        o = _idct8_columns([v[:, k, c] for k in range(8)])
        for r in range(8):
            ws[:, r, c] = (o[r] >> 11).astype(np.int32)  # workspace is int
    out = np.zeros((v.shape[0], 8, 16), dtype=np.uint8)
    for r in range(8):
        o = _idct16_1d([ws[:, r, k] for k in range(8)], False)
        for k in range(16):
            out[:, r, k] = np.clip(((o[k] >> 18) & 1023) - 384, 0, 255)
    return out.reshape(bh, bw, 8, 16).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 16)


def h2v1_turbo(c: np.ndarray, w: int, h: int) -> np.ndarray:
    """Real chroma samples (h, ceil(w/2)) uint8 -> (h, w) uint8, libjpeg-turbo's 4:2:2 upsampling."""
    cw = (w + 1) // 2
    c = c[:h, :cw].astype(np.int32)
    if cw <= 2:  # h2v1_upsample
        return np.repeat(c, 2, axis=1)[:, :w].astype(np.uint8)
    left = c[:, np.clip(np.arange(cw) - 1, 0, cw - 1)]
    right = c[:, np.clip(np.arange(cw) + 1, 0, cw - 1)]
    out = np.empty((h, 2 * cw), dtype=np.int32)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :w].astype(np.uint8)


def decode422_rgb(coefs, qts, w: int, h: int, variant: int, channels: int = 3) -> np.ndarray:
    """coefs: [Y, Cb, Cr] (bh, bw, 64) int16 on libjpeg's width_in_blocks grids -- Y ceil(h/8) x ceil(w/8), chroma
    ceil(h/8) x ceil(ceil(w/2)/8) -- or larger; qts: 3 natural-order tables -> (h, w, channels) uint8, what the libjpeg
    family `variant` returns for JCS_RGB / JCS_EXT_RGBA."""
    y = L.idct_dequant_port(coefs[0], qts[0])[:h, :w]
    if variant == 0:
        cb, cr = [h2v1_turbo(L.idct_dequant_port(coefs[i], qts[i]), w, h) for i in (1, 2)]
    else:
        cb, cr = [idct16x8_ijg9(coefs[i], qts[i])[:h, :w] for i in (1, 2)]
    planes = [np.ascontiguousarray(p) for p in (y, cb, cr)]
    return L.jpeg_ycc_to_rgb_port(*planes, out_bpp=channels, variant=variant).reshape(h, w, channels)
