"""The definition of vp8hip_frames_coef_async (include/vp8hip.h) a second time, in numpy: from the dense IR of a frame (mbs uint8
[nmb, 64] = vp8ir_mb records, coef int16 [nmb, 400] = 25 blocks of 16, column-major inside a block, and the frame header) to the
tensor the call writes.  The factors, the inverse WHT and the int16 wrap are residual_reference.py's, which test_residual_cpu.py
pins to the oracle.  Nothing here knows how the kernel goes about it, and the product never loads this file."""
import numpy as np

import residual_reference as R
from tensor_reference import DTYPES, convert

STAGES = {"dequant": 0, "levels": 1}
LAYOUTS = {"channels": 0, "inplace": 1}
ORDERS = {"raster": 0, "zigzag": 1}
PLANES = ("y", "u", "v", "y2")                   # bit order = plane order
CELLS = {"y": 4, "u": 2, "v": 2, "y2": 1}        # blocks of a macroblock each way
FIRST = {"y": 0, "u": 16, "v": 20, "y2": 24}     # a plane's first block
# vp8_default_zig_zag1d (vp8/common/entropy.c; RFC 6386 section 13): scan position j is block position ZIGZAG[j] = 4 * v + u
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)


def block_kinds(mbs):
    """vp8ir_block_kind (include/vp8_ir.h) for the 25 blocks of every macroblock: 0 nothing, 1 its first coefficient alone, 2 sixteen"""
    mbs = np.asarray(mbs).reshape(-1, 64)
    y_mode = mbs[:, R.O_Y_MODE]
    has_y2 = (y_mode != R.B_PRED) & (y_mode != R.SPLITMV)
    eobs = mbs[:, R.O_EOBS:R.O_EOBS + 25].astype(np.int64)
    kind = np.where(eobs > 1, 2, np.where(eobs == 1, 1, 0))
    kind[:, :16] = np.where(has_y2[:, None] & (eobs[:, :16] == 1), 0, kind[:, :16])
    kind[:, 24] = np.where(has_y2, kind[:, 24], 0)
    kind[(mbs[:, R.O_FLAGS] & R.MB_SKIP) != 0] = 0
    return kind, has_y2


def coef_blocks(hdr, mbs, coef, stage):
    """-> int64 [nmb, 25, 4, 4] (v, u): blocks 0..15 Y, 16..19 U, 20..23 V, 24 Y2, every value an int16's"""
    nmb = hdr.mb_rows * hdr.mb_cols
    mbs = np.asarray(mbs).reshape(nmb, 64)
    q = np.asarray(coef, np.int64).reshape(nmb, 25, 4, 4).transpose(0, 1, 3, 2).copy()   # [mb, block, v, u]
    kind, has_y2 = block_kinds(mbs)
    lone = q.copy()
    lone.reshape(nmb, 25, 16)[:, :, 1:] = 0
    lv = np.where((kind == 2)[:, :, None, None], q, np.where((kind == 1)[:, :, None, None], lone, 0))
    lv[:, :16, 0, 0] = np.where(has_y2[:, None], 0, lv[:, :16, 0, 0])                   # its DC is not coded there
    if stage == "levels":
        return lv
    assert stage == "dequant"
    f = R.factors(hdr)[mbs[:, R.O_SEGMENT] & 3]                                         # [nmb, 6]: y1dc y1ac y2dc y2ac uvdc uvac
    fac = np.empty((nmb, 25, 4, 4), np.int64)
    for blocks, dc, ac in ((slice(0, 16), 0, 1), (slice(16, 24), 4, 5), (slice(24, 25), 2, 3)):
        fac[:, blocks] = f[:, ac][:, None, None, None]
        fac[:, blocks, 0, 0] = f[:, dc][:, None]
    dq = R.s16(lv * fac)                                                                # vp8_dequantize_b_c
    # the luma DCs of a macroblock with a Y2 block: vp8_short_inv_walsh4x4_c of its dequantised Y2 block, _1_c with eob <= 1
    eob24 = mbs[:, R.O_EOBS + 24].astype(np.int64)
    wht = R.inv_walsh(dq[:, 24]).reshape(nmb, 16)
    a1 = R.s16((dq[:, 24, 0, 0] + 3) >> 3)
    dcs = np.where((eob24 > 1)[:, None], wht, a1[:, None])
    live = has_y2 & ((mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0)
    dq[:, :16, 0, 0] = np.where(live[:, None], dcs, dq[:, :16, 0, 0])
    return dq


def size(hdr, layout="channels", planes=PLANES[:3], nfreq=16, dtype="i16"):
    n = 16 if layout == "inplace" else nfreq
    return sum(n * CELLS[p] ** 2 for p in PLANES if p in planes) * hdr.mb_rows * hdr.mb_cols * np.dtype(DTYPES[dtype]).itemsize


def plane_channels(blocks, hdr, plane):
    """blocks (coef_blocks) -> the plane as [16, G * mb_rows, G * mb_cols]: channel 4 * v + u of every block"""
    rows, cols, g = hdr.mb_rows, hdr.mb_cols, CELLS[plane]
    b = blocks[:, FIRST[plane]:FIRST[plane] + g * g].reshape(rows, cols, g, g, 16)      # [mb row, mb col, block row, block col, 4v + u]
    return b.transpose(4, 0, 2, 1, 3).reshape(16, g * rows, g * cols)


def arrange(blocks, hdr, layout="channels", planes=PLANES[:3], nfreq=16, order="raster", dtype="i16", scale=(1.0, 1.0, 1.0, 1.0)):
    """blocks (coef_blocks) -> {plane: array} as the tensor holds them, and the tensor itself, flat: (views, flat)"""
    views = {}
    for k, p in enumerate(PLANES):
        if p not in planes:
            continue
        ch = plane_channels(blocks, hdr, p)
        if layout == "inplace":
            g, rows, cols = CELLS[p], hdr.mb_rows, hdr.mb_cols
            a = ch.reshape(4, 4, g * rows, g * cols).transpose(2, 0, 3, 1).reshape(4 * g * rows, 4 * g * cols)
        else:
            a = ch[[ZIGZAG[j] if order == "zigzag" else j for j in range(nfreq)]]
        views[p] = convert(a, dtype, scale[k])
    return views, np.concatenate([v.ravel() for v in views.values()])
