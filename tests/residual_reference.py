"""The definition of vp8hip_frames_residual_async (include/vp8hip.h) a second time, in numpy: from the dense IR of a frame (mbs uint8
[nmb, 64] = vp8ir_mb records, coef int16 [nmb, 400] = 25 blocks of 16, column-major inside a block, and the frame header) to the
tensor the call writes.  Every `short` of the reference's C is a wrap to int16 here (s16), every `int` a wide integer.  Nothing here
knows how the kernel goes about it, and the product never loads this file."""
import numpy as np

from tensor_reference import DTYPES, convert, grid_map  # noqa: F401  (the tensor's types; its values; the sample map)

LAYOUTS = {"i420": 0, "planar": 1}
B_PRED, SPLITMV = 4, 9
MB_SKIP = 1
# byte offsets in a vp8ir_mb record (include/vp8_ir.h)
O_Y_MODE, O_REF, O_FLAGS, O_SEGMENT, O_EOBS = 0, 2, 3, 4, 8

# dc_qlookup / ac_qlookup (vp8/common/quant_common.c:14-37; RFC 6386 section 14.1)
DC_Q = np.array([
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17, 18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26,
    27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 46, 47, 48, 49, 50, 51, 52,
    53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79,
    80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116,
    118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157], np.int64)
AC_Q = np.array([
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33,
    34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 60, 62, 64,
    66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 100, 102, 104, 106, 108, 110, 112, 114, 116,
    119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152, 155, 158, 161, 164, 167, 170, 173, 177, 181, 185,
    189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284], np.int64)


def s16(x):
    """what a C `short` keeps of an int"""
    return ((np.asarray(x, np.int64) + 32768) & 0xffff) - 32768


def keep(x):
    """s16's stand-in when the truncations are switched off (residual_planes(wrap=False))"""
    return np.asarray(x, np.int64)


def factors(hdr):
    """int64 [4, 6]: y1dc, y1ac, y2dc, y2ac, uvdc, uvac of each segment (vp8cx_init_de_quantizer, mb_init_dequantizer:
    vp8/decoder/decodframe.c:50-109)"""
    out = np.zeros((4, 6), np.int64)

    def qi(v):
        return min(max(v, 0), 127)
    for s in range(4):
        q = int(hdr.base_qindex)
        if hdr.segmentation_enabled:
            q = int(hdr.segment_quant[s]) if hdr.mb_segment_abs_delta else q + int(hdr.segment_quant[s])
        q = qi(q)
        out[s] = (DC_Q[qi(q + hdr.y1dc_delta_q)], AC_Q[q], DC_Q[qi(q + hdr.y2dc_delta_q)] * 2,
                  max(AC_Q[qi(q + hdr.y2ac_delta_q)] * 155 // 100, 8), min(DC_Q[qi(q + hdr.uvdc_delta_q)], 132), AC_Q[qi(q + hdr.uvac_delta_q)])
    return out


def inv_walsh(y2, trunc=s16):
    """vp8_short_inv_walsh4x4_c (vp8/common/idctllm.c:140-192) on dequantised blocks [..., 4, 4] (row, col) -> the sixteen DCs
    [..., 4, 4]: block 4 * r + c at [r, c]"""
    a, b = y2[..., 0, :] + y2[..., 3, :], y2[..., 1, :] + y2[..., 2, :]
    c, d = y2[..., 1, :] - y2[..., 2, :], y2[..., 0, :] - y2[..., 3, :]
    t = trunc(np.stack([a + b, c + d, a - b, d - c], -2))             # `short output[16]`
    a, b = t[..., 0] + t[..., 3], t[..., 1] + t[..., 2]
    c, d = t[..., 1] - t[..., 2], t[..., 0] - t[..., 3]
    return trunc(np.stack([(a + b + 3) >> 3, (c + d + 3) >> 3, (a - b + 3) >> 3, (d - c + 3) >> 3], -1))


def _idct_pass(i0, i1, i2, i3):
    a, b = i0 + i2, i0 - i2
    c = ((i1 * 35468) >> 16) - (i3 + ((i3 * 20091) >> 16))
    d = (i1 + ((i1 * 20091) >> 16)) + ((i3 * 35468) >> 16)
    return a + d, b + c, b - c, a - d


def idct(dq, trunc=s16):
    """vp8_short_idct4x4llm_c (vp8/common/idctllm.c:28-110) without the predictor: dequantised blocks [..., 4, 4] (row, col) ->
    the sixteen values it adds [..., 4, 4]"""
    t = trunc(np.stack(_idct_pass(dq[..., 0, :], dq[..., 1, :], dq[..., 2, :], dq[..., 3, :]), -2))      # vertical, `short output[16]`
    o = _idct_pass(t[..., 0], t[..., 1], t[..., 2], t[..., 3])
    return trunc(np.stack([(v + 4) >> 3 for v in o], -1))


def residual_blocks(hdr, mbs, coef, wrap=True):
    """-> int64 [nmb, 24, 4, 4] (row, col): what decode_macroblock adds to the prediction of every block"""
    trunc = s16 if wrap else keep
    nmb = hdr.mb_rows * hdr.mb_cols
    mbs = np.asarray(mbs).reshape(nmb, 64)
    q = np.asarray(coef, np.int64).reshape(nmb, 25, 4, 4).transpose(0, 1, 3, 2)          # [mb, block, row, col]
    f = factors(hdr)[mbs[:, O_SEGMENT] & 3]                                             # [nmb, 6]
    y_mode = mbs[:, O_Y_MODE]
    has_y2 = (y_mode != B_PRED) & (y_mode != SPLITMV)
    eobs = mbs[:, O_EOBS:O_EOBS + 25].astype(np.int64)
    skip = (mbs[:, O_FLAGS] & MB_SKIP) != 0

    def spread(dc, ac):                          # the sixteen factors of a block: [nmb, 4, 4]
        m = np.repeat(ac[:, None], 16, 1).reshape(nmb, 4, 4).copy()
        m[:, 0, 0] = dc
        return m
    # the Y2 block: decodframe.c:258-284
    wht = inv_walsh(trunc(q[:, 24] * spread(f[:, 2], f[:, 3])), trunc)
    a1 = trunc((trunc(q[:, 24, 0, 0] * f[:, 2]) + 3) >> 3)
    y2dc = np.where((eobs[:, 24] > 1)[:, None, None], wht, a1[:, None, None]).reshape(nmb, 16)
    out = np.zeros((nmb, 24, 4, 4), np.int64)
    one = np.ones(nmb, np.int64)
    for b in range(24):
        luma = b < 16
        dcf = np.where(has_y2, one, f[:, 0]) if luma else f[:, 4]
        acf = f[:, 1] if luma else f[:, 5]
        first = np.where(has_y2, y2dc[:, b], q[:, b, 0, 0]) if luma else q[:, b, 0, 0]
        blk = q[:, b].copy()
        blk[:, 0, 0] = first
        full = idct(trunc(blk * spread(dcf, acf)), trunc)                               # idct_blk.c: eob > 1
        dc = trunc((trunc(first * dcf) + 4) >> 3)                                       # ... else vp8_dc_only_idct_add_c
        out[:, b] = np.where((eobs[:, b] > 1)[:, None, None], full, dc[:, None, None])
    out[skip] = 0
    return out


def residual_planes(hdr, mbs, coef, wrap=True):
    """-> (Y int16 [16 * mb_rows, 16 * mb_cols], U, V int16 [8 * mb_rows, 8 * mb_cols]): the coded area.  wrap=False: the same
    arithmetic with no int16 truncation anywhere (int64; for tests that ask where the truncations bite)"""
    rows, cols = hdr.mb_rows, hdr.mb_cols
    blk = residual_blocks(hdr, mbs, coef, wrap)
    t = np.int16 if wrap else np.int64
    y = blk[:, :16].reshape(rows, cols, 4, 4, 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(16 * rows, 16 * cols)
    u = blk[:, 16:20].reshape(rows, cols, 2, 2, 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(8 * rows, 8 * cols)
    v = blk[:, 20:24].reshape(rows, cols, 2, 2, 4, 4).transpose(0, 2, 4, 1, 3, 5).reshape(8 * rows, 8 * cols)
    return y.astype(t), u.astype(t), v.astype(t)


def grid(hdr, dst_w=0, dst_h=0):
    """-> (gw, gh, cw, ch, sx [gw], sy [gh], scx [cw], scy [ch]): the luma and I420 chroma grids and the sample each column / row takes"""
    if dst_w == 0 and dst_h == 0:
        gw, gh = 16 * hdr.mb_cols, 16 * hdr.mb_rows
        return gw, gh, gw // 2, gh // 2, np.arange(gw), np.arange(gh), np.arange(gw // 2), np.arange(gh // 2)
    cw, ch = (dst_w + 1) // 2, (dst_h + 1) // 2
    return (dst_w, dst_h, cw, ch, grid_map(dst_w, hdr.width), grid_map(dst_h, hdr.height),
            grid_map(cw, (hdr.width + 1) // 2), grid_map(ch, (hdr.height + 1) // 2))


def size(hdr, dst_w=0, dst_h=0, dtype="i16", layout="planar"):
    gw, gh, cw, ch = grid(hdr, dst_w, dst_h)[:4]
    return (3 * gh * gw if layout == "planar" else gh * gw + 2 * ch * cw) * np.dtype(DTYPES[dtype]).itemsize


def arrange(planes, hdr, dst_w=0, dst_h=0, dtype="i16", layout="planar", scale=(1.0, 1.0, 1.0)):
    """the coded area's planes (residual_planes) -> the tensor: [3, gh, gw] ("planar"), or the three planes back to back, flat ("i420")"""
    y, u, v = planes
    _, _, _, _, sx, sy, scx, scy = grid(hdr, dst_w, dst_h)
    if layout == "planar":
        return np.stack([convert(y[sy][:, sx], dtype, scale[0]), convert(u[sy >> 1][:, sx >> 1], dtype, scale[1]),
                         convert(v[sy >> 1][:, sx >> 1], dtype, scale[2])])
    return np.concatenate([convert(y[sy][:, sx], dtype, scale[0]).ravel(), convert(u[scy][:, scx], dtype, scale[1]).ravel(),
                           convert(v[scy][:, scx], dtype, scale[2]).ravel()])


def residual(hdr, mbs, coef, dst_w=0, dst_h=0, dtype="i16", layout="planar", scale=(1.0, 1.0, 1.0)):
    """-> the tensor of one frame as vp8hip_frames_residual_async writes it"""
    return arrange(residual_planes(hdr, mbs, coef), hdr, dst_w, dst_h, dtype, layout, scale)
