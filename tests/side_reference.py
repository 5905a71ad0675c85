"""The definition of vp8hip_frames_side_async (include/vp8hip.h) a second time, in numpy: from the dense IR of a frame (mbs uint8
[nmb, 64] = vp8ir_mb records, mvs int16 [nmb * 16, 2] = (row, col), and the frame header) to the two tensors the call writes,
mv [2, gh, gw] and info [C, gh, gw].  Nothing here knows how the kernel goes about it."""
import numpy as np

from tensor_reference import DTYPES, convert, grid_map  # noqa: F401  (the mv tensor's types; its values by channel; the cell map)

PLANES = {"ref": 1, "mode": 2, "skip": 4, "segment": 8, "qindex": 16, "coded": 32}
B_PRED, SPLITMV = 4, 9
MB_SKIP = 1
# byte offsets in a vp8ir_mb record (include/vp8_ir.h)
O_Y_MODE, O_REF, O_FLAGS, O_SEGMENT, O_EOBS, O_B_MODES = 0, 2, 3, 4, 8, 40


def mask_of(planes):
    if isinstance(planes, int):
        return planes
    m = 0
    for p in planes:
        m |= PLANES[p]
    return m


def grid(hdr, dst_w=0, dst_h=0):
    """-> (gw, gh, bx [gw], by [gh]): the grid and the cell each output column / row takes"""
    if dst_w == 0 and dst_h == 0:
        gw, gh = 4 * hdr.mb_cols, 4 * hdr.mb_rows
        return gw, gh, np.arange(gw), np.arange(gh)
    return dst_w, dst_h, grid_map(dst_w, hdr.width) >> 2, grid_map(dst_h, hdr.height) >> 2


def sizes(hdr, dst_w=0, dst_h=0, dtype="i16", planes=0):
    gw, gh, _, _ = grid(hdr, dst_w, dst_h)
    return 2 * gh * gw * np.dtype(DTYPES[dtype]).itemsize, bin(mask_of(planes)).count("1") * gh * gw


def qindex_of_segments(hdr):
    """the quantiser index of each of the four segments (mb_init_dequantizer, vp8/decoder/decodframe.c)"""
    out = []
    for s in range(4):
        q = int(hdr.base_qindex)
        if hdr.segmentation_enabled:
            q = int(hdr.segment_quant[s]) if hdr.mb_segment_abs_delta else q + int(hdr.segment_quant[s])
        out.append(min(max(q, 0), 127))
    return np.array(out, np.uint8)


def block_kind(mbs):
    """vp8ir_block_kind for the 16 luma blocks of every macroblock: uint8 [nmb, 16]"""
    y_mode = mbs[:, O_Y_MODE]
    has_y2 = ((y_mode != B_PRED) & (y_mode != SPLITMV))[:, None]
    eobs = mbs[:, O_EOBS:O_EOBS + 16]
    kind = np.where(eobs > 1, 2, np.where((eobs == 1) & ~has_y2, 1, 0))
    return np.where((mbs[:, O_FLAGS] & MB_SKIP)[:, None] != 0, 0, kind).astype(np.uint8)


def cells(hdr, mbs, mvs):
    """the native grid: vectors int16 [2, 4 * mb_rows, 4 * mb_cols] (x, y) and the six info planes uint8 [6, ...] in bit order"""
    rows, cols = hdr.mb_rows, hdr.mb_cols
    nmb = rows * cols
    mbs = np.asarray(mbs).reshape(nmb, 64)

    def to_grid(per_block):                      # [nmb, 16] -> [4 * rows, 4 * cols]; block k = (by & 3) * 4 + (bx & 3)
        return per_block.reshape(rows, cols, 4, 4).transpose(0, 2, 1, 3).reshape(4 * rows, 4 * cols)

    def per_mb(v):
        return np.repeat(np.asarray(v)[:, None], 16, 1)
    ref = mbs[:, O_REF]
    if hdr.frame_type == 0:
        vec = np.zeros((nmb, 16, 2), np.int16)                        # (the slot's vector area is stale: not read)
    else:
        vec = np.asarray(mvs, np.int16).reshape(nmb, 16, 2).copy()
        vec[ref == 0] = 0
    mv = np.stack([to_grid(vec[:, :, 1]), to_grid(vec[:, :, 0])])    # channel 0 = x = col, channel 1 = y = row
    y_mode = mbs[:, O_Y_MODE]
    mode = np.where((y_mode == B_PRED)[:, None], 10 + mbs[:, O_B_MODES:O_B_MODES + 16], per_mb(y_mode)).astype(np.uint8)
    seg = mbs[:, O_SEGMENT]
    info = np.stack([to_grid(per_mb(ref)), to_grid(mode), to_grid(per_mb(mbs[:, O_FLAGS] & MB_SKIP)), to_grid(per_mb(seg)),
                     to_grid(per_mb(qindex_of_segments(hdr)[seg & 3])), to_grid(block_kind(mbs))]).astype(np.uint8)
    return mv, info


def side(hdr, mbs, mvs, dst_w=0, dst_h=0, dtype="i16", planes=0, scale=(1.0, 1.0)):
    """-> (mv [2, gh, gw] of DTYPES[dtype], info uint8 [popcount(planes), gh, gw]) as vp8hip_frames_side_async writes them"""
    mv, info = cells(hdr, mbs, mvs)
    _, _, bx, by = grid(hdr, dst_w, dst_h)
    m = mask_of(planes)
    sel = [b for b in range(6) if m >> b & 1]
    return convert(mv[:, by][:, :, bx], dtype, scale), info[sel][:, by][:, :, bx]


def pixel_scale(hdr, dst_w=0, dst_h=0):
    """scale="pixels" of Vp8Hip.frames_side: the flow in pixels of the tensor"""
    if dst_w == 0 and dst_h == 0:
        return np.float32(0.125 * 4 * hdr.mb_cols / (16 * hdr.mb_cols)), np.float32(0.125 * 4 * hdr.mb_rows / (16 * hdr.mb_rows))
    return np.float32(0.125 * dst_w / hdr.width), np.float32(0.125 * dst_h / hdr.height)
