"""The definitions of vp8hip_frames_wear_async and vp8hip_trace_wear_async (include/vp8hip.h) a second time, in numpy, on top of
trace_reference.hop: from the dense IR of a frame (mbs uint8 [nmb, 64] = vp8ir_mb records, mvs int16 [nmb * 16, 2] = (row, col), and
the frame header) and the wear of its references to the frame's wear -- uint32 [d_h, d_w], the counters HOPS, INTRA, EDGE, CODED in
bytes 0..3 -- and from a wear entry to the tensor [C, gh, gw].  Nothing here knows how the kernels go about it."""
import numpy as np

from tensor_reference import grid_map
import trace_reference as R

O_MODE, O_REF, O_FLAGS, O_EOBS = 0, 2, 3, 8      # byte offsets in a vp8ir_mb record (include/vp8_ir.h)
B_PRED, SPLITMV = 4, 9
MB_SKIP = 1
HOPS, INTRA, EDGE, CODED = range(4)              # the counters' bytes
PLANES = {"hops": 1, "intra": 2, "edge": 4, "coded": 8}
DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}


def block_kinds(mbs):
    """vp8ir_block_kind(m, k) for every macroblock and k in 0..24: int [nmb, 25]"""
    m = np.asarray(mbs).reshape(-1, 64)
    eobs = m[:, O_EOBS:O_EOBS + 25].astype(np.int64)
    has_y2 = ((m[:, O_MODE] != B_PRED) & (m[:, O_MODE] != SPLITMV))[:, None]
    starts_at_1 = has_y2 & (np.arange(25) < 16)[None, :]
    kind = np.where(eobs > 1, 2, np.where((eobs == 1) & ~starts_at_1, 1, 0))
    kind[:, 24] = np.where(has_y2[:, 0], kind[:, 24], 0)
    kind[(m[:, O_FLAGS] & MB_SKIP) != 0] = 0
    return kind


def pack(c):
    """counters int [4, ...] (0..255) -> the wear's dwords"""
    c = np.asarray(c).astype(np.uint32)
    return c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24


def unpack(w):
    """the wear's dwords -> counters uint8 [4, ...]"""
    w = np.asarray(w, np.uint32)
    return np.stack([(w >> (8 * b)) & 255 for b in range(4)]).astype(np.uint8)


def incs(hdr, mbs, mvs):
    """one hop's increments per display pixel: uint8 [4, d_h, d_w], each 0 or 1 -- (every hop; the macroblock is intra; the clamp moved
    the position; the luma block, or the macroblock's Y2 block, has coefficients in a macroblock that is not skipped)"""
    w, h, cols = int(hdr.width), int(hdr.height), int(hdr.mb_cols)
    ys, xs = np.mgrid[0:h, 0:w]
    mb = (ys >> 4) * cols + (xs >> 4)
    k = ((ys >> 2) & 3) * 4 + ((xs >> 2) & 3)
    m = np.asarray(mbs).reshape(-1, 64)
    ref = m[:, O_REF][mb]
    v = np.asarray(mvs, np.int16).reshape(-1, 16, 2)[mb, k].astype(np.int64)
    v[ref == 0] = 0
    ux, uy = xs + ((v[..., 1] + 4) >> 3), ys + ((v[..., 0] + 4) >> 3)
    _, sy, sx = R.hop(hdr, mbs, mvs)
    kind = block_kinds(m)
    coded = (kind[mb, k] != 0) | (kind[mb, 24] != 0)
    return np.stack([np.ones((h, w), bool), ref == 0, (sx != ux) | (sy != uy), coded]).astype(np.uint8)


def wear(hdr, mbs, mvs, refs):
    """-> uint32 [d_h, d_w] as vp8hip_frames_wear_async writes it.  refs: the wear of (last, golden, altref), each uint32 [d_h, d_w]
    or None (the job's -1)"""
    w, h = int(hdr.width), int(hdr.height)
    out = np.zeros((h, w), np.uint32)
    if hdr.frame_type == 0:
        return out
    r, sy, sx = R.hop(hdr, mbs, mvs)
    inc = incs(hdr, mbs, mvs).astype(np.int64)
    for q in (1, 2, 3):
        src = refs[q - 1]
        if src is not None:
            sel = r == q
            was = unpack(np.asarray(src, np.uint32)[sy[sel], sx[sel]]).astype(np.int64)
            out[sel] = pack(np.minimum(was + inc[:, sel], 255))
    return out


def plane_mask(planes):
    return planes if isinstance(planes, int) else sum({PLANES[p] for p in planes})


def tensor_size(w, h, dst_w=0, dst_h=0, planes=15, dtype="u8"):
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return bin(plane_mask(planes)).count("1") * gh * gw * np.dtype(DTYPES[dtype]).itemsize


def tensor(w, dst_w=0, dst_h=0, planes=15, dtype="u8", scale=(1.0, 1.0, 1.0, 1.0)):
    """wear uint32 [d_h, d_w] -> [C, gh, gw] of DTYPES[dtype] as vp8hip_trace_wear_async writes it: the counters of `planes` (names or
    the mask) in bit order under each output's centre; u8: the byte; f32: float32(float64(v) * float64(float32(scale[c]))), c the
    counter; f16: that float rounded to a half"""
    h, wd = w.shape
    gw, gh = (wd, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    sx, sy = grid_map(gw, wd), grid_map(gh, h)
    mask = plane_mask(planes)
    which = [c for c in range(4) if mask >> c & 1]
    v = unpack(np.asarray(w, np.uint32)[sy][:, sx])[which]
    if dtype == "u8":
        return v
    s = np.asarray(scale, np.float32).astype(np.float64)[which]
    f = (v.astype(np.float64) * s[:, None, None]).astype(np.float32)
    if dtype == "f32":
        return f
    with np.errstate(over="ignore"):
        return f.astype(np.float16)
