"""The definitions of vp8hip_frames_trace_async and vp8hip_trace_flow_async (include/vp8hip.h) a second time, in numpy: from the
dense IR of a frame (mbs uint8 [nmb, 64] = vp8ir_mb records, mvs int16 [nmb * 16, 2] = (row, col), and the frame header) and the
traces of its references to the frame's trace -- uint32 [d_h, d_w], x' in the low int16 and y' in the high one -- and from a trace
to the flow tensor [2, gh, gw].  Nothing here knows how the kernels go about it."""
import numpy as np

from tensor_reference import DTYPES, convert, grid_map  # noqa: F401

O_REF = 2                                        # byte offset of ref_frame in a vp8ir_mb record (include/vp8_ir.h)


def pack(x, y):
    """(x', y') -> the trace's dwords"""
    return (np.asarray(x).astype(np.int64) & 0xffff).astype(np.uint32) | ((np.asarray(y).astype(np.int64) & 0xffff) << 16).astype(np.uint32)


def unpack(t):
    """the trace's dwords -> (x', y') as int16"""
    t = np.asarray(t, np.uint32)
    return (t & 0xffff).astype(np.uint16).view(np.int16), (t >> 16).astype(np.uint16).view(np.int16)


def clamped(t, w, h):
    """the position a trace names, clamped to the picture: (ax, ay) as int64"""
    tx, ty = unpack(t)
    return np.clip(tx.astype(np.int64), 0, w - 1), np.clip(ty.astype(np.int64), 0, h - 1)


def identity(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return pack(xs, ys)


def hop(hdr, mbs, mvs):
    """one hop of an inter frame, per display pixel: (r, sy, sx) int [d_h, d_w] -- the reference (1..3; an intra macroblock: 1, with
    a zero vector) and the position in it, the vector rounded to whole pixels (ties up) and clamped to the picture"""
    w, h, cols = int(hdr.width), int(hdr.height), int(hdr.mb_cols)
    ys, xs = np.mgrid[0:h, 0:w]
    mb = (ys >> 4) * cols + (xs >> 4)
    k = ((ys >> 2) & 3) * 4 + ((xs >> 2) & 3)
    v = np.asarray(mvs, np.int16).reshape(-1, 16, 2)[mb, k].astype(np.int64)
    ref = np.asarray(mbs).reshape(-1, 64)[:, O_REF][mb].astype(np.int64)
    v[ref == 0] = 0
    r = np.where(ref == 0, 1, ref)
    sx = np.clip(xs + ((v[..., 1] + 4) >> 3), 0, w - 1)
    sy = np.clip(ys + ((v[..., 0] + 4) >> 3), 0, h - 1)
    return r, sy, sx


def trace(hdr, mbs, mvs, refs):
    """-> uint32 [d_h, d_w] as vp8hip_frames_trace_async writes it.  refs: the traces of (last, golden, altref), each uint32
    [d_h, d_w] or None (the job's -1)"""
    w, h = int(hdr.width), int(hdr.height)
    out = identity(w, h)
    if hdr.frame_type == 0:
        return out
    r, sy, sx = hop(hdr, mbs, mvs)
    for q in (1, 2, 3):
        src = refs[q - 1]
        if src is not None:
            sel = r == q
            out[sel] = np.asarray(src, np.uint32)[sy[sel], sx[sel]]
    return out


def flow_size(w, h, dst_w=0, dst_h=0, dtype="i16"):
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return 2 * gh * gw * np.dtype(DTYPES[dtype]).itemsize


def flow(t, dst_w=0, dst_h=0, dtype="i16", scale=(1.0, 1.0)):
    """trace uint32 [d_h, d_w] -> [2, gh, gw] of DTYPES[dtype] as vp8hip_trace_flow_async writes it: x' - sx, y' - sy under each
    output's centre (int16: the difference's low 16 bits)"""
    h, w = t.shape
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    sx, sy = grid_map(gw, w), grid_map(gh, h)
    tx, ty = unpack(t[sy][:, sx])
    a = np.stack([tx.astype(np.int64) - sx[None, :], ty.astype(np.int64) - sy[:, None]])
    return convert(a, dtype, scale)


def pixel_scale(w, h, dst_w=0, dst_h=0):
    """scale="pixels" of Vp8Hip.trace_flow: the flow in pixels of the tensor"""
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return np.float32(gw / w), np.float32(gh / h)
