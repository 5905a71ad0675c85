"""The definition of vp8hip_trace_residual_async (include/vp8hip.h) a second time, in numpy: from two packed I420 images of the
display size -- the frame and its anchor picture -- and the frame's trace (uint32 [d_h, d_w], x' in the low int16 and y' in the high
one) to the tensor [3, gh, gw].  Built on rgb_reference (the bytes), trace_reference (the dwords) and tensor_reference (the grid and
the element types).  Nothing here knows how the kernel goes about it."""
import numpy as np

import rgb_reference as RGB
from tensor_reference import DTYPES, convert, grid_map
from trace_reference import clamped


def size(w, h, dst_w=0, dst_h=0, dtype="i16"):
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return 3 * gh * gw * np.dtype(DTYPES[dtype]).itemsize


def pack_i420(y, u, v):
    """three planes -> the packed image"""
    return np.concatenate([np.asarray(p, np.uint8).ravel() for p in (y, u, v)])


def residual(cur, anchor, t, w, h, dst_w=0, dst_h=0, dtype="i16", matrix="bt601", order="rgb", scale=(1.0, 1.0, 1.0)):
    """cur, anchor: packed I420 of w x h; t: the trace of cur -> [3, gh, gw] of DTYPES[dtype] as vp8hip_trace_residual_async writes
    it: the RGB bytes of cur under each output's centre minus those of anchor at the clamped position the trace names there; scale
    by COLOUR (R, G, B), planes in `order`"""
    t = np.asarray(t, np.uint32)
    assert t.shape == (h, w)
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    c = RGB.convert(cur, w, h, matrix=matrix).astype(np.int64)          # [3, h, w], R, G, B
    a = RGB.convert(anchor, w, h, matrix=matrix).astype(np.int64)
    sx, sy = grid_map(gw, w), grid_map(gh, h)
    ax, ay = clamped(t[sy][:, sx], w, h)
    d = c[:, sy[:, None], sx[None, :]] - a[:, ay, ax]
    out = convert(d, dtype, np.broadcast_to(np.asarray(scale, np.float32), (3,)))
    return np.ascontiguousarray(out[::-1] if order == "bgr" else out)
