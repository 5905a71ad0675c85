"""The definition of vp8hip_trace_gather_async (include/vp8hip.h) a second time, in numpy: from a source tensor [C, sh, sw] of any
element type and a frame's trace (uint32 [d_h, d_w], x' in the low int16 and y' in the high one) to the tensor [C, gh, gw].  The
integer maps are restated exactly as the header writes them.  NEAREST moves elements; BILINEAR gives R, the header's real number,
in float64: a product of a float (or half) and a 17-bit weight is exact there, and the sum of the four is off by at most three
float64 roundings, 2^-51 relative to the largest corner -- far below every bound the header allows the call, which bound() restates.
Layouts are not a matter of the definition: the arrays here are indexed [c, y, x] whatever the memory format.  Nothing here knows how
the kernels go about it."""
import numpy as np

from tensor_reference import grid_map
from trace_reference import clamped


def size(w, h, channels, elem, dst_w=0, dst_h=0):
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return channels * gh * gw * elem


def anchor_positions(t, w, h, dst_w=0, dst_h=0):
    """(ax, ay) int64 [gh, gw]: the clamped position the trace names under each output's centre"""
    t = np.asarray(t, np.uint32)
    assert t.shape == (h, w)
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    sx, sy = grid_map(gw, w), grid_map(gh, h)
    return clamped(t[sy][:, sx], w, h)


def nearest_cell(a, s, d):
    """cx = ((2 ax + 1) * sw) / (2 d_w): the cell of s under the centre of pixel a of d"""
    return ((2 * np.asarray(a, np.int64) + 1) * s) // (2 * d)


def bilinear_cell(a, s, d):
    """-> (x0, x1, wx, px): px = clamp(((2 ax + 1) * sw * 128) / d_w - 128, 0, (sw - 1) * 256), x0 = px >> 8, wx = px & 255,
    x1 = min(x0 + 1, sw - 1)"""
    p = np.clip(((2 * np.asarray(a, np.int64) + 1) * s * 128) // d - 128, 0, (s - 1) * 256)
    x0 = p >> 8
    return x0, np.minimum(x0 + 1, s - 1), p & 255, p


def nearest(src, t, w, h, dst_w=0, dst_h=0):
    """src [C, sh, sw] -> [C, gh, gw] of src's type: src[:, cy, cx]"""
    src = np.asarray(src)
    _, sh, sw = src.shape
    ax, ay = anchor_positions(t, w, h, dst_w, dst_h)
    return np.ascontiguousarray(src[:, nearest_cell(ay, sh, h), nearest_cell(ax, sw, w)])


def bilinear(src, t, w, h, dst_w=0, dst_h=0):
    """src [C, sh, sw] of float16 / float32 -> (R, M): float64 [C, gh, gw] each, the header's R and M = max(|a|, |b|, |c'|, |d|)"""
    src = np.asarray(src)
    assert src.dtype in (np.float16, np.float32)
    _, sh, sw = src.shape
    ax, ay = anchor_positions(t, w, h, dst_w, dst_h)
    x0, x1, wx, _ = bilinear_cell(ax, sw, w)
    y0, y1, wy, _ = bilinear_cell(ay, sh, h)
    s64 = src.astype(np.float64)
    a, b, c, d = s64[:, y0, x0], s64[:, y0, x1], s64[:, y1, x0], s64[:, y1, x1]
    wx, wy = wx.astype(np.float64), wy.astype(np.float64)
    R = (a * ((256 - wx) * (256 - wy)) + b * (wx * (256 - wy)) + c * ((256 - wx) * wy) + d * (wx * wy)) / 65536.0
    M = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))
    return R, M


def bound(R, M, dtype):
    """the header's bound on |out - R|: floats 8 * 2^-24 * M; halves that + 2^-11 * |R| + 2^-25"""
    b = 8.0 * 2.0 ** -24 * M
    if np.dtype(dtype) == np.float16:
        b = b + 2.0 ** -11 * np.abs(R) + 2.0 ** -25
    return b


def bilinear_excess(out, R, M):
    """the largest |out - R| - bound over the tensor: <= 0 where the call keeps the header's promise"""
    out = np.asarray(out)
    return float((np.abs(out.astype(np.float64) - R) - bound(R, M, out.dtype)).max())
