"""The definitions of vp8hip_trace_invert_async and vp8hip_trace_cover_async (include/vp8hip.h) a second time, in numpy, on top of
trace_reference.clamped and tensor_reference.grid_map: from a trace -- uint32 [d_h, d_w] -- to FIRST and COUNT over the anchor's grid,
uint32 [d_h, d_w] each, and from a COUNT entry to the tensor [C, gh, gw].  Nothing here knows how the kernels go about it."""
import numpy as np

from tensor_reference import grid_map
import trace_reference as R

NONE = np.uint32(0xffffffff)                     # FIRST where no frame pixel names the anchor pixel
PLANES = {"count": 1, "seen": 2}
DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}


def invert(t, w, h):
    """trace uint32 [h, w] -> (first, count), uint32 [h, w] each: for anchor pixel (ay, ax), the first frame pixel in raster order
    whose clamped trace is (ax, ay), packed as a trace packs a position (0xffffffff: none), and how many such frame pixels there are"""
    ax, ay = R.clamped(np.asarray(t, np.uint32).reshape(h, w), w, h)
    a = (ay * w + ax).ravel()                    # frame pixels in raster order -> the anchor pixel each names
    # the first occurrence of each anchor pixel among the frame pixels in raster order is its first descendant
    named, where, many = np.unique(a, return_index=True, return_counts=True)
    first = np.full(h * w, NONE, np.uint32)
    first[named] = R.pack(where % w, where // w)
    count = np.zeros(h * w, np.uint32)
    count[named] = many
    return first.reshape(h, w), count.reshape(h, w)


def plane_mask(planes):
    return planes if isinstance(planes, int) else sum({PLANES[p] for p in planes})


def tensor_size(w, h, dst_w=0, dst_h=0, planes=3, dtype="u8"):
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    return bin(plane_mask(planes)).count("1") * gh * gw * np.dtype(DTYPES[dtype]).itemsize


def tensor(count, dst_w=0, dst_h=0, planes=3, dtype="u8", scale=(1.0, 1.0)):
    """COUNT uint32 [d_h, d_w] -> [C, gh, gw] of DTYPES[dtype] as vp8hip_trace_cover_async writes it: the planes of `planes` (names or
    the mask) in bit order under each output's centre, "count" min(c, 255) and "seen" c != 0; u8: that value; f32:
    float32(float64(v) * float64(float32(scale[plane]))); f16: that float rounded to a half"""
    h, w = count.shape
    gw, gh = (w, h) if dst_w == 0 and dst_h == 0 else (dst_w, dst_h)
    sx, sy = grid_map(gw, w), grid_map(gh, h)
    mask = plane_mask(planes)
    which = [c for c in range(2) if mask >> c & 1]
    c = np.asarray(count, np.uint32)[sy][:, sx]
    v = np.stack([np.minimum(c, 255), c != 0]).astype(np.uint8)[which]
    if dtype == "u8":
        return v
    s = np.asarray(scale, np.float32).astype(np.float64)[which]
    f = (v.astype(np.float64) * s[:, None, None]).astype(np.float32)
    if dtype == "f32":
        return f
    with np.errstate(over="ignore"):
        return f.astype(np.float16)
