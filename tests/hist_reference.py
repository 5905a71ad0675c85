"""The definitions of vp8hip_frames_hist_async, vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async and
vp8hip_trace_cover_hist_async (include/vp8hip.h) a second time, in numpy: np.bincount(..., minlength=256) over the U8 tensors the
other reference modules give -- a picture's planes at the display size, side_reference's info tensor on the native grid (plus
MVMAG), wear_reference.tensor and invert_reference.tensor.  Nothing here knows how the kernels go about it."""
import numpy as np

import invert_reference as V
import side_reference as S
import wear_reference as W

FRAME_PLANES = {"y": 1, "u": 2, "v": 4}
SLOT_PLANES = dict(S.PLANES, mvmag=64)
MVMAG = 6                                         # the plane of bit 64, behind side_reference's six


def mask_of(planes, table):
    return planes if isinstance(planes, int) else sum({table[p] for p in planes})


def hist_size(nplanes):
    return nplanes * 1024


def counts(tensor):
    """a U8 tensor [C, ...] -> uint32 [C, 256]"""
    t = np.asarray(tensor)
    assert t.dtype == np.uint8
    return np.stack([np.bincount(p.ravel(), minlength=256) for p in t]).astype(np.uint32).reshape(len(t), 256)


def frames(planes_yuv, ref_yuv=None, planes=7):
    """the planes (y, u, v) of a picture at the display size, uint8 each -- and those of the picture it is compared with -- ->
    uint32 [popcount(planes), 256]: the samples equal to k, or the sample positions where |a - b| equals k"""
    mask = mask_of(planes, FRAME_PLANES)
    out = []
    for p in range(3):
        if not mask >> p & 1:
            continue
        a = np.asarray(planes_yuv[p])
        assert a.dtype == np.uint8
        if ref_yuv is not None:
            a = np.abs(a.astype(np.int16) - np.asarray(ref_yuv[p]).astype(np.int16)).astype(np.uint8)
        out.append(np.bincount(a.ravel(), minlength=256))
    return np.stack(out).astype(np.uint32)


def mvmag(vx, vy):
    """the MVMAG value of vectors (vx, vy) in 1/8 pel, int16: whole pixels by (v + 4) >> 3, arithmetic, as the trace rounds a hop; the
    larger magnitude, capped at 255"""
    px = (np.asarray(vx, np.int32) + 4) >> 3
    py = (np.asarray(vy, np.int32) + 4) >> 3
    return np.minimum(np.maximum(np.abs(px), np.abs(py)), 255).astype(np.uint8)


def slot_tensor(hdr, mbs, mvs, planes):
    """the U8 tensor the slot call counts: side_reference's info planes on the native grid, then MVMAG, those of `planes` in bit order"""
    mask = mask_of(planes, SLOT_PLANES)
    mv, info = S.cells(hdr, mbs, mvs)
    every = np.concatenate([info, mvmag(mv[0], mv[1])[None]])
    return every[[b for b in range(7) if mask >> b & 1]]


def slots(hdr, mbs, mvs, planes):
    return counts(slot_tensor(hdr, mbs, mvs, planes))


def wear(entry, planes=15):
    """a wear entry uint32 [d_h, d_w] -> uint32 [popcount(planes), 256] over wear_reference.tensor at the display size"""
    return counts(W.tensor(entry, 0, 0, planes, "u8"))


def cover(count, planes=3):
    """a COUNT entry uint32 [d_h, d_w] -> uint32 [popcount(planes), 256] over invert_reference.tensor at the display size"""
    return counts(V.tensor(count, 0, 0, planes, "u8"))


def sse(h):
    """the sum of squared differences a pair histogram [256] holds"""
    return int((np.asarray(h, np.int64) * np.arange(256, dtype=np.int64) ** 2).sum())
