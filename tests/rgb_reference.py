"""The colour conversion of vp8hip_frames_rgb_async (include/vp8hip.h) restated in numpy, for the tests.  There is no routine in the
reference tree to match (its libyuv snapshot has only the scaler), so the arithmetic is defined by the header, exactly, in
integers; this file says the same thing a second time and tests/test_rgb_cpu.py ties it to the exact float64 matrices.

The result for a frame is convert(S), S being the packed I420 image the scaler writes (scale_reference.scale_frame)."""
import numpy as np

import scale_reference as S

# yoff, cy, crv, cgu, cgv, cbu: the exact matrices times 256, rounded
MATRICES = {
    "bt601": (16, 298, 409, -100, -208, 516),
    "bt601-full": (0, 256, 359, -88, -183, 454),
    "bt709": (16, 298, 459, -55, -136, 541),
}
MATRIX_IDS = {"bt601": 0, "bt601-full": 1, "bt709": 2}          # VP8HIP_RGB_BT601 ...
LAYOUTS = {"planar": 0, "packed3": 1, "packed4": 2}             # VP8HIP_RGB_PLANAR ...
ORDERS = {"rgb": 0, "bgr": 1}
DTYPES = {"u8": 0, "f16": 1, "f32": 2}                          # VP8HIP_RGB_U8 ...
NP_DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def scale_bias(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """the float32 pair Vp8Hip.frames_rgb passes for mean / std on the 0..1 scale: computed in float64, cast once"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def exact_matrix(matrix):
    """(yoff, ky, [[ru, rv], [gu, gv], [bu, bv]]) of the exact conversion in float64: channel = ky * (Y - yoff) + cu * (U - 128) + cv * (V - 128)"""
    kr, kb = (0.2126, 0.0722) if matrix == "bt709" else (0.299, 0.114)
    kg = 1.0 - kr - kb
    full = matrix == "bt601-full"
    ky, kc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    rv, bu = 2.0 * (1.0 - kr), 2.0 * (1.0 - kb)
    return (0 if full else 16), ky, [[0.0, kc * rv], [-kc * kb * bu / kg, -kc * kr * rv / kg], [kc * bu, 0.0]]


def rgb_bytes(y, u, v, matrix):
    """R, G, B bytes (int64 arrays) of Y, U, V arrays of one shape: the header's integer arithmetic"""
    yoff, cy, crv, cgu, cgv, cbu = MATRICES[matrix]
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    l = cy * (y - yoff) + 128
    r = np.clip((l + crv * (v - 128)) >> 8, 0, 255)
    g = np.clip((l + cgu * (u - 128) + cgv * (v - 128)) >> 8, 0, 255)
    b = np.clip((l + cbu * (u - 128)) >> 8, 0, 255)
    return r, g, b


def element(v, c_scale, c_bias, dtype):
    """the element for byte(s) v of a colour with float32 scale / bias"""
    if dtype == "u8":
        return np.asarray(v).astype(np.uint8)
    f = np.float32(np.asarray(v).astype(np.float64) * np.float64(c_scale) + np.float64(c_bias))
    return f if dtype == "f32" else np.float16(f)


def convert(packed, w, h, matrix="bt601", layout="planar", order="rgb", dtype="u8", scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """packed I420 (S.i420_size(w, h) bytes) -> [3, h, w] (planar), [h, w, 3] (packed3) or [h, w, 4] (packed4: fourth byte 255, u8
    only): chroma replicated, channels in `order`, scale / bias by COLOUR (R, G, B)"""
    assert not (layout == "packed4" and dtype != "u8")
    cw, ch = (w + 1) // 2, (h + 1) // 2
    packed = np.asarray(packed, np.uint8)
    assert packed.size == S.i420_size(w, h)
    y = packed[:w * h].reshape(h, w)
    u = packed[w * h:w * h + cw * ch].reshape(ch, cw)
    v = packed[w * h + cw * ch:].reshape(ch, cw)
    yy, xx = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    rgb = rgb_bytes(y, u[yy, xx], v[yy, xx], matrix)
    chans = [element(rgb[c], np.float32(scale[c]), np.float32(bias[c]), dtype) for c in range(3)]
    if order == "bgr":
        chans = chans[::-1]
    if layout == "planar":
        return np.stack(chans, axis=0)
    if layout == "packed4":
        chans.append(np.full((h, w), 255, np.uint8))
    return np.ascontiguousarray(np.stack(chans, axis=-1))


def rgb_frame(buf, g, w, h, dw, dh, filt, **kw):
    """the w x h picture in frame buffer `buf` (geometry g) as RGB at dw x dh: convert(I420Scale(...))"""
    return convert(S.scale_frame(buf, g, w, h, dw, dh, filt), dw, dh, **kw)


def frame_size(w, h, layout, dtype):
    """vp8hip_rgb_size for good parameters"""
    return w * h * (4 if layout == "packed4" else 3) * np.dtype(NP_DTYPES[dtype]).itemsize
