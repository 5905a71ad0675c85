"""What the numpy restatements of the calls that write tensors of int16 values share (side_reference.py, residual_reference.py): the
element types, the map from an output grid onto what it is laid over, and the conversion of the values.  Nothing here knows how
the kernels go about it."""
import numpy as np

DTYPES = {"i16": np.int16, "f16": np.float16, "f32": np.float32}


def grid_map(dst, d):
    """source sample under the centre of each of dst outputs laid over d samples: ((2x + 1) * d) // (2 * dst)"""
    x = np.arange(dst, dtype=np.int64)
    return ((2 * x + 1) * d) // (2 * dst)


def convert(v, dtype, scale):
    """int16 -> the tensor's type: the value, or float32(float64(v) * float64(float32(scale))), or that rounded to a half.  scale: one
    number, or one per leading index of v (the channels of [C, ...])"""
    if dtype == "i16":
        return v.astype(np.int16)
    s = np.asarray(scale, np.float32).astype(np.float64)
    f = (v.astype(np.float64) * s.reshape(s.shape + (1,) * (v.ndim - s.ndim))).astype(np.float32)
    if dtype == "f32":
        return f
    with np.errstate(over="ignore"):             # (beyond the halves' range: infinity)
        return f.astype(np.float16)
