"""The definition of vp8hip_frames_ssim_async (include/vp8hip.h) a second time, in numpy: the windows of a plane, a window's five sums
in int64, n and d, v = float64(n) / float64(d), the Q32 totals, the F32 / F16 maps, and the mean summed in raster order as vp8_ssim2
(vp8/encoder/ssim.c) sums it.  Nothing here knows how the kernel goes about it.  Also the generator of the planes the fixture
tests/golden/ssim_ref.json was recorded for: integer mixing written out here, not numpy's Generator, whose streams are not promised
across versions."""
import numpy as np

PLANES = {"y": 1, "u": 2, "v": 4}
C1, C2 = 26634, 239708                            # similarity() with count 64
Q = 4294967296.0                                  # 2^32


def mask_of(planes):
    return planes if isinstance(planes, int) else sum({PLANES[p] for p in planes})


def windows(pw, ph):
    """(nwx, nwy) of a plane of pw x ph: top left corners 4 * wx < pw - 8 and 4 * wy < ph - 8"""
    return ((pw - 5) // 4 if pw > 8 else 0), ((ph - 5) // 4 if ph > 8 else 0)


def loop_windows(pw, ph):
    """the same by counting vp8_ssim2's loop"""
    return len(range(0, max(pw - 8, 0), 4)), len(range(0, max(ph - 8, 0), 4))


def n_d(s, r):
    """planes s, r (uint8 [ph, pw]) -> (n, d): int64 [nwy, nwx] each ([0, 0] where the plane has no windows)"""
    s, r = np.asarray(s), np.asarray(r)
    assert s.dtype == np.uint8 and r.dtype == np.uint8 and s.shape == r.shape and s.ndim == 2
    nwx, nwy = windows(s.shape[1], s.shape[0])
    if not nwx or not nwy:
        z = np.zeros((0, 0), np.int64)
        return z, z

    def sums(a):
        v = np.lib.stride_tricks.sliding_window_view(a, (8, 8))[::4, ::4][:nwy, :nwx]
        return v.sum(axis=(2, 3), dtype=np.int64)
    a, b = s.astype(np.int64), r.astype(np.int64)
    ss, sr, sss, srr, ssr = sums(a), sums(b), sums(a * a), sums(b * b), sums(a * b)
    n = (2 * ss * sr + C1) * (2 * 64 * ssr - 2 * ss * sr + C2)
    d = (ss * ss + sr * sr + C1) * (64 * sss - ss * ss + 64 * srr - sr * sr + C2)
    return n, d


def values(s, r):
    """the window values, float64 [nwy, nwx]: both conversions round to nearest, the division is IEEE's"""
    n, d = n_d(s, r)
    return n.astype(np.float64) / d.astype(np.float64)


def q32(v):
    """window values -> int64: llrint(v * 2^32), half to even (np.rint); the product is exact"""
    return np.rint(np.asarray(v, np.float64) * Q).astype(np.int64)


def plane_scores(s, r):
    """(total, count) of one plane pair, Python ints"""
    v = values(s, r)
    return int(q32(v).sum(dtype=np.int64)), int(v.size)


def scores(a_yuv, b_yuv, planes=7):
    """the planes (y, u, v) of two pictures -> int64 [popcount(planes), 2]"""
    mask = mask_of(planes)
    return np.array([plane_scores(a_yuv[p], b_yuv[p]) for p in range(3) if mask >> p & 1], np.int64).reshape(-1, 2)


def ssim_map(a_yuv, b_yuv, planes=7, dtype="f32"):
    """... -> the flat map: the planes asked for back to back, float32(v), or that rounded to float16"""
    mask = mask_of(planes)
    parts = [values(a_yuv[p], b_yuv[p]).astype(np.float32).ravel() for p in range(3) if mask >> p & 1]
    flat = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return flat if dtype == "f32" else flat.astype(np.float16)


def map_elems(w, h, planes=7):
    mask = mask_of(planes)
    out = 0
    for p in range(3):
        if mask >> p & 1:
            nwx, nwy = windows((w + 1) // 2 if p else w, (h + 1) // 2 if p else h)
            out += nwx * nwy
    return out


def q32_mean(s, r):
    """the mean the scores give: total / 2^32 / count (NaN without windows)"""
    total, count = plane_scores(s, r)
    return float(total) / Q / count if count else float("nan")


def raster_mean(s, r):
    """vp8_ssim2: the window values added one by one in raster order, in double, then divided by their number (NaN: 0 / 0)"""
    v = values(s, r)
    total = 0.0
    for x in v.ravel().tolist():
        total += x
    return total / v.size if v.size else float("nan")


# ---- the planes of the fixture -------------------------------------------------------------------------------------------------
def mixed_bytes(seed, n):
    """n bytes from a seed: the top byte of splitmix64's output function over seed * 2^32 + i, in wrapping uint64 arithmetic"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + (np.uint64(seed) << np.uint64(32))) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(56)).astype(np.uint8)


KINDS = ("noise", "perturbed", "identical", "extremes", "antiphase", "one_sample")


def pair(kind, w, h, seed):
    """the plane pair (s, r), uint8 [h, w] each, of a fixture case"""
    a = mixed_bytes(seed, w * h).reshape(h, w)
    if kind == "noise":
        return a, mixed_bytes(seed + 1000, w * h).reshape(h, w)
    if kind == "perturbed":                       # a smooth picture and the same with a few levels of noise on it
        yy, xx = np.mgrid[0:h, 0:w]
        base = ((xx * 3 + yy * 5) % 256).astype(np.int64)
        return base.astype(np.uint8), np.clip(base + (a.astype(np.int64) % 7) - 3, 0, 255).astype(np.uint8)
    if kind == "identical":
        return a, a.copy()
    if kind == "extremes":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if kind == "antiphase":                       # checkerboards of 0 and 255, one against its inverse
        yy, xx = np.mgrid[0:h, 0:w]
        c = (((xx + yy) & 1) * 255).astype(np.uint8)
        return c, (255 - c).astype(np.uint8)
    if kind == "one_sample":
        b = a.copy()
        b[h // 2, w // 2] ^= 0x80
        return a, b
    raise ValueError(kind)
