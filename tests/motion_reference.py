"""The definition of vp8hip_frames_motion_async (include/vp8hip.h) a second time, in numpy: the edge-replicated picture, the UMV
bounds, the clamped centre, the candidates in the reference's order with its strict <, the cost term and the five planes.  Nothing
here knows how the kernel goes about it.  search_mb_loop is vp8_full_search_sad_c's loop written out candidate by candidate (slow:
small distances only), search_mb the same answer by array operations.  Also the generator of the pictures the fixture
tests/golden/motion_ref.json was recorded for (integer mixing, ssim_reference.mixed_bytes)."""
import numpy as np

from ssim_reference import mixed_bytes

PLANES = {"sad": 1, "sad0": 2, "sse": 4, "var": 8, "srcvar": 16}
NAMES = tuple(PLANES)
BORDER = 16                                       # VP8BORDERINPIXELS - 16


def mask_of(planes):
    return planes if isinstance(planes, int) else sum({PLANES[p] for p in planes})


def edge(S, y0, x0, h, w):
    """E(S) over rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1: S with its coordinates clamped to the picture"""
    rows = np.clip(np.arange(y0, y0 + h), 0, S.shape[0] - 1)
    cols = np.clip(np.arange(x0, x0 + w), 0, S.shape[1] - 1)
    return S[np.ix_(rows, cols)]


def bounds(shape, my, mx):
    """(rmin, rmax, cmin, cmax) of macroblock (my, mx) of a picture of `shape` (coded luma)"""
    rows, cols = shape[0] // 16, shape[1] // 16
    return -(16 * my + BORDER), 16 * (rows - 1 - my) + BORDER, -(16 * mx + BORDER), 16 * (cols - 1 - mx) + BORDER


def clamp_centre(shape, my, mx, cx, cy):
    rmin, rmax, cmin, cmax = bounds(shape, my, mx)
    return min(max(int(cx), cmin), cmax), min(max(int(cy), rmin), rmax)


def cost_term(cost, spb, ri, ci):
    """mvsad_err_cost at row index ri = r - cy + d and column index ci = c - cx + d (scalars or arrays)"""
    if cost is None or not spb:
        return 0 * (ri + ci)
    cost = np.asarray(cost, np.int64)
    return ((cost[0][ri] + cost[1][ci]) * int(spb) + 128) >> 8


def variance(a, b):
    """(sse, var) of two 16x16 blocks: vp8_variance16x16_c with the product in 64 bits"""
    diff = a.astype(np.int64) - b.astype(np.int64)
    sse, s = int((diff * diff).sum()), int(diff.sum())
    return sse, (sse - ((s * s) >> 8)) & 0xffffffff


def _planes_at(s, ref, my, mx, r, c, value):
    blk = s[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
    sse, var = variance(blk, edge(ref, 16 * my + r, 16 * mx + c, 16, 16))
    sad0 = int(np.abs(blk.astype(np.int64) - ref[16 * my:16 * my + 16, 16 * mx:16 * mx + 16].astype(np.int64)).sum())
    return [int(value), sad0, sse, var, variance(blk, np.full((16, 16), 128, np.uint8))[1]]


def search_mb_loop(s, ref, my, mx, d, cx=0, cy=0, cost=None, spb=0):
    """one macroblock, candidate by candidate as the reference walks them -> ((c_best, r_best), the five planes)"""
    rmin, rmax, cmin, cmax = bounds(s.shape, my, mx)
    cx, cy = clamp_centre(s.shape, my, mx, cx, cy)
    blk = s[16 * my:16 * my + 16, 16 * mx:16 * mx + 16].astype(np.int64)

    def value(r, c):
        sad = int(np.abs(blk - edge(ref, 16 * my + r, 16 * mx + c, 16, 16).astype(np.int64)).sum())
        return sad + int(cost_term(cost, spb, r - cy + d, c - cx + d))
    best, at = value(cy, cx), (cy, cx)
    for r in range(max(cy - d, rmin), min(cy + d, rmax)):
        for c in range(max(cx - d, cmin), min(cx + d, cmax)):
            v = value(r, c)
            if v < best:
                best, at = v, (r, c)
    return (at[1], at[0]), _planes_at(s, ref, my, mx, at[0], at[1], best)


def search_mb(s, ref, my, mx, d, cx=0, cy=0, cost=None, spb=0):
    """the same, all candidates at once"""
    rmin, rmax, cmin, cmax = bounds(s.shape, my, mx)
    cx, cy = clamp_centre(s.shape, my, mx, cx, cy)
    blk = s[16 * my:16 * my + 16, 16 * mx:16 * mx + 16].astype(np.int32)
    win = edge(ref, 16 * my + cy - d, 16 * mx + cx - d, 2 * d + 16, 2 * d + 16).astype(np.int32)
    views = np.lib.stride_tricks.sliding_window_view(win, (16, 16))[:2 * d, :2 * d]
    idx = np.arange(2 * d)
    value = np.abs(views - blk).sum(axis=(2, 3), dtype=np.int64) + cost_term(cost, spb, idx[:, None], idx[None, :])
    r, c = cy - d + idx, cx - d + idx
    visited = ((r >= rmin) & (r < rmax))[:, None] & ((c >= cmin) & (c < cmax))[None, :]
    loop = np.where(visited, value, np.iinfo(np.int64).max).ravel()
    k = int(np.argmin(loop))                      # the first of the smallest, in raster order
    centre = int(value[d, d])                     # valued first, visited or not
    ri, ci = (k // (2 * d), k % (2 * d)) if loop[k] < centre else (d, d)
    return (int(c[ci]), int(r[ri])), _planes_at(s, ref, my, mx, int(r[ri]), int(c[ci]), min(int(loop[k]), centre))


def search(s, ref, d, centre=None, cost=None, spb=0, mb=search_mb):
    """pictures s, ref (uint8, the coded luma size) -> (mv int16 [2, rows, cols] = (c_best << 3, r_best << 3), stats uint32
    [5, rows, cols] in bit order).  centre: None or integers [2, rows, cols] (x, y)"""
    s, ref = np.asarray(s), np.asarray(ref)
    assert s.dtype == np.uint8 and ref.dtype == np.uint8 and s.shape == ref.shape and s.shape[0] % 16 == 0 and s.shape[1] % 16 == 0
    rows, cols = s.shape[0] // 16, s.shape[1] // 16
    mv, stats = np.zeros((2, rows, cols), np.int16), np.zeros((5, rows, cols), np.uint32)
    for my in range(rows):
        for mx in range(cols):
            cx, cy = (0, 0) if centre is None else (int(centre[0][my][mx]), int(centre[1][my][mx]))
            (c, r), planes = mb(s, ref, my, mx, d, cx, cy, cost, spb)
            mv[:, my, mx] = (c << 3, r << 3)
            stats[:, my, mx] = planes
    return mv, stats


def pick(stats, planes):
    """the planes of `planes` (names or the mask) of a stats array [5, ...], in bit order"""
    mask = mask_of(planes)
    return stats[[p for p in range(5) if mask >> p & 1]]


# ---- the pictures of the fixture -----------------------------------------------------------------------------------------------
KINDS = ("noise", "shifted", "flat", "stripes", "smooth", "extremes")
SHIFT = (3, -2)                                   # (dy, dx) of "shifted": s(y, x) = E(ref)(y + dy, x + dx)


def shifted(ref, dy, dx):
    return np.ascontiguousarray(edge(ref, dy, dx, ref.shape[0], ref.shape[1]))


def pair(kind, w, h, seed):
    """the picture pair (s, ref), uint8 [h, w] each (w, h multiples of 16), of a fixture case"""
    a = mixed_bytes(seed, w * h).reshape(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return a, mixed_bytes(seed + 1000, w * h).reshape(h, w)
    if kind == "shifted":                         # the block's content lies SHIFT away in ref
        return shifted(a, *SHIFT), a
    if kind == "flat":
        return np.full((h, w), 90, np.uint8), np.full((h, w), 97, np.uint8)
    if kind == "stripes":                         # vertical stripes of period 4: every fourth column ties
        st = ((xx % 4) * 60 + 20).astype(np.uint8)
        return st, st.copy()
    if kind == "smooth":                          # a slow ramp under a few levels of noise, the other picture moved by (1, 2)
        base = ((xx * 5 + yy * 3) // 2 % 256).astype(np.int64)
        ref = np.clip(base + a.astype(np.int64) % 5, 0, 255).astype(np.uint8)
        return np.clip(shifted(ref, 1, 2).astype(np.int64) + (a.astype(np.int64) >> 6) - 1, 0, 255).astype(np.uint8), ref
    if kind == "extremes":                        # |sum| = 65280: past the reference's int product (VAR is not compared there)
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    raise ValueError(kind)


def fixture_cost(d, seed):
    """a cost table int32 [2, 2 d + 1] growing away from the centre, with a little integer noise"""
    i = np.abs(np.arange(2 * d + 1) - d)
    n = mixed_bytes(seed, 2 * (2 * d + 1)).reshape(2, -1).astype(np.int32) % 16
    return (np.stack([i * 37, i * 29]) + n).astype(np.int32)


def fixture_centre(kind, rows, cols, seed):
    """None ("zero") or integers [2, rows, cols]: "near" a few pixels around (0, 0), "far" beyond the bounds on every side"""
    if kind == "zero":
        return None
    b = mixed_bytes(seed, 2 * rows * cols).reshape(2, rows, cols).astype(np.int32)
    return (b % 9 - 4) if kind == "near" else (b - 128) * 3
