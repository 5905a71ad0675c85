"""The definition of vp8hip_frames_subpel_async (include/vp8hip.h) a second time, in numpy: the edge-replicated picture, the clamped
start, the two-pass bilinear predictor, the variance in 64 bits, the cost term with its clamped index and the reference's order of
evaluations and strict comparisons.  Nothing here knows how the kernel goes about it.  refine_mb is vp8_find_best_sub_pixel_step
written out evaluation by evaluation; refine does every macroblock of a picture with it (eleven small array operations each).
Also the generator of the pictures the fixture tests/golden/subpel_ref.json was recorded for."""
import numpy as np

from motion_reference import bounds, edge, fixture_centre, pair as motion_pair
from ssim_reference import mixed_bytes

PLANES = {"val": 1, "var": 2, "sse": 4, "var0": 8}
NAMES = tuple(PLANES)


def mask_of(planes):
    return planes if isinstance(planes, int) else sum({PLANES[p] for p in planes})


def pick(stats, planes):
    """the planes of `planes` (names or the mask) of a stats array [4, ...], in bit order"""
    mask = mask_of(planes)
    return stats[[p for p in range(4) if mask >> p & 1]]


def clamp_start(shape, my, mx, x8, y8):
    """the start tensor's (x, y) in 1/8 pel -> (sx, sy) in whole pixels inside the UMV bounds"""
    rmin, rmax, cmin, cmax = bounds(shape, my, mx)
    return min(max(int(x8) >> 3, cmin), cmax), min(max(int(y8) >> 3, rmin), rmax)


def predict(ref, y0, x0, vy, vx):
    """the 16x16 prediction of the block at (y0, x0) at the vector (vy, vx) in 1/8 pel: vp8_sub_pixel_variance16x16_c's two passes"""
    by, bx, oy, ox = vy >> 3, vx >> 3, vy & 7, vx & 7
    win = edge(ref, y0 + by, x0 + bx, 17, 17).astype(np.int64)
    h = (win[:, :16] * (128 - 16 * ox) + win[:, 1:] * (16 * ox) + 64) >> 7
    return (h[:16] * (128 - 16 * oy) + h[1:] * (16 * oy) + 64) >> 7


def dist(blk, pred):
    """(DIST, sse, sum) of a block against a prediction"""
    diff = blk.astype(np.int64) - pred
    sse, s = int((diff * diff).sum()), int(diff.sum())
    return (sse - ((s * s) >> 8)) & 0xffffffff, sse, s


def cost_term(cost, epb, R, vy, vx, ry, rx):
    """mv_err_cost of the vector (vy, vx) counted from (ry, rx), the index clamped to +-R"""
    if cost is None or not epb:
        return 0
    iy = min(max((vy - ry) >> 1, -R), R) + R
    ix = min(max((vx - rx) >> 1, -R), R) + R
    return ((int(cost[0][iy]) + int(cost[1][ix])) * int(epb) + 128) >> 8


def refine_mb(s, ref, my, mx, sx=0, sy=0, rx=0, ry=0, cost=None, epb=0, precision=4, log=None):
    """one macroblock from the whole-pixel start (sx, sy), already clamped -> ((vx, vy), [VAL, VAR, SSE, VAR0]).  log: a list that
    receives (vy, vx, sum, cost index y, cost index x before the clamp) of every evaluation"""
    blk = s[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
    R = None if cost is None else (np.asarray(cost).shape[1] - 1) // 2

    def value(vy, vx):
        var, sse, sm = dist(blk, predict(ref, 16 * my, 16 * mx, vy, vx))
        if log is not None:
            log.append((vy, vx, sm, (vy - ry) >> 1, (vx - rx) >> 1))
        return var + cost_term(cost, epb, R, vy, vx, ry, rx), var, sse, vy, vx
    best = value(8 * sy, 8 * sx)
    var0 = best[1]
    for h in (4, 2)[:1 if precision == 2 else 2]:
        cy, cx = best[3], best[4]
        left, right, up, down = value(cy, cx - h), value(cy, cx + h), value(cy - h, cx), value(cy + h, cx)
        for cand in (left, right, up, down):
            if cand[0] < best[0]:
                best = cand
        diag = value(cy + (-h if up[0] < down[0] else h), cx + (-h if left[0] < right[0] else h))
        if diag[0] < best[0]:
            best = diag
    return (best[4], best[3]), [best[0], best[1], best[2], var0]


def refine(s, ref, start=None, rvec=None, cost=None, epb=0, precision=4, log=None):
    """pictures s, ref (uint8, the coded luma size) -> (mv int16 [2, rows, cols] = (x, y) in 1/8 pel, stats uint32 [4, rows, cols] in
    bit order).  start, rvec: None or integers [2, rows, cols] (x, y) in 1/8 pel"""
    s, ref = np.asarray(s), np.asarray(ref)
    assert s.dtype == np.uint8 and ref.dtype == np.uint8 and s.shape == ref.shape and s.shape[0] % 16 == 0 and s.shape[1] % 16 == 0
    assert precision in (2, 4)
    rows, cols = s.shape[0] // 16, s.shape[1] // 16
    mv, stats = np.zeros((2, rows, cols), np.int16), np.zeros((4, rows, cols), np.uint32)
    for my in range(rows):
        for mx in range(cols):
            sx, sy = clamp_start(s.shape, my, mx, *((0, 0) if start is None else (start[0][my][mx], start[1][my][mx])))
            rx, ry = (0, 0) if rvec is None else (int(rvec[0][my][mx]), int(rvec[1][my][mx]))
            (vx, vy), planes = refine_mb(s, ref, my, mx, sx, sy, rx, ry, cost, epb, precision, log)
            mv[:, my, mx] = (vx, vy)
            stats[:, my, mx] = planes
    return mv, stats


# ---- the pictures of the fixture -----------------------------------------------------------------------------------------------
KINDS = ("noise", "shifted", "flat", "stripes", "smooth", "half", "quarter", "extremes")
SUBSHIFT = {"half": (4, -4), "quarter": (-2, 6)}      # (vy, vx) in 1/8 pel of the two sub-pel kinds


def lowpass(seed, w, h):
    """a smooth picture: noise through a 5x5 box filter twice, in integers"""
    a = mixed_bytes(seed, (w + 16) * (h + 16)).reshape(h + 16, w + 16).astype(np.int64)
    for _ in range(2):
        v = np.lib.stride_tricks.sliding_window_view(a, (5, 5)).sum(axis=(2, 3))
        a = (v + 12) // 25
    # (two passes take 8 off each side) -- stretched to most of the byte range so that the shifts differ
    a = a[:h, :w]
    lo, hi = int(a.min()), int(a.max())
    return ((a - lo) * 220 // max(hi - lo, 1) + 16).astype(np.uint8)


def subshifted(ref, vy, vx):
    """the picture whose every block is the reference's prediction at the vector (vy, vx): the bilinear shift of E(ref)"""
    h, w = ref.shape
    by, bx, oy, ox = vy >> 3, vx >> 3, vy & 7, vx & 7
    win = edge(ref, by, bx, h + 1, w + 1).astype(np.int64)
    hp = (win[:, :w] * (128 - 16 * ox) + win[:, 1:] * (16 * ox) + 64) >> 7
    return ((hp[:h] * (128 - 16 * oy) + hp[1:] * (16 * oy) + 64) >> 7).astype(np.uint8)


def pair(kind, w, h, seed):
    """the picture pair (s, ref), uint8 [h, w] each (w, h multiples of 16), of a fixture case"""
    if kind in SUBSHIFT:
        ref = lowpass(seed, w, h)
        return subshifted(ref, *SUBSHIFT[kind]), ref
    return motion_pair(kind, w, h, seed)


def fixture_cost(R, seed):
    """a cost table int32 [2, 2 R + 1] growing away from the centre, with a little integer noise"""
    i = np.abs(np.arange(2 * R + 1) - R)
    n = mixed_bytes(seed, 2 * (2 * R + 1)).reshape(2, -1).astype(np.int32) % 16
    return (np.stack([i * 11 + 40, i * 9 + 30]) + n).astype(np.int32)


def fixture_start(kind, rows, cols, seed):
    """None ("zero") or integers [2, rows, cols] (x, y) in 1/8 pel: "near" a few pixels around (0, 0) with fractional bits set (they
    are shifted out), "far" beyond the bounds on every side, "bounds" exactly on a UMV bound of each macroblock"""
    if kind == "zero":
        return None
    if kind in ("near", "far"):
        c = fixture_centre(kind, rows, cols, seed)
        return c * 8 + (mixed_bytes(seed + 5, 2 * rows * cols).reshape(2, rows, cols).astype(np.int32) & 7)
    assert kind == "bounds"
    out = np.zeros((2, rows, cols), np.int32)
    pick_ = mixed_bytes(seed, rows * cols).reshape(rows, cols)
    for my in range(rows):
        for mx in range(cols):
            rmin, rmax, cmin, cmax = bounds((16 * rows, 16 * cols), my, mx)
            k = int(pick_[my, mx]) & 3
            out[0, my, mx] = 8 * (cmin if k & 1 else cmax)
            out[1, my, mx] = 8 * (rmin if k & 2 else rmax)
    return out


def fixture_ref(kind, rows, cols, seed):
    """None ("zero") or the reference vectors [2, rows, cols] (x, y) in 1/8 pel, odd values among them"""
    if kind == "zero":
        return None
    return mixed_bytes(seed, 2 * rows * cols).reshape(2, rows, cols).astype(np.int32) % 41 - 20
