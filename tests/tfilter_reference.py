"""The definition of vp8hip_frames_tfilter_async (include/vp8hip.h) a second time, in numpy: the edge-replicated planes, the base and
the offsets of a vector with arithmetic shifts, the chroma vector, the two-pass six-tap and bilinear predictors, the weight from
the error, the blend and the normalisation.  Nothing here knows how the kernel goes about it.  Also the generator of the pictures,
vectors and errors the fixture tests/golden/tfilter_ref.json was recorded for."""
import numpy as np

from motion_reference import edge
from ssim_reference import mixed_bytes

FILTERS = ("sixtap", "bilinear")
SIXTAP = np.array([[0, 0, 128, 0, 0, 0], [0, -6, 123, 12, -1, 0], [2, -11, 108, 36, -8, 1], [0, -9, 93, 50, -6, 0], [3, -16, 77, 77, -16, 3],
                   [0, -6, 50, 93, -9, 0], [1, -8, 36, 108, -11, 2], [0, -1, 12, 123, -6, 0]], np.int64)      # vp8_sub_pel_filters
THRESH = (10000, 20000)                                 # the reference's THRESH_LOW, THRESH_HIGH


def predict(ref, y0, x0, vy, vx, n, filt):
    """the n x n prediction of the block at (y0, x0) of plane `ref` at the vector (vy, vx) in 1/8 pel of that plane"""
    vy, vx = int(vy), int(vx)
    by, bx, oy, ox = vy >> 3, vx >> 3, vy & 7, vx & 7
    if not (oy | ox):
        return edge(ref, y0 + by, x0 + bx, n, n).astype(np.int64)
    if filt == "sixtap":
        win = edge(ref, y0 + by - 2, x0 + bx - 2, n + 5, n + 5).astype(np.int64)
        h = sum(win[:, t:t + n] * SIXTAP[ox][t] for t in range(6))
        h = np.clip((h + 64) >> 7, 0, 255)
        p = sum(h[t:t + n] * SIXTAP[oy][t] for t in range(6))
        return np.clip((p + 64) >> 7, 0, 255)
    assert filt == "bilinear"
    win = edge(ref, y0 + by, x0 + bx, n + 1, n + 1).astype(np.int64)
    h = (win[:, :n] * (128 - 16 * ox) + win[:, 1:] * (16 * ox) + 64) >> 7
    return (h[:n] * (128 - 16 * oy) + h[1:] * (16 * oy) + 64) >> 7


def weight(err, thresh=THRESH):
    """2, 1 or 0 from an error, compared unsigned"""
    e = int(err) & 0xffffffff
    return 2 if e < thresh[0] else 1 if e < thresh[1] else 0


def modifier(s, q, strength, w):
    """the per-pixel weight of a prediction q against the centre s"""
    d = s.astype(np.int64) - q
    m = (d * d * 3 + ((1 << (strength - 1)) if strength else 0)) >> strength
    return (16 - np.minimum(m, 16)) * w


def normalise(acc, cnt):
    """cpi->fixed_divide: ((acc + (cnt >> 1)) * (0x80000 / cnt)) >> 19 in uint32, the low byte; 0 where cnt is 0"""
    div = np.where(cnt > 0, 0x80000 // np.maximum(cnt, 1), 0)
    return ((((acc + (cnt >> 1)) * div) & 0xffffffff) >> 19) & 0xff


def tfilter_planes(centre, sources, mvs=None, errs=None, strength=3, filt="sixtap", thresh=THRESH):
    """centre: the coded planes (y, u, v) of the centre picture; sources: a list of such; mvs: None or per source None or integers
    [2, rows, cols] (x, y) in 1/8 pel; errs: None or per source None or [rows, cols] -> (the three filtered coded planes uint8, the
    three count planes uint16)"""
    assert 0 <= strength <= 6 and filt in FILTERS and 1 <= len(sources) <= 15
    rows, cols = centre[0].shape[0] // 16, centre[0].shape[1] // 16
    acc = [np.zeros(p.shape, np.int64) for p in centre]
    cnt = [np.zeros(p.shape, np.int64) for p in centre]
    for k, src in enumerate(sources):
        mv = None if mvs is None else mvs[k]
        err = None if errs is None else errs[k]
        for my in range(rows):
            for mx in range(cols):
                w = 2 if err is None else weight(err[my][mx], thresh)
                if not w:
                    continue
                vx, vy = (0, 0) if mv is None else (int(mv[0][my][mx]), int(mv[1][my][mx]))
                for pl in range(3):
                    n = 8 if pl else 16
                    py, px = (vy >> 1, vx >> 1) if pl else (vy, vx)
                    q = predict(src[pl], n * my, n * mx, py, px, n, filt)
                    at = (slice(n * my, n * my + n), slice(n * mx, n * mx + n))
                    m = modifier(centre[pl][at], q, strength, w)
                    cnt[pl][at] += m
                    acc[pl][at] += m * q
    assert all(int(c.max()) <= 480 for c in cnt)
    return [normalise(a, c).astype(np.uint8) for a, c in zip(acc, cnt)], [c.astype(np.uint16) for c in cnt]


def pack(planes, w, h):
    """coded planes (y, u, v) -> the packed I420 layout at the display size w x h"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return np.concatenate([planes[0][:h, :w].ravel(), planes[1][:ch, :cw].ravel(), planes[2][:ch, :cw].ravel()])


def tfilter(centre, sources, mvs=None, errs=None, strength=3, filt="sixtap", thresh=THRESH, display=None):
    """-> (the picture, packed I420 uint8, and its count, uint16, at the display size (w, h); default: the coded size)"""
    pic, cnt = tfilter_planes(centre, sources, mvs, errs, strength, filt, thresh)
    h, w = centre[0].shape if display is None else (display[1], display[0])
    return pack(pic, w, h), pack(cnt, w, h)


# ---- the pictures, vectors and errors of the fixture -------------------------------------------------------------------------------
def lowpass_plane(seed, w, h):
    """a smooth plane: noise through a 5x5 box filter twice, in integers, stretched over most of the byte range"""
    a = mixed_bytes(seed, (w + 16) * (h + 16)).reshape(h + 16, w + 16).astype(np.int64)
    for _ in range(2):
        a = (np.lib.stride_tricks.sliding_window_view(a, (5, 5)).sum(axis=(2, 3)) + 12) // 25
    a = a[:h, :w]
    lo, hi = int(a.min()), int(a.max())
    return ((a - lo) * 220 // max(hi - lo, 1) + 16).astype(np.uint8)


def picture(kind, w, h, seed):
    """coded planes (y, u, v) of w x h (multiples of 16): "noise", "smooth", or "flat<value>" """
    cw, ch = w // 2, h // 2
    if kind == "noise":
        return [mixed_bytes(seed, w * h).reshape(h, w), mixed_bytes(seed + 1, cw * ch).reshape(ch, cw), mixed_bytes(seed + 2, cw * ch).reshape(ch, cw)]
    if kind == "smooth":
        return [lowpass_plane(seed, w, h), lowpass_plane(seed + 1, cw, ch), lowpass_plane(seed + 2, cw, ch)]
    assert kind.startswith("flat")
    v = int(kind[4:])
    return [np.full((h, w), v, np.uint8), np.full((ch, cw), v, np.uint8), np.full((ch, cw), v, np.uint8)]


def noisy(planes, seed, amp):
    """the picture plus integer noise of -amp .. amp, clipped: a neighbouring picture of a sequence"""
    out = []
    for k, p in enumerate(planes):
        n = mixed_bytes(seed + 7 * k, p.size).reshape(p.shape).astype(np.int64) % (2 * amp + 1) - amp
        out.append(np.clip(p.astype(np.int64) + n, 0, 255).astype(np.uint8))
    return out


def sequence(w, h, seed, count):
    """a centre picture (smooth) and `count` sources: the centre itself first, then noisy copies of growing amplitude, each moved a
    little (by whole pixels, edge-replicated)"""
    centre = picture("smooth", w, h, seed)
    sources = [centre]
    for k in range(1, count):
        n = noisy(centre, seed + 100 * k, 1 + 3 * (k % 6))
        dy, dx = (k % 3) - 1, ((k // 3) % 3) - 1
        sources.append([np.ascontiguousarray(edge(p, dy if i == 0 else dy // 2, dx if i == 0 else dx // 2, p.shape[0], p.shape[1]))
                        for i, p in enumerate(n)])
    return centre, sources


VECTORS = ("zero", "phases", "negodd", "outside", "search")


def fixture_mv(kind, rows, cols, seed, k=0):
    """None ("zero") or vectors [2, rows, cols] (x, y) in 1/8 pel for source k: "phases": every luma phase 0..7 and, through the
    halving, every chroma phase, in both directions, a few pixels around 0; "negodd": negative odd values; "outside": vectors that
    carry the block wholly outside the picture, on every side ("search" is made by the caller from the pictures)"""
    if kind == "zero":
        return None
    b = mixed_bytes(seed + 11 * k, 2 * rows * cols).reshape(2, rows, cols).astype(np.int64)
    i = np.arange(rows * cols).reshape(rows, cols) + k
    if kind == "phases":
        # x walks the sixteen values 0..15 (all luma phases, and after >> 1 all chroma phases) with a whole-pixel part of either sign
        x = (i % 16) + 16 * ((b[0] % 5) - 2)
        y = ((i // 16 + i * 7) % 16) + 16 * ((b[1] % 5) - 2)
        sign = np.where((i + k) % 2 == 0, 1, -1)
        return np.stack([x * sign, y * -sign])
    if kind == "negodd":
        return np.stack([-(2 * (b[0] % 40) + 1), -(2 * (b[1] % 24) + 1)])
    assert kind == "outside"
    far = 8 * (16 * max(rows, cols) + 40)
    pickx, picky = (b[0] % 3) - 1, (b[1] % 3) - 1
    pickx = np.where((pickx == 0) & (picky == 0), 1, pickx)
    return np.stack([pickx * (far + b[1] % 16), picky * (far + b[0] % 16)])


WEIGHTS = ("two", "mixed", "none")


def fixture_err(kind, rows, cols, seed, k=0, thresh=THRESH):
    """None ("two": every weight 2) or an error plane [rows, cols] uint32: "mixed" walks the values on both sides of both thresholds
    (thresh - 1, thresh) and a few others; "none": every weight 0"""
    if kind == "two":
        return None
    if kind == "none":
        return np.full((rows, cols), thresh[1], np.uint32) + (mixed_bytes(seed + k, rows * cols).reshape(rows, cols) % 2).astype(np.uint32) * 5000
    assert kind == "mixed"
    values = np.array([0, thresh[0] - 1, thresh[0], thresh[1] - 1, thresh[1], 2 * thresh[1], 17, thresh[0] + 1], np.uint32)
    i = np.arange(rows * cols).reshape(rows, cols) + 3 * k + seed
    return values[i % len(values)]
