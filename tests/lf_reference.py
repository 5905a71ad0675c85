"""A plain restatement of the VP8 loop filter's per-line arithmetic (vp8/common/loopfilter_filters.c) and of its limits
(loopfilter.c:24-96), vectorised with numpy in int32 / int64 -- the yardstick of the packed filters of the lane-per-row kernels
(csrc/hip/vp8_simt_prims.hip.h), which work on biased signed 8.8 pairs.  Nothing here is clever: signed char clamps are
written as clamps, the masks as the reference's comparisons.

A line is the 8 pixels across one edge, p3 p2 p1 p0 q0 q1 q2 q3 (columns 0..7 of an (N, 8) array); the limits are per line.
Also the line generators the tests share: corner lines at the limits, lines on the masks' boundaries, black and white."""
import numpy as np

KINDS = ("mbedge", "inner", "simple_mb", "simple_b")       # the `kind` byte of vp8hip_lane_loop_filter_lines


def sclamp(t):
    """vp8_signed_char_clamp"""
    return np.clip(t, -128, 127)


def _cols(lines):
    L = np.asarray(lines).astype(np.int32)
    return [L[:, k] for k in range(8)]


def filter_mask(limit, blimit, lines):
    """vp8_filter_mask: -1 where the edge is filtered, 0 where not"""
    p3, p2, p1, p0, q0, q1, q2, q3 = _cols(lines)
    m = ((np.abs(p3 - p2) > limit) | (np.abs(p2 - p1) > limit) | (np.abs(p1 - p0) > limit)
         | (np.abs(q1 - q0) > limit) | (np.abs(q2 - q1) > limit) | (np.abs(q3 - q2) > limit)
         | (np.abs(p0 - q0) * 2 + np.abs(p1 - q1) // 2 > blimit))
    return np.where(m, 0, -1).astype(np.int32)


def hevmask(thresh, lines):
    """vp8_hevmask: -1 where the edge has high variance"""
    _, _, p1, p0, q0, q1, _, _ = _cols(lines)
    return np.where((np.abs(p1 - p0) > thresh) | (np.abs(q1 - q0) > thresh), -1, 0).astype(np.int32)


def simple_mask(blimit, lines):
    """vp8_simple_filter_mask"""
    _, _, p1, p0, q0, q1, _, _ = _cols(lines)
    return np.where(np.abs(p0 - q0) * 2 + np.abs(p1 - q1) // 2 <= blimit, -1, 0).astype(np.int32)


def _signed(lines):
    """the pixels as the reference's signed chars: (signed char)(u ^ 0x80) == u - 128"""
    return [c - 128 for c in _cols(lines)]


def _out(lines, **changed):
    out = np.array(lines, dtype=np.uint8, copy=True)
    for k, v in changed.items():
        out[:, "p3 p2 p1 p0 q0 q1 q2 q3".split().index(k)] = (v.astype(np.int32) + 128).astype(np.uint8)
    return out


def loop_filter(lines, blimit, limit, thresh):
    """vp8_loop_filter_c's per-line body (vp8_filter_mask, vp8_hevmask, vp8_filter): inner edges, changes p1 p0 q0 q1"""
    mask, hev = filter_mask(limit, blimit, lines), hevmask(thresh, lines)
    _, _, ps1, ps0, qs0, qs1, _, _ = _signed(lines)
    f = sclamp(ps1 - qs1) & hev
    f = sclamp(f + 3 * (qs0 - ps0)) & mask
    f1 = sclamp(f + 4) >> 3
    f2 = sclamp(f + 3) >> 3
    q0n = sclamp(qs0 - f1)
    p0n = sclamp(ps0 + f2)
    f = ((f1 + 1) >> 1) & ~hev
    q1n = sclamp(qs1 - f)
    p1n = sclamp(ps1 + f)
    return _out(lines, p1=p1n, p0=p0n, q0=q0n, q1=q1n)


def mbloop_filter(lines, blimit, limit, thresh):
    """vp8_mbloop_filter_c's per-line body (vp8_filter_mask, vp8_hevmask, vp8_mbfilter): macroblock edges, changes p2..q2"""
    mask, hev = filter_mask(limit, blimit, lines), hevmask(thresh, lines)
    _, ps2, ps1, ps0, qs0, qs1, qs2, _ = _signed(lines)
    f = sclamp(ps1 - qs1)
    f = sclamp(f + 3 * (qs0 - ps0)) & mask
    f2 = f & hev
    f1 = sclamp(f2 + 4) >> 3
    f2 = sclamp(f2 + 3) >> 3
    qs0 = sclamp(qs0 - f1)
    ps0 = sclamp(ps0 + f2)
    f = f & ~hev
    u = sclamp((63 + f * 27) >> 7)
    q0n, p0n = sclamp(qs0 - u), sclamp(ps0 + u)
    u = sclamp((63 + f * 18) >> 7)
    q1n, p1n = sclamp(qs1 - u), sclamp(ps1 + u)
    u = sclamp((63 + f * 9) >> 7)
    q2n, p2n = sclamp(qs2 - u), sclamp(ps2 + u)
    return _out(lines, p2=p2n, p1=p1n, p0=p0n, q0=q0n, q1=q1n, q2=q2n)


def simple_filter(lines, blimit):
    """vp8_loop_filter_simple_{horizontal,vertical}_edge_c's per-line body: changes p0 q0"""
    mask = simple_mask(blimit, lines)
    _, _, p1, p0, q0, q1, _, _ = _signed(lines)
    f = sclamp(p1 - q1)
    f = sclamp(f + 3 * (q0 - p0)) & mask
    f1 = sclamp(f + 4) >> 3
    q0n = sclamp(q0 - f1)
    f2 = sclamp(f + 3) >> 3
    p0n = sclamp(p0 + f2)
    return _out(lines, p0=p0n, q0=q0n)


def filter_kind(lines, kind, mblim, blim, lim, thr, gate=None):
    """each line through the filter of its kind (KINDS), with the macroblock-edge or the inner-edge limit as the kind says;
    lines whose gate is 0 come back unchanged"""
    lines = np.asarray(lines, dtype=np.uint8)
    kind = np.broadcast_to(kind, len(lines))
    out = lines.copy()
    for k, fn in enumerate((lambda L, s: mbloop_filter(L, mblim[s], lim[s], thr[s]), lambda L, s: loop_filter(L, blim[s], lim[s], thr[s]),
                            lambda L, s: simple_filter(L, mblim[s]), lambda L, s: simple_filter(L, blim[s]))):
        sel = np.nonzero(kind == k)[0]
        if sel.size:
            out[sel] = fn(lines[sel], sel)
    if gate is not None:
        out[gate == 0] = lines[gate == 0]
    return out


# ---- limits ----

def lf_limits(sharpness, level, frame_type):
    """vp8_loop_filter_update_sharpness (loopfilter.c:66-96) and lf_init_lut's hev thresholds (:24-50): (mblim, blim, lim, hev_thr)
    as the reference's unsigned chars"""
    ilimit = level >> (1 if sharpness > 0 else 0)
    ilimit >>= 1 if sharpness > 4 else 0
    if sharpness > 0 and ilimit > 9 - sharpness:
        ilimit = 9 - sharpness
    ilimit = max(ilimit, 1)
    if level >= 40:
        thr = 2 if frame_type == 0 else 3
    elif level >= 20:
        thr = 1 if frame_type == 0 else 2
    elif level >= 15:
        thr = 1
    else:
        thr = 0
    return (2 * (level + 2) + ilimit) & 0xff, (2 * level + ilimit) & 0xff, ilimit, thr


def limits_table():
    """every (sharpness, level, frame type): an int32 array of rows sharpness, level, frame_type, mblim, blim, lim, hev_thr"""
    rows = [(s, l, t) + lf_limits(s, l, t) for s in range(8) for l in range(64) for t in range(2)]
    return np.array(rows, dtype=np.int32)


# ---- line generators ----

def _place(rng, rel):
    """relative lines (N, 8) shifted by a random offset into 0..255 where they fit, clipped where they do not"""
    lo, hi = rel.min(axis=1), rel.max(axis=1)
    span = hi - lo
    off = -lo + (rng.random(len(rel)) * np.maximum(255 - span + 1, 1)).astype(np.int64)
    return np.clip(rel + off[:, None], 0, 255).astype(np.uint8)


def _outer(rng, n, lim, past=0.15):
    """p3 - p2 ... offsets: the interior limit, one past it with probability `past`, either sign"""
    mag = lim + (rng.random(n) < past)
    return mag * rng.choice((-1, 1), size=n)


def corner_lines(rng, lim, thr, p0q0=None):
    """For every (p0, q0) in 256^2 (or the pairs given; lim / thr scalars or one per pair), 12 choices of (p1, q1): at +-lim, +-(lim + 1), +-thr, +-(thr + 1) from
    p0 / q0, and the four pairs of extremes 0 / 255.  p2, p3, q2, q3 at the interior limit from their neighbours or one past it.
    Returns (N, 8) uint8, N = 12 * pairs: line c * pairs + j is choice c of pair j."""
    if p0q0 is None:
        p0, q0 = [a.ravel() for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    else:
        p0, q0 = p0q0
    p0, q0 = np.asarray(p0, np.int64), np.asarray(q0, np.int64)
    lim, thr = np.broadcast_to(lim, p0.shape).astype(np.int64), np.broadcast_to(thr, p0.shape).astype(np.int64)
    offs = [(lim, -lim), (-lim, lim), (lim + 1, -(lim + 1)), (-(lim + 1), lim),
            (thr, -thr), (-thr, thr + 1), (thr + 1, -(thr + 1)), (-(thr + 1), thr)]
    ext = [(0, 255), (255, 0), (0, 0), (255, 255)]
    parts = []
    for dp, dq in offs:
        parts.append(np.stack([p0 + dp, q0 + dq], axis=1))
    for a, b in ext:
        parts.append(np.stack([np.full_like(p0, a), np.full_like(q0, b)], axis=1))
    pq1 = np.clip(np.concatenate(parts), 0, 255)
    P0, Q0 = np.tile(p0, 12), np.tile(q0, 12)
    n = len(P0)
    lim = np.tile(lim, 12)
    p1, q1 = pq1[:, 0], pq1[:, 1]
    p2 = p1 + _outer(rng, n, lim)
    p3 = p2 + _outer(rng, n, lim)
    q2 = q1 + _outer(rng, n, lim)
    q3 = q2 + _outer(rng, n, lim)
    return np.clip(np.stack([p3, p2, p1, P0, Q0, q1, q2, q3], axis=1), 0, 255).astype(np.uint8)


def boundary_lines(rng, lim, elim, thr):
    """Random lines, one per entry of the per-line limits, each built on one boundary of the masks, on a random side of it:
    2|p0 - q0| + |p1 - q1| / 2 == elim (+1), one of the six differences the mask limits == lim (+1), or
    max(|p1 - p0|, |q1 - q0|) == thr (+1); the other differences inside their limits.  Returns (N, 8) uint8."""
    lim, elim, thr = (np.asarray(a, np.int64) for a in (lim, elim, thr))
    n = len(lim)
    sign = lambda: rng.choice((-1, 1), size=n)
    uni = lambda m: (rng.random(n) * (m + 1)).astype(np.int64) * sign()          # uniform in [-m, m] (zero twice as rare)
    side = rng.integers(0, 2, size=n)
    target = rng.integers(0, 3, size=n)
    # differences along the line: p3->p2, p2->p1, p1->p0, p0->q0, q0->q1, q1->q2, q2->q3
    d = np.stack([uni(lim), uni(lim), uni(lim), uni(np.maximum(elim // 6, 0)), uni(lim), uni(lim), uni(lim)], axis=1)
    r = np.arange(n)
    # one of the six limited differences on the limit
    t = target == 1
    which = rng.choice((0, 1, 2, 4, 5, 6), size=n)
    d[r[t], which[t]] = ((lim + side) * sign())[t]
    # the hev boundary on one side; the other side inside
    t = target == 2
    hs = rng.choice((2, 4), size=n)
    inner = np.minimum(thr, lim)
    d[r[t], 2] = uni(inner)[t]
    d[r[t], 4] = uni(inner)[t]
    d[r[t], hs[t]] = ((thr + side) * sign())[t]
    # the edge limit: d0 = |p0 - q0|, D = |p1 - q1| with 2 d0 + D // 2 == elim + side, p1 / q1 within lim of p0 / q0
    t = np.nonzero(target == 0)[0]
    e = (elim + side)[t]
    tries = 64
    d0 = rng.integers(0, 128, size=(len(t), tries))
    D = 2 * (e[:, None] - 2 * d0) + rng.integers(0, 2, size=(len(t), tries))
    ok = (D >= 0) & (D <= 255) & (np.abs(D - d0) <= 2 * lim[t, None])
    pick = np.argmax(ok, axis=1)
    found = ok[np.arange(len(t)), pick]
    d0, D = d0[np.arange(len(t)), pick], D[np.arange(len(t)), pick]
    # p1 = p0 - s a, q1 = q0 + s b with a + b = D - d0, |a|, |b| <= lim
    rest = D - d0
    lt = lim[t]
    a = np.clip((rng.random(len(t)) * (2 * lt + 1)).astype(np.int64) - lt, np.maximum(-lt, rest - lt), np.minimum(lt, rest + lt))
    b = rest - a
    s = rng.choice((-1, 1), size=len(t))
    keep = t[found]
    d[keep, 2] = (s * a)[found]
    d[keep, 3] = (s * d0)[found]
    d[keep, 4] = (s * b)[found]
    rel = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(d, axis=1)], axis=1)
    return _place(rng, rel)


def boundary_hits(lines, lim, elim, thr):
    """which boundaries a set of lines meets, decisively (the other conditions of the mask pass): counts of lines with
    e == elim, e == elim + 1, max outer difference == lim, == lim + 1, max(|p1 - p0|, |q1 - q0|) == thr, == thr + 1"""
    p3, p2, p1, p0, q0, q1, q2, q3 = _cols(lines)
    e = np.abs(p0 - q0) * 2 + np.abs(p1 - q1) // 2
    outer = np.max(np.abs(np.stack([p3 - p2, p2 - p1, p1 - p0, q1 - q0, q2 - q1, q3 - q2])), axis=0)
    h = np.maximum(np.abs(p1 - p0), np.abs(q1 - q0))
    on = (outer <= lim) & (e <= elim)
    return {"elim": int(((e == elim) & (outer <= lim)).sum()), "elim+1": int(((e == elim + 1) & (outer <= lim)).sum()),
            "lim": int(((outer == lim) & (e <= elim)).sum()), "lim+1": int(((outer == lim + 1) & (e <= elim)).sum()),
            "thr": int(((h == thr) & on).sum()), "thr+1": int(((h == thr + 1) & on).sum())}


def black_white_lines():
    """the 256 lines of 0 / 255 pixels"""
    k = np.arange(256)
    return (((k[:, None] >> np.arange(8)[None, :]) & 1) * 255).astype(np.uint8)
