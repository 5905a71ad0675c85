"""GPU: the packed loop filter of the lane-per-row kernels (csrc/hip/vp8_simt_prims.hip.h: masks, add3w, lf_mbedge, lf_inner,
lf_simple, mb_limits, and lf_block_row<2> for chroma) edge by edge at its corners, against tests/lf_reference.py -- the plain
integer restatement of loopfilter_filters.c that tests/test_lf_reference_cpu.py pins to the oracle.

Lines go through vp8hip_lane_loop_filter_lines two to a lane, with the limits derived on the device from (sharpness, level,
frame type), every filter kind mixed in each wave and some edges gated off, as the frame kernels run them.  Every output byte
is compared, the ones the filter must not touch included."""
import ctypes

import numpy as np
import pytest

import lf_reference as R
from vp8_testlib import oracle

pytestmark = pytest.mark.gpu
vp, ci = ctypes.c_void_p, ctypes.c_int
TABLE = R.limits_table()            # rows: sharpness, level, frame type, mblim, blim, lim, hev_thr


class OraLfi(ctypes.Structure):
    _fields_ = [("mblim", ctypes.c_ubyte), ("blim", ctypes.c_ubyte), ("lim", ctypes.c_ubyte), ("hev_thr", ctypes.c_ubyte)]


@pytest.fixture(scope="module")
def L(pkg):
    lib = pkg.load_hip()
    lib.vp8hip_lane_loop_filter_lines.argtypes = [vp, vp, vp, ci]
    lib.vp8hip_lane_loop_filter_chroma_mbs.argtypes = [vp, vp, vp, ci]
    lib.vp8hip_lane_add3w_sweep.argtypes = [vp, vp, ci]
    return lib


def table_row(sharp, level, ftype):
    return (np.asarray(sharp) * 64 + np.asarray(level)) * 2 + np.asarray(ftype)


def lanes(rng, lines, row, kind, closed=0.1):
    """pair consecutive lines into lanes of one limit set (TABLE row) and kind; par bytes per lane, ~`closed` of the gates shut"""
    m = len(lines) // 2
    par = np.zeros((m, 8), np.uint8)
    par[:, 0:3] = TABLE[row, 0:3]
    par[:, 3] = kind
    par[:, 4] = rng.random(m) >= closed
    return np.ascontiguousarray(lines[:2 * m]), par


def shuffled(rng, parts):
    """lanes of several (lines, par) parts, in a random order: every wave mixes kinds, limits and gates"""
    lines = np.concatenate([p[0] for p in parts]).reshape(-1, 2, 8)
    par = np.concatenate([p[1] for p in parts])
    order = rng.permutation(len(par))
    return np.ascontiguousarray(lines[order].reshape(-1, 8)), np.ascontiguousarray(par[order])


def check_lines(L, lines, par, what):
    got = np.zeros_like(lines)
    assert L.vp8hip_lane_loop_filter_lines(vp(lines.ctypes.data), vp(got.ctypes.data), vp(par.ctypes.data), len(lines)) == 0
    lp = np.repeat(par, 2, axis=0)                  # per line
    T = TABLE[table_row(lp[:, 0].astype(np.int64), lp[:, 1].astype(np.int64), lp[:, 2].astype(np.int64))]
    want = R.filter_kind(lines, lp[:, 3], T[:, 3], T[:, 4], T[:, 5], T[:, 6], lp[:, 4])
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        msg = [f"{what}: {bad.size} of {len(lines)} lines differ"]
        for i in bad[:6]:
            msg.append(f"  line {i} (lane {i // 2}, {'high' if i & 1 else 'low'} half) {lines[i].tolist()}: got {got[i].tolist()} want "
                       f"{want[i].tolist()}; sharpness {lp[i, 0]} level {lp[i, 1]} frame type {lp[i, 2]} -> mblim/blim/lim/thr "
                       f"{T[i, 3:7].tolist()}, kind {R.KINDS[lp[i, 3]]}, gate {'open' if lp[i, 4] else 'shut'}")
        raise AssertionError("\n".join(msg))
    return want


# level 63 at sharpness 0 (the largest limits: saturated filter values), level 1 at sharpness 7, every step of hev_thr in both
# frame types (levels 14 / 15, 19 / 20, 39 / 40), and sharpness > 4
CORNER_SETS = [(0, 63, 0), (0, 63, 1), (7, 1, 0), (6, 40, 1)] + [(s, l, t) for t, s in ((0, 0), (1, 3)) for l in (14, 15, 19, 20, 39, 40)]


@pytest.mark.parametrize("sharp,level,ftype", CORNER_SETS)
def test_corner_lines(L, sharp, level, ftype):
    """every (p0, q0) in 256^2 x 12 choices of (p1, q1) at the interior and hev limits, their next values and the extremes,
    through each of the four kinds"""
    rng = np.random.default_rng(1000 + 100 * sharp + 2 * level + ftype)
    row = int(table_row(sharp, level, ftype))
    lim, thr = int(TABLE[row, 5]), int(TABLE[row, 6])
    parts = [lanes(rng, R.corner_lines(rng, lim, thr), row, kind) for kind in range(4)]
    lines, par = shuffled(rng, parts)
    want = check_lines(L, lines, par, f"corner lines, sharpness {sharp} level {level} frame type {ftype}")
    assert (want != lines).any(axis=1).sum() >= 1000          # (level 1 at sharpness 7: about 11k of the 3.1M lines)


def test_every_limit_set(L):
    """4096 lines for each of the 1024 (sharpness, level, frame type), each on one boundary of the masks -- the edge limit, an
    interior difference, the hev threshold -- on one side or the other.  The lines are counted to hit every boundary from both
    sides for each kind (the hev threshold for the normal filters only)."""
    rng = np.random.default_rng(2024)
    per = 4096
    hits = {k: {} for k in range(4)}
    for chunk in np.array_split(np.arange(len(TABLE)), 4):
        row = np.repeat(chunk, per)
        kind = np.repeat(rng.integers(0, 4, size=len(row) // 2), 2)         # one kind per lane
        elim = np.where(kind % 2 == 0, TABLE[row, 3], TABLE[row, 4])
        lines = R.boundary_lines(rng, TABLE[row, 5], elim, TABLE[row, 6])
        for k in range(4):
            s = kind == k
            for name, v in R.boundary_hits(lines[s], TABLE[row[s], 5], elim[s], TABLE[row[s], 6]).items():
                hits[k][name] = hits[k].get(name, 0) + v
        par = np.zeros((len(row) // 2, 8), np.uint8)
        par[:, 0:3] = TABLE[row[::2], 0:3]
        par[:, 3] = kind[::2]
        par[:, 4] = rng.random(len(par)) >= 0.1
        lines, par = shuffled(rng, [(lines, par)])
        check_lines(L, lines, par, f"boundary lines, limit sets {chunk[0]}..{chunk[-1]}")
    for k in range(4):
        names = ("elim", "elim+1", "lim", "lim+1", "thr", "thr+1") if k < 2 else ("elim", "elim+1")
        assert all(hits[k][n] > 0 for n in names), (R.KINDS[k], hits[k])


def test_black_and_white(L):
    """the 256 lines of 0 / 255 pixels, through every kind at every limit set"""
    rng = np.random.default_rng(77)
    bw = R.black_white_lines()
    parts = [lanes(rng, bw, row, kind) for row in range(len(TABLE)) for kind in range(4)]
    lines, par = shuffled(rng, parts)
    check_lines(L, lines, par, "black and white lines")


def test_add3w_sweep(L):
    """add3w (v_pk_mad_i16 ... clamp) == clamp(f + 3 w) == add3w_stepwise for all 2^32 pairs of 16-bit values, different pairs
    in the two halves"""
    count = np.zeros(1, np.uint64)
    recs = np.zeros((16, 4), np.uint32)
    assert L.vp8hip_lane_add3w_sweep(vp(count.ctypes.data), vp(recs.ctypes.data), 16) == 0
    if count[0]:
        s16 = lambda v: (int(v) & 0xffff) - ((int(v) & 0x8000) << 1)
        msg = [f"{int(count[0])} pairs (f, w) where add3w differs from clamp(f + 3 w) or the stepwise form"]
        for klo, khi, got, step in recs[:min(16, int(count[0]))]:
            for half, k in ((0, klo), (1, khi)):
                f, w = s16(k >> 16), s16(k)
                msg.append(f"  half {half}: f {f} w {w}: add3w {s16(int(got) >> (16 * half))} stepwise {s16(int(step) >> (16 * half))} "
                           f"exact {max(-32768, min(32767, f + 3 * w))}")
        raise AssertionError("\n".join(msg))


def chroma_sources(rng, n, noise):
    """the generator of test_gpu_lane_blocks.py::test_loop_filter_macroblocks at 12 x 12"""
    base = rng.integers(0, 256, size=(n, 1, 1))
    grad = rng.integers(-3, 4, size=(n, 1, 1)) * np.arange(12).reshape(1, 12, 1) + rng.integers(-3, 4, size=(n, 1, 1)) * np.arange(12).reshape(1, 1, 12)
    step = (np.arange(12).reshape(1, 1, 12) >= rng.integers(0, 12, size=(n, 1, 1))) * rng.integers(-30, 31, size=(n, 1, 1))
    return np.clip(base + grad + step + rng.integers(-noise, noise + 1, size=(n, 12, 12)), 0, 255).astype(np.uint8)


def corner_macroblocks(rng, src, rows):
    """the left edge's eight rows and the top edge's eight columns made of corner lines at each macroblock's own limits"""
    n = len(src)
    lim, thr = np.repeat(TABLE[rows, 5], 16), np.repeat(TABLE[rows, 6], 16)
    p0 = rng.integers(0, 256, size=n * 16)
    q0 = np.clip(p0 + rng.integers(-40, 41, size=n * 16), 0, 255)
    c = R.corner_lines(rng, lim, thr, (p0, q0)).reshape(12, n * 16, 8)
    lines = c[rng.integers(0, 12, size=n * 16), np.arange(n * 16)].reshape(n, 16, 8)
    src = src.copy()
    src[:, 4:12, 0:8] = lines[:, :8]                              # rows 0..7, columns -4..3: across the left edge
    top = lines[:, 8:].transpose(0, 2, 1)                         # columns 0..7: rows -4..3 across the top edge
    src[:, 0:4, 4:12] = top[:, 0:4]
    src[:, 4:8, 8:12] = top[:, 4:8, 4:8]                          # (columns 0..3 of rows 0..3 belong to the left edge's lines)
    return src


@pytest.mark.parametrize("seed,noise", [(1, 3), (2, 12), (3, 40), (4, 255), (5, 255), (6, 6)])
def test_chroma_macroblocks(L, seed, noise):
    """lf_block_row<2> twice per macroblock, as the chroma role of the key-frame kernel runs it (top edge, then the inner
    horizontal edge, with the rows and the left neighbour's columns handed over between them), against the oracle's
    vp8_loop_filter_{mbv,bv,mbh,bh} on the u plane in vp8_loop_filter_frame's order (loopfilter.c:259-280); 30 % of the
    macroblocks take the simple filter, which leaves chroma alone.  Seed 5: black and white; seed 6: corner lines across the edges."""
    O = oracle()
    rng = np.random.default_rng(seed)
    n = 64 * 40 + 17                        # a last wave with idle lanes
    rows = rng.integers(0, len(TABLE), size=n)
    rows = np.where(TABLE[rows, 1] == 0, rows + 2, rows)          # (level 0: no filter at all)
    src = chroma_sources(rng, n, noise)
    if seed == 5:
        src = np.where(src > 127, 255, 0).astype(np.uint8)
    if seed == 6:
        src = corner_macroblocks(rng, src, rows)
    par = np.zeros((n, 8), np.uint8)
    par[:, :4] = TABLE[rows, 3:7]
    par[:, 4:7] = rng.integers(0, 2, size=(n, 3))
    par[:, 7] = rng.random(n) < 0.3
    got = np.zeros_like(src)
    assert L.vp8hip_lane_loop_filter_chroma_mbs(vp(src.ctypes.data), vp(got.ctypes.data), vp(par.ctypes.data), n) == 0
    want = src.copy()
    dummy = np.zeros((24, 24), np.uint8)
    dy = vp(dummy.ctypes.data + 4 * 24 + 4)
    for i in range(n):
        mbv, inner, mbh, simple = (int(v) for v in par[i, 4:8])
        if simple:                          # loopfilter.c:283-299: the simple filter is luma only
            continue
        u = vp(want[i].ctypes.data + 4 * 12 + 4)
        lf = OraLfi(*[int(v) for v in par[i, :4]])
        if mbv: O.vp8o_loop_filter_mbv(dy, u, None, ci(24), ci(12), ctypes.byref(lf))
        if inner: O.vp8o_loop_filter_bv(dy, u, None, ci(24), ci(12), ctypes.byref(lf))
        if mbh: O.vp8o_loop_filter_mbh(dy, u, None, ci(24), ci(12), ctypes.byref(lf))
        if inner: O.vp8o_loop_filter_bh(dy, u, None, ci(24), ci(12), ctypes.byref(lf))
    bad = np.nonzero((got != want).reshape(n, -1).any(axis=1))[0]
    if bad.size:
        i = bad[0]
        raise AssertionError(f"{bad.size} of {n} chroma macroblocks differ; first {i}: mblim/blim/lim/thr {par[i, :4].tolist()}, "
                             f"left/inner/top edge {par[i, 4:7].tolist()}, simple {par[i, 7]}; differing (row, column) from -4: "
                             f"{[(int(y) - 4, int(x) - 4) for y, x in zip(*np.nonzero(got[i] != want[i]))][:12]}")
    assert seed == 5 or (want != src).any()
