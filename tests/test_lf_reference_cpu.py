"""CPU: tests/lf_reference.py -- the numpy restatement of loopfilter_filters.c the loop-filter edge tests
(tests/test_gpu_lf_edges.py) measure the packed kernels against -- equals the oracle's per-edge functions
(vp8o_loop_filter_{mbh,bh,simple_mbh,simple_bh}, pinned to the reference by tests/test_oracle_vs_ref.py) line for line,
on lines from the same corner generator, and its limits table equals vp8o_lf_limits for every (sharpness, level, frame type)."""
import ctypes

import numpy as np
import pytest

import lf_reference as R
from vp8_testlib import oracle

vp, ci = ctypes.c_void_p, ctypes.c_int


class OraLfi(ctypes.Structure):
    _fields_ = [("mblim", ctypes.c_ubyte), ("blim", ctypes.c_ubyte), ("lim", ctypes.c_ubyte), ("hev_thr", ctypes.c_ubyte)]


def test_limits_table():
    O = oracle()
    T = R.limits_table()
    assert T.shape == (8 * 64 * 2, 7)
    lfi = OraLfi()
    for s, l, t, mblim, blim, lim, thr in T:
        O.vp8o_lf_limits(ci(int(s)), ci(int(l)), ci(int(t)), ctypes.byref(lfi))
        assert (lfi.mblim, lfi.blim, lfi.lim, lfi.hev_thr) == (mblim, blim, lim, thr), (s, l, t)
    # the hev threshold's steps (lf_init_lut) and the extremes of the limits
    assert {int(v) for v in T[:, 6]} == {0, 1, 2, 3}
    assert T[:, 3].max() == 193 and T[:, 4].max() == 189 and T[:, 5].max() == 63 and T[:, 5].min() == 1


def corner_blocks(seed, blocks):
    """12 * blocks blocks of 16 corner lines, each block with one random limit set of the table"""
    rng = np.random.default_rng(seed)
    T = R.limits_table()
    pick = rng.integers(0, len(T), size=blocks)
    lim, thr = np.repeat(T[pick, 5], 16), np.repeat(T[pick, 6], 16)
    p0q0 = rng.integers(0, 256, size=(2, blocks * 16))
    near = rng.random(blocks * 16) < 0.75               # most pairs close enough for the edge limits to let them through
    p0q0[1, near] = np.clip(p0q0[0, near] + rng.integers(-40, 41, size=near.sum()), 0, 255)
    lines = R.corner_lines(rng, lim, thr, p0q0).reshape(12 * blocks, 16, 8)
    return lines, T[np.tile(pick, 12)]


@pytest.mark.parametrize("fn", ["mbh", "bh", "simple_mbh", "simple_bh"])
def test_filters_match_oracle(fn):
    """16 lines as the columns of a horizontal block edge.  bh filters three edges (rows 4, 8, 12 of the block): the lines sit on
    the middle one, and q0 = p0 ^ 0x80 across the other two keeps their masks shut (2 * 128 > any edge limit)."""
    O = oracle()
    lines, lims = corner_blocks({"mbh": 1, "bh": 2, "simple_mbh": 3, "simple_bh": 4}[fn], 1100)
    nb = len(lines)
    assert nb * 16 >= 200_000
    inner = fn in ("bh", "simple_bh")
    rows, top, yrow = (16, 4, 0) if inner else (8, 0, 4)       # rows of the block, the row of p3, the row y points at
    rng = np.random.default_rng(99)
    buf = rng.integers(0, 256, size=(nb, rows, 16)).astype(np.uint8)
    buf[:, top:top + 8, :] = lines.transpose(0, 2, 1)
    if inner:
        buf[:, 3, :] = buf[:, 4, :] ^ 0x80
        buf[:, 12, :] = buf[:, 11, :] ^ 0x80
    got = buf.copy()
    f = getattr(O, "vp8o_loop_filter_" + fn)
    for b in range(nb):
        mblim, blim, lim, thr = (int(v) for v in lims[b, 3:7])
        y = vp(got[b].ctypes.data + yrow * 16)
        if fn.startswith("simple"):
            f(y, ci(16), ctypes.c_ubyte(blim if inner else mblim))
        else:
            f(y, None, None, ci(16), ci(0), ctypes.byref(OraLfi(mblim, blim, lim, thr)))
    flat = lines.reshape(-1, 8)
    L = lambda k: np.repeat(lims[:, k], 16)
    kind = {"mbh": 0, "bh": 1, "simple_mbh": 2, "simple_bh": 3}[fn]
    want = R.filter_kind(flat, kind, L(3), L(4), L(5), L(6))
    have = got[:, top:top + 8, :].transpose(0, 2, 1).reshape(-1, 8)
    bad = np.nonzero((have != want).any(axis=1))[0]
    assert bad.size == 0, [(flat[i].tolist(), have[i].tolist(), want[i].tolist(), lims[i // 16].tolist()) for i in bad[:4]]
    outside = np.concatenate([got[:, :top], got[:, top + 8:]], axis=1), np.concatenate([buf[:, :top], buf[:, top + 8:]], axis=1)
    assert np.array_equal(*outside)                 # the shut edges changed nothing
    changed = (want != flat).any(axis=1).mean()
    assert changed > 0.1, changed                   # a fair share of the lines are ones the filters act on
