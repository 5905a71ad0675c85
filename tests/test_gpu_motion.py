"""GPU (-m gpu): the block motion search between pictures in device memory (vp8hip_frames_motion_async; Vp8Hip.frames_motion;
csrc/hip/vp8_motion.hip), bit for bit against the numpy restatement (tests/motion_reference.py, itself pinned to the reference's
vp8_full_search_sad_c by tests/test_motion_cpu.py) applied to the coded luma vp8hip_frame_download gives: the vectors and the five
planes.  torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes
import hashlib
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, decode_stream, guarded, large_launch, two_key_frames_queued
import scale_reference as SC
import motion_reference as MR

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (48, 32), (33, 17), (176, 144)]
DISTANCES = [1, 4, 16, 64]
PLANE_SETS = [31, ("sad",), ("var", "sad0"), 21, ("srcvar", "sse", "sad"), 10]
SHIFT = (3, -2)                                   # (dy, dx) of frame buffer 2 against frame buffer 0
# frame buffers of upload_pictures: noise, other noise, the first shifted, flat 90, flat 97, stripes, stripes moved a column, 0, 255
PAIRS = [(0, 1), (2, 0), (3, 4), (5, 5), (6, 5), (0, 0), (1, 2)]
EXTREMES = (7, 8)                                 # |sum| = 65280: compared on every plane too -- the definition is in 64 bits


def luma(ctx, fb):
    """the coded luma of a frame buffer as downloaded"""
    return np.ascontiguousarray(SC.planes(ctx.download_full(fb), ctx.g)[0])


class Expected:
    """the restatement over downloaded pictures, each (pair, distance, centre, cost) computed once: vectors and all five planes"""

    def __init__(self, pictures):
        self.pictures, self.memo = pictures, {}

    def get(self, job, d, centre=None, cost=None, spb=0, key=None):
        k = (job, d, key, spb)
        if k not in self.memo:
            self.memo[k] = MR.search(self.pictures[job[0]], self.pictures[job[1]], d, centre, cost, spb)
        return self.memo[k]


def stats_bits(t):
    return t.cpu().numpy().view(np.uint32)


def check(ctx, exp, jobs, d, which, what, centre=None, cost=None, spb=0, key=None):
    """frames_motion over `jobs`: the restatement's vectors and planes; -> (mv, stats) as arrays"""
    cen = None if centre is None else torch.from_numpy(np.stack([centre] * len(jobs)).astype(np.int16)).to("cuda:0")
    mv, st = ctx.frames_motion(jobs, d, cen, cost, spb, which)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    mask = MR.mask_of(which)
    assert mv.dtype == torch.int16 and tuple(mv.shape) == (len(jobs), 2, rows, cols)
    got_mv = mv.cpu().numpy()
    got_st = None
    if mask:
        assert st.dtype == torch.int32 and tuple(st.shape) == (len(jobs), bin(mask).count("1"), rows, cols)
        got_st = stats_bits(st)
    else:
        assert st is None
    for i, j in enumerate(jobs):
        want_mv, want_st = exp.get(j, d, centre, cost, spb, key)
        assert np.array_equal(got_mv[i], want_mv), (what, j, d, got_mv[i].tolist(), want_mv.tolist())
        if mask:
            assert np.array_equal(got_st[i], MR.pick(want_st, mask)), (what, j, d, which)
    return got_mv, got_st


def raw_call(ctx, P, jobs, d=4, spb=0, mask=1, cost=None, centre=None, centre_stride=0, mv=None, mv_stride=0, stats=None, stats_stride=0, n=None):
    """vp8hip_frames_motion_async itself, on pointers: -> its status"""
    arr = (P.HistJob * max(len(jobs), 1))(*jobs)
    vp = ctypes.c_void_p
    table = None if cost is None else np.ascontiguousarray(cost, np.int32)
    p = P.MotionParams(d, spb, mask, None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return ctx.L.vp8hip_frames_motion_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(p), vp(centre) if centre else None, centre_stride,
                                            vp(mv) if mv else None, mv_stride, vp(stats) if stats else None, stats_stride)


def upload_pictures(ctx, seed):
    """nine frame buffers (see PAIRS), each picture's coded luma inside a frame buffer image of other bytes -- the raster borders hold
    garbage, which must not be read into any sum; -> the coded lumas as downloaded"""
    g = ctx.g
    aw, ah = g.aligned_w, g.aligned_h
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (ah, aw), dtype=np.uint8)
    yy, xx = np.mgrid[0:ah, 0:aw]
    stripes = ((xx % 4) * 60 + 20).astype(np.uint8)
    pics = [a, rng.integers(0, 256, (ah, aw), dtype=np.uint8), MR.shifted(a, *SHIFT), np.full((ah, aw), 90, np.uint8), np.full((ah, aw), 97, np.uint8),
            stripes, MR.shifted(stripes, 0, 1), np.zeros((ah, aw), np.uint8), np.full((ah, aw), 255, np.uint8)]
    for k, p in enumerate(pics):
        buf = rng.integers(0, 256, g.frame_size, dtype=np.uint8)
        SC.planes(buf, g)[0][:] = p
        ctx.upload_frame(k, buf)
    got = [luma(ctx, k) for k in range(len(pics))]
    assert all(np.array_equal(x, y) for x, y in zip(got, pics))
    return got


@pytest.fixture(scope="module")
def raster(pkg):
    """one context per size with the nine pictures uploaded, and its expected values, shared by the tests of this module"""
    made = {}

    def get(size):
        if size not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], 10, 1)
            made[size] = (ctx, Expected(upload_pictures(ctx, size[0] * 137 + size[1])))
        return made[size]
    yield get
    for ctx, _ in made.values():
        ctx.close()


@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("size", SIZES)
def test_pairs_from_raster(pkg, raster, size, d):
    """uploaded frame buffers: the smallest picture, one that is not square, a display size that is not aligned (coded 48x32) and one
    of 99 macroblocks; every distance -- at 64 the window is larger than the picture: every clamp and every bound is active --; noise,
    shifted noise, flat, stripes, 0 against 255 and a frame against itself; the plane sets in rotation; the known answers"""
    ctx, exp = raster(size)
    sets = itertools.cycle(PLANE_SETS)
    big = size == (176, 144) and d == 64            # (the restatement takes seconds there: one pair)
    jobs = [(2, 0)] if big else PAIRS + [EXTREMES]
    k = jobs.index((2, 0))
    for which in [next(sets)] if big else PLANE_SETS[:3]:
        check(ctx, exp, jobs, d, which, (size, d))
    mv, st = check(ctx, exp, jobs, d, 31, (size, d, "all planes"))
    if d > 3:                                       # the shift lies inside [-d, d): found exactly, everywhere
        assert (mv[k][0] == SHIFT[1] << 3).all() and (mv[k][1] == SHIFT[0] << 3).all() and not st[k][[0, 2, 3]].any()
    if not big:
        assert not mv[2].any() and (st[2][0] == 7 * 256).all()                       # flat: the centre
        assert not mv[3].any() and not st[3][0].any() and not mv[5].any()            # stripes and noise against themselves: the centre, 0
        assert (st[7][0] == 65280).all() and (st[7][2] == 255 * 255 * 256).all() and not st[7][3].any()
    only_mv, none = check(ctx, exp, jobs, d, (), (size, d, "mv alone"))
    assert none is None and np.array_equal(only_mv, mv)


def test_stripes_ties_and_determinism(pkg, raster):
    """period-4 stripes moved by a column: the first candidate in raster order among the ties -- the top row, the leftmost tying column
    -- and two calls give identical bits"""
    ctx, exp = raster((176, 144))
    for d in (4, 16):
        mv, st = check(ctx, exp, [(6, 5)] * 3, d, 31, "stripes")
        inner = mv[0][:, 2:-2, 2:-2] >> 3
        assert (inner[0] == -d + (1 + d) % 4).all() and (inner[1] == -d).all() and not st[0][0].any()
        again = ctx.frames_motion([(6, 5)] * 3, d, planes=31)
        assert np.array_equal(again[0].cpu().numpy(), mv) and np.array_equal(stats_bits(again[1]), st)
        assert np.array_equal(mv[0], mv[1]) and np.array_equal(st[0], st[2])


@pytest.mark.parametrize("size", [(48, 32), (176, 144)])
def test_centre_tensor(pkg, raster, size):
    """zeros equal no tensor; centres beyond the UMV bounds are clamped; centres off the dword grid; a centre equal to the true shift
    with d = 1 finds it"""
    ctx, exp = raster(size)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    zeros = np.zeros((2, rows, cols), np.int16)
    mv0, st0 = check(ctx, exp, PAIRS[:3], 4, 31, "zeros", centre=zeros, key="zeros")
    mvn, stn = check(ctx, exp, PAIRS[:3], 4, 31, "none")
    assert np.array_equal(mv0, mvn) and np.array_equal(st0, stn)
    for d in (1, 4, 16):
        far = MR.fixture_centre("far", rows, cols, 50 + d).astype(np.int16)
        near = MR.fixture_centre("near", rows, cols, 60 + d).astype(np.int16)
        assert (np.abs(far) > 64).any()
        check(ctx, exp, [(0, 1), (2, 0), (6, 5)], d, 31, ("far", d), centre=far, key=("far", d))
        check(ctx, exp, [(0, 1), (2, 0), (6, 5)], d, ("sad", "var"), ("near", d), centre=near, key=("near", d))
    huge = np.full((2, rows, cols), 32767, np.int16)
    huge[1] = -32768
    check(ctx, exp, [(0, 1)], 4, 31, "int16's ends", centre=huge, key="huge")
    true = np.zeros((2, rows, cols), np.int16)
    true[0], true[1] = SHIFT[1], SHIFT[0]
    mv, st = check(ctx, exp, [(2, 0)], 1, 31, "the true shift", centre=true, key="true")
    assert (mv[0][0] == SHIFT[1] << 3).all() and (mv[0][1] == SHIFT[0] << 3).all() and not st[0][0].any()
    assert st0[1][1].all()                                                         # ... which (0, 0) does not give


def test_cost_term(pkg, raster):
    """a table that makes a farther exact match lose to a nearer inexact one; the fixture's tables at both ends of sad_per_bit"""
    ctx, exp = raster((176, 144))
    d = 8
    plain, _ = check(ctx, exp, [(2, 0)], d, ("sad",), "no cost")
    assert (plain[0][0] == SHIFT[1] << 3).all()
    cost = np.zeros((2, 2 * d + 1), np.int32)
    cost[:] = np.abs(np.arange(2 * d + 1) - d) * 8000
    mv, st = check(ctx, exp, [(2, 0), (0, 1)], d, 31, "steep cost", cost=cost, spb=255, key="steep")
    assert not mv[0].any() and (st[0][0] == st[0][1]).all()                          # the centre, at the price of SAD0
    for spb in (1, 40, 255):
        table = MR.fixture_cost(d, spb)
        check(ctx, exp, [(0, 1), (2, 0), (6, 5)], d, 31, ("cost", spb), cost=table, spb=spb, key=("fixture", spb))
    top = np.full((2, 2 * d + 1), 65535, np.int32)
    check(ctx, exp, [(0, 1)], d, 31, "the largest entries", cost=top, spb=255, key="top")
    # a table with sad_per_bit 0 is no table
    a, _ = check(ctx, exp, [(2, 0)], d, ("sad",), "spb 0", cost=cost, spb=0)
    assert np.array_equal(a, plain)


def test_every_plane_subset(pkg, raster):
    """all 31 masks, and names in any order: the planes come in bit order"""
    ctx, exp = raster((48, 32))
    for mask in range(1, 32):
        check(ctx, exp, [(0, 1), (2, 0)], 4, mask, mask)
    for names in itertools.permutations(("srcvar", "sad0", "var"), 3):
        check(ctx, exp, [(1, 0)], 4, names, names)


def test_many_jobs_and_other_distances(pkg, raster):
    """more jobs than one launch takes (256) with a remainder, in any order with repeats; distances whose window is no multiple of
    the item (odd, 2 mod 4) and the ones the measurement uses"""
    ctx, exp = raster((32, 32))
    rng = np.random.default_rng(32)
    jobs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 9, 600), rng.integers(0, 9, 600))]
    check(ctx, exp, jobs, 4, 31, "600 jobs")
    ctx, exp = raster((48, 32))
    for d in (2, 3, 5, 7, 8, 9, 30, 32, 33, 63):
        check(ctx, exp, [(0, 1), (2, 0), (6, 5)], d, 31, ("distance", d))


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_pairs_from_tiles(pkg, name, monkeypatch):
    """frames a large launch left as tiles: tiles against tiles, tiles against an uploaded raster frame in both orders, a frame against
    itself, a frame buffer never written; no raster pool is made for them and the context's memory does not change.  Expected values
    from pictures downloaded AFTER the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 4
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        before = ctx.memory_usage()
        few = name != "kf_odd_67x45"                                         # (99 macroblocks: the restatement's time)
        tiles = [(a, b) for a in range(n) for b in range(n) if (a + 2 * b) % 3 == 0][::3 if few else 1] + [(0, n + 1), (n + 1, 1)]
        first = [ctx.frames_motion(tiles, d, planes=31) for d in (4, 16)]
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        rnd = np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                                             # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        before = ctx.memory_usage()
        mixed_jobs = [(0, n), (n, 1), (n, n)] if few else [(k, n) for k in range(n)] + [(n, k) for k in range(n)] + [(n, n)]
        mixed = ctx.frames_motion(mixed_jobs, 16, planes=31)
        ctx.sync()
        assert ctx.memory_usage() == before
        never = np.zeros((ctx.g.aligned_h, ctx.g.aligned_w), np.uint8)
        exp = Expected([luma(ctx, k) for k in range(n + 1)] + [never])
        assert nsrc < 2 or not np.array_equal(exp.pictures[0], exp.pictures[1])
        for (mv, st), d in zip(first, (4, 16)):
            mv, st = mv.cpu().numpy(), stats_bits(st)
            for i, j in enumerate(tiles):
                want = exp.get(j, d)
                assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], want[1]), (name, j, d)
                if j[0] == j[1]:
                    assert not mv[i].any() and not st[i][:4].any()
        mv, st = mixed[0].cpu().numpy(), stats_bits(mixed[1])
        for i, j in enumerate(mixed_jobs):
            want = exp.get(j, 16)
            assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], want[1]), (name, j)
        check(ctx, exp, mixed_jobs, 16, 31, (name, "after the downloads"))     # ... and with every frame in raster form
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["raster", "tiles"])
def test_decoded_content(pkg, form, monkeypatch):
    """consecutive frames of an inter stream, frame k against frame k - 1, as the decoder left them; both forms give the same bits"""
    P = pkg
    ctx, shown = decode_stream(P, "p_odd_130x98", form, monkeypatch)
    try:
        jobs = [(shown[k], shown[k - 1]) for k in range(1, len(shown))][:4]
        assert len(jobs) >= 3
        mv, st = ctx.frames_motion(jobs, 16, planes=31)
        ctx.sync()
        exp = Expected({k: luma(ctx, k) for k in set(shown)})
        got_mv, got_st = mv.cpu().numpy(), stats_bits(st)
        for i, j in enumerate(jobs):
            want = exp.get(j, 16)
            assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], want[1]), (form, j)
        assert (got_st[:, 0] <= got_st[:, 1]).all()                            # the best is never worse than (0, 0), the centre
    finally:
        ctx.close()


def test_the_wrapper(pkg, raster):
    """shapes and types, out_mv / out_stats filled and returned, what the wrapper and the call refuse"""
    P = pkg
    ctx, exp = raster((48, 32))
    jobs = [(0, 1), (2, 0)]
    assert P.motion_sizes(3, 2, 31) == (24, 120)
    L = ctx.L
    assert L.vp8hip_motion_mv_size(ctx.h) == 24
    for mask, d, spb, size in ((31, 16, 0, 120), (1, 64, 255, 24), (0, 16, 0, 0), (32, 16, 0, 0), (1, 0, 0, 0), (1, 65, 0, 0), (1, 16, 256, 0), (1, 16, -1, 0)):
        assert L.vp8hip_motion_stats_size(ctx.h, ctypes.byref(P.MotionParams(d, spb, mask, None))) == size, (mask, d, spb)
    out_mv = torch.zeros((2, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    out_st = torch.zeros((2, 2, 2, 3), dtype=torch.int32, device="cuda:0")
    got = ctx.frames_motion(jobs, 4, planes=("var", "sad"), out_mv=out_mv, out_stats=out_st)
    assert got[0] is out_mv and got[1] is out_st
    want = exp.get(jobs[1], 4)
    assert np.array_equal(out_mv.cpu().numpy()[1], want[0]) and np.array_equal(stats_bits(out_st)[1], MR.pick(want[1], 9))
    st_only = torch.zeros((2, 5, 2, 3), dtype=torch.int32, device="cuda:0")       # stats alone, through the call itself
    torch.cuda.synchronize()
    assert raw_call(ctx, P, jobs, 4, 0, 31, stats=st_only.data_ptr(), stats_stride=120) == 0
    ctx.sync()
    assert np.array_equal(stats_bits(st_only)[0], exp.get(jobs[0], 4)[1]) and np.array_equal(stats_bits(st_only)[1], want[1])
    cen = torch.zeros((2, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    for bad in (lambda: ctx.frames_motion(jobs, 4, planes=31, out_stats=out_st), lambda: ctx.frames_motion(jobs, 4, out_mv=out_mv.to(torch.int32)),
                lambda: ctx.frames_motion(jobs, 4, out_mv=out_mv[:1]), lambda: ctx.frames_motion(jobs, 4, centre=cen[:1]),
                lambda: ctx.frames_motion(jobs, 4, centre=cen.to(torch.int32)), lambda: ctx.frames_motion(jobs, 4, centre=cen.cpu())):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ctx.frames_motion([(0, 10)]), lambda: ctx.frames_motion([(10, 0)]), lambda: ctx.frames_motion(jobs, 4, centre=out_mv, out_mv=out_mv)):
        with pytest.raises(RuntimeError):
            bad()


def test_guarded_destinations(pkg, raster):
    """vectors at every alignment int16 allows and stats at every alignment uint32 allows, with and without bytes between the jobs:
    the values, and the bytes around them"""
    ctx, exp = raster((48, 32))
    jobs = [(0, 1), (2, 0), (6, 5)]
    for which, d, (off, pad), (soff, spad) in ((31, 4, (2, 0), (4, 0)), (("sad",), 16, (6, 2), (8, 4)), (10, 1, (16, 10), (12, 12)), (("srcvar", "sad0"), 64, (14, 6), (4, 8))):
        mask = MR.mask_of(which)
        np_ = bin(mask).count("1")
        msize, ssize = 24, 24 * np_
        mbig, mflat = guarded(3, msize, pad, off)
        sbig, sflat = guarded(3, ssize, spad, soff)
        out_mv, out_st = mflat.view(torch.int16).unflatten(1, (2, 2, 3)), sflat.view(torch.int32).unflatten(1, (np_, 2, 3))
        assert out_mv.data_ptr() % 16 == off % 16 and out_st.data_ptr() % 16 == soff % 16
        got = ctx.frames_motion(jobs, d, planes=which, out_mv=out_mv, out_stats=out_st)
        assert got[0] is out_mv and got[1] is out_st
        mv, st = out_mv.cpu().numpy(), stats_bits(out_st)
        for i, j in enumerate(jobs):
            want = exp.get(j, d)
            assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], MR.pick(want[1], mask)), (which, d, j)
        assert_guards_intact(mbig, 3, msize, pad, off, what=("mv", which, off, pad))
        assert_guards_intact(sbig, 3, ssize, spad, soff, what=("stats", which, soff, spad))


def test_refusals(pkg):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    wide = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        wide.configure(4096, 16, 1, 1)                                       # 256 macroblocks across: no centre tensor
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        wide.upload_frame(0, rng.integers(0, 256, wide.g.frame_size, dtype=np.uint8))
        msize, ssize = P.motion_sizes(3, 2, 31)
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dm = big.data_ptr()
        ds, dc = dm + (1 << 18), dm + (1 << 19)
        assert dm % 16 == 0
        ok_cost = np.zeros((2, 9), np.int32)

        def call(jobs=((0, 1),), d=4, spb=0, mask=31, cost=None, cen=None, cs=msize, mv=dm, ms=msize, st=ds, ss=ssize, n=None, c=ctx):
            return raw_call(c, P, list(jobs), d, spb, mask, cost, cen, cs, mv, ms, st, ss, n)
        assert call(n=0) == -2 and call(n=-1) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call([(bad, 0)]) == -2 and call([(0, bad)]) == -2 and call([(0, 1), (1, bad)]) == -2, bad
        for d in (0, -1, 65, 1 << 20):
            assert call(d=d) == -2, d
        for mask in (32, 64, 0x3f, 1 << 31):
            assert call(mask=mask) == -2 and call(mask=mask, st=None) == -2, mask
        assert call(mask=0) == -2                                            # stats without planes
        assert call(mv=None, st=None) == -2                                  # both outputs NULL
        for bad in (-1, 65536, 1 << 30):
            for at in ((0, 0), (1, 8), (0, 8)):
                table = ok_cost.copy()
                table[at] = bad
                assert call(cost=table, spb=1) == -2, (bad, at)
        assert call(spb=-1) == -2 and call(spb=256) == -2 and call(cost=ok_cost, spb=256) == -2
        assert call(ms=msize - 2) == -2 and call(ss=ssize - 4) == -2 and call(cen=dc, cs=msize - 2) == -2      # strides below the sizes
        assert call(mv=dm + 1) == -2 and call(ms=msize + 1) == -2            # mv: multiples of 2
        assert call(st=ds + 2) == -2 and call(ss=ssize + 2) == -2            # stats: multiples of 4
        assert call(cen=dc + 1) == -2 and call(cen=dc, cs=msize + 1) == -2   # centre: multiples of 2
        assert call(st=dm + 8) == -2 and call(mv=ds + ssize - 2, n=1) == -2  # mv and stats overlap
        assert call(cen=dm) == -2 and call(cen=dm + msize - 2) == -2 and call(cen=ds + 4) == -2 and call(cen=ds, mv=None) == -2     # ... or the centre
        assert call([(0, 0)], cen=dc, c=wide, mv=dm, ms=4 * 256, cs=4 * 256, st=None) == -2                     # a centre tensor on 256 macroblocks across
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=p, ms=s, st=None), dm, msize, 2)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=p, ms=s), dm, msize, 2, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=None, st=p, ss=s), ds, ssize, 4)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, st=p, ss=s), ds, ssize, 4, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, cen=p, cs=s), dc, msize, 2, null=False)
        ctx.sync()
        wide.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                             # nothing was enqueued
        # the same calls into memory the test owns are accepted
        big[1 << 19:(1 << 19) + 3 * msize] = 0
        torch.cuda.synchronize()
        assert call() == 0 and call(st=None) == 0 and call(st=None, mask=0) == 0 and call(mv=None) == 0 and call(cen=dc) == 0
        assert call(cost=ok_cost, spb=255) == 0 and call(d=64) == 0 and call(d=1) == 0 and call([(0, 0)], c=wide, mv=dm, ms=4 * 256, st=None) == 0
        bad_cost = ok_cost.copy()
        bad_cost[0, 0] = -1
        assert call(cost=bad_cost, spb=0) == 0                               # (a table that is not read)
        ctx.sync()
        wide.sync()
    finally:
        ctx.close()
        wide.close()


def test_ordering_against_a_decode_into_the_same_frame_buffer(pkg):
    """frames_motion, then at once a decode of another frame into one of the pair's frame buffers: the vectors are those of the
    pictures that were there at the call; and an earlier decode is seen without a sync"""
    P = pkg
    ctx, parser = two_key_frames_queued(P)
    try:
        out = ctx.frames_motion([(0, 1), (1, 0)], 4, planes=31)          # behind the decode of frame 0 ...
        ctx.decode([(1, 0, None)], P.STAGE_ALL)                           # ... and in front of the decode of frame 1 into the same frame buffer
        got_mv, got_st = out[0].cpu().numpy(), stats_bits(out[1])
        after = stats_bits(ctx.frames_motion([(0, 1)], 4, planes=("sad",))[1])
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        exp = Expected([luma(ctx, 0), luma(ctx, 1)])
        assert not np.array_equal(exp.pictures[0], exp.pictures[1])
        for i, j in enumerate(((0, 1), (1, 0))):
            want = exp.get(j, 4)
            assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], want[1]), j
        assert not after.any() and got_st[0][0].any()
    finally:
        parser.close()
        ctx.close()


def test_no_new_device_memory_and_sources_untouched(pkg):
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        w, h = 130, 98
        ctx.configure(w, h, 2, 1)
        rng = np.random.default_rng(98)
        bufs = [rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8) for _ in range(2)]
        for k, b in enumerate(bufs):
            ctx.upload_frame(k, b)
        ctx.sync()
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        out_mv = torch.empty((2, 2, rows, cols), dtype=torch.int16, device="cuda:0")
        out_st = torch.empty((2, 5, rows, cols), dtype=torch.int32, device="cuda:0")
        cen = torch.zeros((2, 2, rows, cols), dtype=torch.int16, device="cuda:0")
        cost = MR.fixture_cost(16, 1)
        torch.cuda.synchronize()
        md5 = [hashlib.md5(ctx.download_full(k).tobytes()).hexdigest() for k in range(2)]
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        ctx.frames_motion([(0, 1), (1, 1)], 16, cen, cost, 7, 31, out_mv=out_mv, out_stats=out_st)
        ctx.sync()
        assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            got = ctx.download_full(k)
            assert np.array_equal(got, b) and hashlib.md5(got.tobytes()).hexdigest() == md5[k]
        assert not cen.cpu().numpy().any()
    finally:
        ctx.close()
