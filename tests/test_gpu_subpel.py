"""GPU (-m gpu): the sub-pixel refinement of block motion between pictures in device memory (vp8hip_frames_subpel_async;
Vp8Hip.frames_subpel; csrc/hip/vp8_subpel.hip), bit for bit against the numpy restatement (tests/subpel_reference.py, itself pinned
to the reference's vp8_find_best_sub_pixel_step by tests/test_subpel_cpu.py) applied to the coded luma vp8hip_frame_download gives: the
vectors and the four planes.  torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes
import hashlib
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, decode_stream, guarded, large_launch, two_key_frames_queued
import scale_reference as SC
import motion_reference as MR
import subpel_reference as SR

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (48, 32), (33, 17), (176, 144)]
PLANE_SETS = [15, ("val",), ("var0", "sse"), 5, ("var", "val", "var0"), 10]
SHIFT = (3, -2)                                   # (dy, dx) of frame buffer 2 against frame buffer 0
# frame buffers of upload_pictures: noise, other noise, the first shifted, flat 90, flat 97, stripes, stripes moved a column, 0, 255,
# smooth, its half-pel shift, its quarter-pel shift
PAIRS = [(0, 1), (2, 0), (3, 4), (5, 5), (6, 5), (0, 0), (1, 2), (10, 9), (11, 9), (9, 10), (7, 8)]
NFB = 12


def luma(ctx, fb):
    """the coded luma of a frame buffer as downloaded"""
    return np.ascontiguousarray(SC.planes(ctx.download_full(fb), ctx.g)[0])


class Expected:
    """the restatement over downloaded pictures, each (pair, inputs) computed once: vectors and all four planes"""

    def __init__(self, pictures):
        self.pictures, self.memo = pictures, {}

    def get(self, job, start=None, ref=None, cost=None, epb=0, precision=4, key=None):
        k = (job, key, epb if cost is not None else 0, precision)
        if k not in self.memo:
            self.memo[k] = SR.refine(self.pictures[job[0]], self.pictures[job[1]], start, ref, cost, epb, precision)
        return self.memo[k]


def stats_bits(t):
    return t.cpu().numpy().view(np.uint32)


def on_device(a, n):
    return None if a is None else torch.from_numpy(np.stack([a] * n).astype(np.int16)).to("cuda:0")


def check(ctx, exp, jobs, which, what, start=None, ref=None, cost=None, epb=0, precision=4, key=None):
    """frames_subpel over `jobs` (every job the same start and ref): the restatement's vectors and planes; -> (mv, stats) as arrays"""
    mv, st = ctx.frames_subpel(jobs, on_device(start, len(jobs)), on_device(ref, len(jobs)), cost, epb, precision, which)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    mask = SR.mask_of(which)
    assert mv.dtype == torch.int16 and tuple(mv.shape) == (len(jobs), 2, rows, cols)
    got_mv = mv.cpu().numpy()
    got_st = None
    if mask:
        assert st.dtype == torch.int32 and tuple(st.shape) == (len(jobs), bin(mask).count("1"), rows, cols)
        got_st = stats_bits(st)
    else:
        assert st is None
    for i, j in enumerate(jobs):
        want_mv, want_st = exp.get(j, start, ref, cost, epb, precision, key)
        assert np.array_equal(got_mv[i], want_mv), (what, j, got_mv[i].tolist(), want_mv.tolist())
        if mask:
            assert np.array_equal(got_st[i], SR.pick(want_st, mask)), (what, j, which, got_st[i].tolist(), SR.pick(want_st, mask).tolist())
    return got_mv, got_st


def raw_call(ctx, P, jobs, precision=4, epb=0, R=0, mask=1, cost=None, start=None, start_stride=0, ref=None, ref_stride=0, mv=None, mv_stride=0,
             stats=None, stats_stride=0, n=None):
    """vp8hip_frames_subpel_async itself, on pointers: -> its status"""
    arr = (P.HistJob * max(len(jobs), 1))(*jobs)
    vp = ctypes.c_void_p
    table = None if cost is None else np.ascontiguousarray(cost, np.int32)
    p = P.SubpelParams(precision, epb, R, mask, None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return ctx.L.vp8hip_frames_subpel_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(p), vp(start) if start else None, start_stride,
                                            vp(ref) if ref else None, ref_stride, vp(mv) if mv else None, mv_stride, vp(stats) if stats else None,
                                            stats_stride)


def upload_pictures(ctx, seed):
    """twelve frame buffers (see PAIRS), each picture's coded luma inside a frame buffer image of other bytes -- the raster borders
    hold garbage, which must not be read into any sum; -> the coded lumas as downloaded"""
    g = ctx.g
    aw, ah = g.aligned_w, g.aligned_h
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (ah, aw), dtype=np.uint8)
    yy, xx = np.mgrid[0:ah, 0:aw]
    stripes = ((xx % 4) * 60 + 20).astype(np.uint8)
    smooth = SR.lowpass(seed, aw, ah)
    pics = [a, rng.integers(0, 256, (ah, aw), dtype=np.uint8), MR.shifted(a, *SHIFT), np.full((ah, aw), 90, np.uint8), np.full((ah, aw), 97, np.uint8),
            stripes, MR.shifted(stripes, 0, 1), np.zeros((ah, aw), np.uint8), np.full((ah, aw), 255, np.uint8), smooth,
            SR.subshifted(smooth, *SR.SUBSHIFT["half"]), SR.subshifted(smooth, *SR.SUBSHIFT["quarter"])]
    assert len(pics) == NFB
    for k, p in enumerate(pics):
        buf = rng.integers(0, 256, g.frame_size, dtype=np.uint8)
        SC.planes(buf, g)[0][:] = p
        ctx.upload_frame(k, buf)
    got = [luma(ctx, k) for k in range(len(pics))]
    assert all(np.array_equal(x, y) for x, y in zip(got, pics))
    return got


@pytest.fixture(scope="module")
def raster(pkg):
    """one context per size with the twelve pictures uploaded, and its expected values, shared by the tests of this module"""
    made = {}

    def get(size):
        if size not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], NFB, 1)
            made[size] = (ctx, Expected(upload_pictures(ctx, size[0] * 139 + size[1])))
        return made[size]
    yield get
    for ctx, _ in made.values():
        ctx.close()


@pytest.mark.parametrize("precision", [4, 2])
@pytest.mark.parametrize("size", SIZES)
def test_pairs_from_raster(pkg, raster, size, precision):
    """uploaded frame buffers: the smallest picture (every macroblock a corner), one that is not square, a display size that is not
    aligned (coded 48x32) and one of 99 macroblocks; noise, shifted noise, flat, stripes, smooth against its sub-pel shifts, 0 against
    255 and a frame against itself; the plane sets in rotation; the known answers"""
    ctx, exp = raster(size)
    for which in PLANE_SETS[:3]:
        check(ctx, exp, PAIRS, which, (size, precision), precision=precision)
    mv, st = check(ctx, exp, PAIRS, 15, (size, precision, "all planes"), precision=precision)
    assert not mv[2].any() and not st[2][[0, 1, 3]].any() and (st[2][2] == 49 * 256).all()            # flat: v0, every comparison is strict
    assert not mv[3].any() and not st[3].any() and not mv[5].any() and not st[5].any()                 # a frame against itself: v0, 0
    k = PAIRS.index((10, 9))                                                                        # the half-pel shift: found exactly
    assert (mv[k][0] == SR.SUBSHIFT["half"][1]).all() and (mv[k][1] == SR.SUBSHIFT["half"][0]).all() and not st[k][:3].any()
    if precision == 4:
        k = PAIRS.index((11, 9))
        assert (mv[k][0] == SR.SUBSHIFT["quarter"][1]).all() and (mv[k][1] == SR.SUBSHIFT["quarter"][0]).all() and not st[k][:3].any()
    k = PAIRS.index((7, 8))                                                                         # |sum| = 65280: the variance in 64 bits
    assert not mv[k].any() and not st[k][[0, 1, 3]].any() and (st[k][2] == 255 * 255 * 256).all()
    only_mv, none = check(ctx, exp, PAIRS, (), (size, precision, "mv alone"), precision=precision)
    assert none is None and np.array_equal(only_mv, mv)


@pytest.mark.parametrize("size", [(48, 32), (176, 144)])
def test_the_two_call_recipe_and_other_starts(pkg, raster, size):
    """start = frames_motion's mv on the same jobs, end to end; zeros equal no tensor; the fractional bits of a start are shifted out;
    starts far beyond the UMV bounds and on them are clamped; int16's ends"""
    ctx, exp = raster(size)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    jobs = [(0, 1), (2, 0), (10, 9), (11, 9), (6, 5)]
    whole, _ = ctx.frames_motion(jobs, 4, planes=())
    mv, st = ctx.frames_subpel(jobs, start=whole, planes=15)
    got_whole, got_mv, got_st = whole.cpu().numpy(), mv.cpu().numpy(), stats_bits(st)
    for i, j in enumerate(jobs):
        want = SR.refine(exp.pictures[j[0]], exp.pictures[j[1]], got_whole[i].astype(np.int64))
        assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], want[1]), (size, j)
        assert np.array_equal(got_whole[i], MR.search(exp.pictures[j[0]], exp.pictures[j[1]], 4)[0])
    assert (got_mv[1][0] == SHIFT[1] << 3).all() and (got_mv[1][1] == SHIFT[0] << 3).all() and not got_st[1].any()    # the whole-pel shift stays
    assert (np.abs(got_mv.astype(np.int64) - got_whole) <= 6).all() and (got_st[:, 1] <= got_st[:, 3]).all()
    zeros = np.zeros((2, rows, cols), np.int64)
    mv0, st0 = check(ctx, exp, jobs[:3], 15, "zeros", start=zeros, key="zeros")
    mvn, stn = check(ctx, exp, jobs[:3], 15, "none")
    assert np.array_equal(mv0, mvn) and np.array_equal(st0, stn)
    for precision in (4, 2):
        for kind in ("near", "far", "bounds"):
            start = SR.fixture_start(kind, rows, cols, 50 + precision)
            check(ctx, exp, [(0, 1), (2, 0), (10, 9)], 15, (kind, precision), start=start, precision=precision, key=(kind, precision))
    assert (np.abs(SR.fixture_start("far", rows, cols, 54)) > 8 * 64).any() and (SR.fixture_start("near", rows, cols, 54) & 7).any()
    huge = np.full((2, rows, cols), 32767, np.int64)
    huge[1] = -32768
    check(ctx, exp, [(0, 1), (9, 10)], 15, "int16's ends", start=huge, key="huge")


def test_cost_term_and_reference_vectors(pkg, raster):
    """a table that keeps the refinement at the vector the cost is counted from; tables at both ends of error_per_bit and of the
    range; reference vectors that are odd and that put the index beyond the table (clamped); a table with error_per_bit 0 is none"""
    ctx, exp = raster((176, 144))
    rows, cols = 9, 11
    plain, _ = check(ctx, exp, [(10, 9)], ("val",), "no cost")
    assert (plain[0][0] == -4).all()
    steep = np.zeros((2, 81), np.int32)
    steep[:] = np.abs(np.arange(81) - 40) * 800
    mv, st = check(ctx, exp, [(10, 9), (0, 1)], 15, "steep", cost=steep, epb=16383, key="steep")
    assert not mv[0].any() and (st[0][0] == st[0][3]).all()
    rvec = SR.fixture_ref("given", rows, cols, 9)
    assert (rvec & 1).any()
    start = SR.fixture_start("near", rows, cols, 10)
    for R, epb in ((1, 1), (40, 300), (255, 16383), (1023, 1), (1023, 16383)):
        table = SR.fixture_cost(R, epb)
        check(ctx, exp, [(0, 1), (10, 9), (11, 9)], 15, ("cost", R, epb), start, rvec, table, epb, 4, key=("cost", R, epb))
        check(ctx, exp, [(11, 9)], ("val", "var"), ("cost", R, epb, 2), None, rvec, table, epb, 2, key=("cost2", R, epb))
    far_ref = (SR.fixture_ref("given", rows, cols, 11) * 1500).clip(-32768, 32767)
    check(ctx, exp, [(0, 1), (10, 9)], 15, "indices beyond the table", start, far_ref, SR.fixture_cost(40, 3), 70, 4, key="far ref")
    top = np.full((2, 2047), 65535, np.int32)
    check(ctx, exp, [(0, 1)], 15, "the largest entries", None, rvec, top, 16383, 4, key="top")
    a, _ = check(ctx, exp, [(10, 9)], ("val",), "epb 0", ref=rvec, cost=steep, epb=0)
    assert np.array_equal(a, plain)


def test_two_tables_queued_back_to_back(pkg, raster):
    """two calls with different tables and nothing between them: each sees its own; and the caller may change the table on return"""
    ctx, exp = raster((176, 144))
    steep = np.zeros((2, 81), np.int32)
    steep[:] = np.abs(np.arange(81) - 40) * 800
    gentle = SR.fixture_cost(40, 7)
    jobs = [(10, 9), (11, 9), (0, 1)]
    ctx.sync()
    mine = steep.copy()
    a = ctx.frames_subpel(jobs, cost=mine, error_per_bit=16383, planes=15)
    mine[:] = 65535                                                         # (the call has copied it)
    b = ctx.frames_subpel(jobs, cost=gentle, error_per_bit=300, planes=15)
    c = ctx.frames_subpel(jobs, planes=15)
    ctx.sync()
    for got, (cost, epb, key) in zip((a, b, c), ((steep, 16383, "steep"), (gentle, 300, "gentle"), (None, 0, None))):
        for i, j in enumerate(jobs):
            want = exp.get(j, None, None, cost, epb, 4, key)
            assert np.array_equal(got[0].cpu().numpy()[i], want[0]) and np.array_equal(stats_bits(got[1])[i], want[1]), (key, j)
    assert not np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())


def test_every_plane_subset_and_determinism(pkg, raster):
    """all 15 masks, and names in any order: the planes come in bit order; two runs give the same bits"""
    ctx, exp = raster((48, 32))
    for mask in range(1, 16):
        check(ctx, exp, [(0, 1), (11, 9)], mask, mask)
    for names in itertools.permutations(("var0", "val", "sse"), 3):
        check(ctx, exp, [(1, 0)], names, names)
    ctx, exp = raster((176, 144))
    mv, st = check(ctx, exp, [(0, 1), (6, 5), (0, 1)], 15, "twice")
    again = ctx.frames_subpel([(0, 1), (6, 5), (0, 1)], planes=15)
    assert np.array_equal(again[0].cpu().numpy(), mv) and np.array_equal(stats_bits(again[1]), st)
    assert np.array_equal(mv[0], mv[2]) and np.array_equal(st[0], st[2])


def test_many_jobs(pkg, raster):
    """more jobs than one launch takes (256) with a remainder, in any order with repeats, each job with a start of its own"""
    ctx, exp = raster((32, 32))
    rng = np.random.default_rng(33)
    jobs = [(int(a), int(b)) for a, b in zip(rng.integers(0, NFB, 600), rng.integers(0, NFB, 600))]
    check(ctx, exp, jobs, 15, "600 jobs")
    starts = rng.integers(-40 * 8, 40 * 8, (600, 2, 2, 2)).astype(np.int16)
    mv, st = ctx.frames_subpel(jobs, start=torch.from_numpy(starts).to("cuda:0"), planes=("val", "var0"), precision=2)
    got_mv, got_st = mv.cpu().numpy(), stats_bits(st)
    for i in (0, 1, 255, 256, 257, 511, 512, 599):
        want = SR.refine(exp.pictures[jobs[i][0]], exp.pictures[jobs[i][1]], starts[i].astype(np.int64), precision=2)
        assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], SR.pick(want[1], 9)), i


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
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        tiles = [(a, b) for a in range(n) for b in range(n) if (a + 2 * b) % 3 == 0] + [(0, n + 1), (n + 1, 1)]
        start = SR.fixture_start("near", rows, cols, 3)
        first = [ctx.frames_subpel(tiles, on_device(st, len(tiles)), planes=15, precision=pr) for st, pr in ((None, 4), (start, 2))]
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        rnd = np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                                             # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        before = ctx.memory_usage()
        mixed_jobs = [(k, n) for k in range(n)] + [(n, k) for k in range(n)] + [(n, n)]
        mixed = ctx.frames_subpel(mixed_jobs, on_device(start, len(mixed_jobs)), planes=15)
        ctx.sync()
        assert ctx.memory_usage() == before
        never = np.zeros((ctx.g.aligned_h, ctx.g.aligned_w), np.uint8)
        exp = Expected([luma(ctx, k) for k in range(n + 1)] + [never])
        assert nsrc < 2 or not np.array_equal(exp.pictures[0], exp.pictures[1])
        for (mv, st), (s0, pr) in zip(first, ((None, 4), (start, 2))):
            mv, st = mv.cpu().numpy(), stats_bits(st)
            for i, j in enumerate(tiles):
                want = exp.get(j, s0, precision=pr, key=pr)
                assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], want[1]), (name, j, pr)
                if j[0] == j[1] and s0 is None:
                    assert not mv[i].any() and not st[i].any()
        mv, st = mixed[0].cpu().numpy(), stats_bits(mixed[1])
        for i, j in enumerate(mixed_jobs):
            want = exp.get(j, start, key="mixed")
            assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], want[1]), (name, j)
        check(ctx, exp, mixed_jobs, 15, (name, "after the downloads"), start=start, key="mixed")     # ... and with every frame in raster form
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["raster", "tiles"])
def test_decoded_content(pkg, form, monkeypatch):
    """consecutive frames of an inter stream, frame k against frame k - 1, as the decoder left them, through both calls; both forms
    give the same bits"""
    P = pkg
    ctx, shown = decode_stream(P, "p_odd_130x98", form, monkeypatch)
    try:
        jobs = [(shown[k], shown[k - 1]) for k in range(1, len(shown))][:4]
        assert len(jobs) >= 3
        whole, _ = ctx.frames_motion(jobs, 8, planes=())
        mv, st = ctx.frames_subpel(jobs, start=whole, planes=15)
        ctx.sync()
        exp = Expected({k: luma(ctx, k) for k in set(shown)})
        got_whole, got_mv, got_st = whole.cpu().numpy(), mv.cpu().numpy(), stats_bits(st)
        for i, j in enumerate(jobs):
            want = SR.refine(exp.pictures[j[0]], exp.pictures[j[1]], got_whole[i].astype(np.int64))
            assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], want[1]), (form, j)
        assert (got_st[:, 1] <= got_st[:, 3]).all() and (got_mv & 7).any()      # never worse than the start; some vector is fractional
    finally:
        ctx.close()


def test_the_wrapper(pkg, raster):
    """shapes and types, out_mv / out_stats filled and returned, what the wrapper and the call refuse"""
    P = pkg
    ctx, exp = raster((48, 32))
    jobs = [(0, 1), (10, 9)]
    assert P.subpel_sizes(3, 2, 15) == (24, 96)
    L = ctx.L
    assert L.vp8hip_subpel_mv_size(ctx.h) == 24
    for mask, prec, epb, size in ((15, 4, 0, 96), (1, 2, 16383, 24), (0, 4, 0, 0), (16, 4, 0, 0), (1, 0, 0, 0), (1, 3, 0, 0), (1, 8, 0, 0), (1, 4, 16384, 0),
                                  (1, 4, -1, 0)):
        assert L.vp8hip_subpel_stats_size(ctx.h, ctypes.byref(P.SubpelParams(prec, epb, 0, mask, None))) == size, (mask, prec, epb)
    out_mv = torch.zeros((2, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    out_st = torch.zeros((2, 2, 2, 3), dtype=torch.int32, device="cuda:0")
    got = ctx.frames_subpel(jobs, planes=("var0", "val"), out_mv=out_mv, out_stats=out_st)
    assert got[0] is out_mv and got[1] is out_st
    want = exp.get(jobs[1])
    assert np.array_equal(out_mv.cpu().numpy()[1], want[0]) and np.array_equal(stats_bits(out_st)[1], SR.pick(want[1], 9))
    st_only = torch.zeros((2, 4, 2, 3), dtype=torch.int32, device="cuda:0")       # stats alone, through the call itself
    torch.cuda.synchronize()
    assert raw_call(ctx, P, jobs, mask=15, stats=st_only.data_ptr(), stats_stride=96) == 0
    ctx.sync()
    assert np.array_equal(stats_bits(st_only)[0], exp.get(jobs[0])[1]) and np.array_equal(stats_bits(st_only)[1], want[1])
    t = torch.zeros((2, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    for bad in (lambda: ctx.frames_subpel(jobs, planes=15, out_stats=out_st), lambda: ctx.frames_subpel(jobs, out_mv=out_mv.to(torch.int32)),
                lambda: ctx.frames_subpel(jobs, out_mv=out_mv[:1]), lambda: ctx.frames_subpel(jobs, start=t[:1]), lambda: ctx.frames_subpel(jobs, ref=t[:1]),
                lambda: ctx.frames_subpel(jobs, start=t.to(torch.int32)), lambda: ctx.frames_subpel(jobs, start=t.cpu()),
                lambda: ctx.frames_subpel(jobs, ref=t.cpu())):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ctx.frames_subpel([(0, NFB)]), lambda: ctx.frames_subpel([(NFB, 0)]), lambda: ctx.frames_subpel(jobs, start=out_mv, out_mv=out_mv),
                lambda: ctx.frames_subpel(jobs, ref=out_mv, out_mv=out_mv)):
        with pytest.raises(RuntimeError):
            bad()
    same = ctx.frames_subpel(jobs, start=t, ref=t, cost=SR.fixture_cost(40, 1), error_per_bit=5)      # start and ref may be the same memory
    assert np.array_equal(same[0].cpu().numpy()[1], exp.get(jobs[1], None, None, SR.fixture_cost(40, 1), 5, 4, "same")[0])


def test_guarded_destinations(pkg, raster):
    """vectors at every alignment int16 allows and stats at every alignment uint32 allows, with and without bytes between the jobs:
    the values, and the bytes around them"""
    ctx, exp = raster((48, 32))
    jobs = [(0, 1), (10, 9), (6, 5)]
    for which, pr, (off, pad), (soff, spad) in ((15, 4, (2, 0), (4, 0)), (("val",), 2, (6, 2), (8, 4)), (10, 4, (16, 10), (12, 12)),
                                                (("var0", "var"), 2, (14, 6), (4, 8))):
        mask = SR.mask_of(which)
        np_ = bin(mask).count("1")
        msize, ssize = 24, 24 * np_
        mbig, mflat = guarded(3, msize, pad, off)
        sbig, sflat = guarded(3, ssize, spad, soff)
        out_mv, out_st = mflat.view(torch.int16).unflatten(1, (2, 2, 3)), sflat.view(torch.int32).unflatten(1, (np_, 2, 3))
        assert out_mv.data_ptr() % 16 == off % 16 and out_st.data_ptr() % 16 == soff % 16
        got = ctx.frames_subpel(jobs, precision=pr, planes=which, out_mv=out_mv, out_stats=out_st)
        assert got[0] is out_mv and got[1] is out_st
        mv, st = out_mv.cpu().numpy(), stats_bits(out_st)
        for i, j in enumerate(jobs):
            want = exp.get(j, precision=pr)
            assert np.array_equal(mv[i], want[0]) and np.array_equal(st[i], SR.pick(want[1], mask)), (which, pr, j)
        assert_guards_intact(mbig, 3, msize, pad, off, what=("mv", which, off, pad))
        assert_guards_intact(sbig, 3, ssize, spad, soff, what=("stats", which, soff, spad))


def test_refusals(pkg):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    wide = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        wide.configure(4096, 16, 1, 1)                                       # 256 macroblocks across: no start tensor
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        wide.upload_frame(0, rng.integers(0, 256, wide.g.frame_size, dtype=np.uint8))
        msize, ssize = P.subpel_sizes(3, 2, 15)
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dm = big.data_ptr()
        ds, dc, dr = dm + (1 << 18), dm + (1 << 19), dm + (3 << 18)
        assert dm % 16 == 0
        ok_cost = np.zeros((2, 9), np.int32)

        def call(jobs=((0, 1),), pr=4, epb=0, R=4, mask=15, cost=None, st0=None, s0s=msize, rf=None, rs=msize, mv=dm, ms=msize, st=ds, ss=ssize, n=None,
                 c=ctx):
            return raw_call(c, P, list(jobs), pr, epb, R, mask, cost, st0, s0s, rf, rs, mv, ms, st, ss, n)
        assert call(n=0) == -2 and call(n=-1) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call([(bad, 0)]) == -2 and call([(0, bad)]) == -2 and call([(0, 1), (1, bad)]) == -2, bad
        for pr in (0, 1, 3, 8, -4, 1 << 20):
            assert call(pr=pr) == -2, pr
        for mask in (16, 64, 0x1f, 1 << 31):
            assert call(mask=mask) == -2 and call(mask=mask, st=None) == -2, mask
        assert call(mask=0) == -2                                            # stats without planes
        assert call(mv=None, st=None) == -2                                  # both outputs NULL
        for bad in (-1, 65536, 1 << 30):
            for at in ((0, 0), (1, 8), (0, 8)):
                table = ok_cost.copy()
                table[at] = bad
                assert call(cost=table, epb=1) == -2, (bad, at)
        assert call(epb=-1) == -2 and call(epb=16384) == -2 and call(cost=ok_cost, epb=16384) == -2
        assert call(cost=ok_cost, epb=1, R=0) == -2 and call(cost=ok_cost, epb=1, R=1024) == -2 and call(cost=ok_cost, epb=1, R=-1) == -2
        assert call(ms=msize - 2) == -2 and call(ss=ssize - 4) == -2 and call(st0=dc, s0s=msize - 2) == -2 and call(rf=dr, rs=msize - 2) == -2
        assert call(mv=dm + 1) == -2 and call(ms=msize + 1) == -2            # mv: multiples of 2
        assert call(st=ds + 2) == -2 and call(ss=ssize + 2) == -2            # stats: multiples of 4
        assert call(st0=dc + 1) == -2 and call(st0=dc, s0s=msize + 1) == -2  # start: multiples of 2
        assert call(rf=dr + 1) == -2 and call(rf=dr, rs=msize + 1) == -2     # ref: multiples of 2
        assert call(st=dm + 8) == -2 and call(mv=ds + ssize - 2, n=1) == -2  # mv and stats overlap
        assert call(st0=dm) == -2 and call(st0=dm + msize - 2) == -2 and call(st0=ds + 4) == -2 and call(st0=ds, mv=None) == -2     # ... or the start
        assert call(rf=dm) == -2 and call(rf=dm + msize - 2) == -2 and call(rf=ds + 4) == -2 and call(rf=ds, mv=None) == -2          # ... or the ref
        assert call([(0, 0)], st0=dc, c=wide, mv=dm, ms=4 * 256, s0s=4 * 256, st=None) == -2                   # a start tensor on 256 macroblocks across
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=p, ms=s, st=None), dm, msize, 2)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=p, ms=s), dm, msize, 2, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mv=None, st=p, ss=s), ds, ssize, 4)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, st=p, ss=s), ds, ssize, 4, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, st0=p, s0s=s), dc, msize, 2, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, rf=p, rs=s), dr, msize, 2, null=False)
        ctx.sync()
        wide.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                             # nothing was enqueued
        # the same calls into memory the test owns are accepted
        big[1 << 19:(1 << 19) + 3 * msize] = 0
        big[3 << 18:(3 << 18) + 3 * msize] = 0
        torch.cuda.synchronize()
        assert call() == 0 and call(st=None) == 0 and call(st=None, mask=0) == 0 and call(mv=None) == 0 and call(st0=dc) == 0 and call(rf=dr) == 0
        assert call(st0=dc, rf=dc) == 0 and call(pr=2) == 0 and call(cost=ok_cost, epb=16383, rf=dr) == 0
        assert call([(0, 0)], c=wide, mv=dm, ms=4 * 256, st=None) == 0 and call([(0, 0)], c=wide, rf=dr, rs=4 * 256, mv=dm, ms=4 * 256, st=None) == 0
        bad_cost = ok_cost.copy()
        bad_cost[0, 0] = -1
        assert call(cost=bad_cost, epb=0, R=0) == 0                          # (a table that is not read, nor is its range)
        ctx.sync()
        wide.sync()
    finally:
        ctx.close()
        wide.close()


def test_ordering_against_a_decode_into_the_same_frame_buffer(pkg):
    """frames_subpel, then at once a decode of another frame into one of the pair's frame buffers: the vectors are those of the
    pictures that were there at the call; and an earlier decode is seen without a sync"""
    P = pkg
    ctx, parser = two_key_frames_queued(P)
    try:
        out = ctx.frames_subpel([(0, 1), (1, 0)], planes=15)              # behind the decode of frame 0 ...
        ctx.decode([(1, 0, None)], P.STAGE_ALL)                           # ... and in front of the decode of frame 1 into the same frame buffer
        got_mv, got_st = out[0].cpu().numpy(), stats_bits(out[1])
        after = stats_bits(ctx.frames_subpel([(0, 1)], planes=("val",))[1])
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        exp = Expected([luma(ctx, 0), luma(ctx, 1)])
        assert not np.array_equal(exp.pictures[0], exp.pictures[1])
        for i, j in enumerate(((0, 1), (1, 0))):
            want = exp.get(j)
            assert np.array_equal(got_mv[i], want[0]) and np.array_equal(got_st[i], want[1]), j
        assert not after.any() and got_st[0][0].any()
    finally:
        parser.close()
        ctx.close()


def test_no_new_device_memory_and_sources_untouched(pkg):
    """without a table the call adds no device memory, with one none that the pools or torch's allocator would show (the context's
    8 KB copy); no frame buffer and no input tensor is written"""
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
        out_st = torch.empty((2, 4, rows, cols), dtype=torch.int32, device="cuda:0")
        start = torch.full((2, 2, rows, cols), 21, dtype=torch.int16, device="cuda:0")
        ref = torch.full((2, 2, rows, cols), -3, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        md5 = [hashlib.md5(ctx.download_full(k).tobytes()).hexdigest() for k in range(2)]
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        ctx.frames_subpel([(0, 1), (1, 1)], start, ref, None, 0, 4, 15, out_mv=out_mv, out_stats=out_st)
        ctx.sync()
        assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        cost = SR.fixture_cost(1023, 1)
        ctx.frames_subpel([(0, 1), (1, 1)], start, ref, cost, 7, 4, 15, out_mv=out_mv, out_stats=out_st)
        ctx.sync()
        assert ctx.memory_usage() == before and torch.cuda.memory_allocated() == reserved
        ctx.frames_subpel([(0, 1), (1, 1)], start, ref, SR.fixture_cost(40, 2), 900, 2, 15, out_mv=out_mv, out_stats=out_st)
        ctx.sync()
        assert ctx.memory_usage() == before and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            got = ctx.download_full(k)
            assert np.array_equal(got, b) and hashlib.md5(got.tobytes()).hexdigest() == md5[k]
        assert (start.cpu().numpy() == 21).all() and (ref.cpu().numpy() == -3).all()
    finally:
        ctx.close()
