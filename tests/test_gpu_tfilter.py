"""GPU (-m gpu): the motion-compensated temporal filter of pictures in device memory (vp8hip_frames_tfilter_async; Vp8Hip.frames_tfilter;
csrc/hip/vp8_tfilter.hip), bit for bit against the numpy restatement (tests/tfilter_reference.py, itself pinned to the reference's
vp8_temporal_filter_apply_c over the reference's predictions by tests/test_tfilter_cpu.py) applied to the coded planes
vp8hip_frame_download gives: the picture and the per-pixel count.  torch is imported here, before the package loads libvpx's
library: one HIP runtime per process."""
import ctypes
import hashlib

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, decode_stream, guarded, large_launch, picture_into, two_key_frames_queued
import scale_reference as SC
import tfilter_reference as TR

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (48, 32), (37, 21), (176, 144)]
# frame buffers of upload_pictures: 0 .. 14 a sequence (0 the centre, smooth; the others noisy and moved), 15 .. 18 flat 90, flat 97,
# noise, flat 200
NFB = 19
# the pair list of most tests: the centre over its fifteen, then pairs of the others; the last is used by no job
PAIRS = [(0, k) for k in range(15)] + [(17, 0), (17, 17), (15, 16), (15, 15), (15, 18), (0, 5)]
JOBS = [(0, 0, 15), (0, 0, 1), (0, 1, 2), (17, 15, 2), (0, 1, 2), (15, 17, 3), (0, 2, 1)]


def coded(ctx, fb):
    """the three coded planes of a frame buffer as downloaded"""
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


class Expected:
    """the restatement over downloaded pictures, each (job, inputs) computed once: (picture, count) at the display size"""

    def __init__(self, pictures, display):
        self.pictures, self.display, self.memo = pictures, display, {}

    def get(self, job, pairs, mvs=None, errs=None, strength=3, filt="sixtap", key=None, thresh=TR.THRESH):
        fb, first, count = job
        refs = tuple(pairs[k][1] for k in range(first, first + count))
        k = (fb, refs, first if (mvs is not None or errs is not None) else None, key, strength, filt, thresh)
        if k not in self.memo:
            self.memo[k] = TR.tfilter(self.pictures[fb], [self.pictures[r] for r in refs], None if mvs is None else mvs[first:first + count],
                                      None if errs is None else errs[first:first + count], strength, filt, thresh, self.display)
        return self.memo[k]


def count_bits(t):
    return t.cpu().numpy().view(np.uint16)


def mv_on_device(mvs):
    return None if mvs is None else torch.from_numpy(np.stack(mvs).astype(np.int16)).to("cuda:0")


def err_on_device(errs):
    return None if errs is None else torch.from_numpy(np.stack(errs).astype(np.uint32).view(np.int32)).to("cuda:0")


def check(ctx, exp, jobs, pairs, what, mvs=None, errs=None, strength=3, filt="sixtap", key=None, thresh=TR.THRESH):
    """frames_tfilter over `jobs`: the restatement's picture and count; -> (pictures, counts) as arrays"""
    pic, cnt = ctx.frames_tfilter(jobs, pairs, mv_on_device(mvs), err_on_device(errs), strength, filt, thresh, want_count=True)
    size = TR.pack(exp.pictures[jobs[0][0]], *exp.display).size
    assert pic.dtype == torch.uint8 and cnt.dtype == torch.int16 and tuple(pic.shape) == (len(jobs), size) == tuple(cnt.shape)
    got_pic, got_cnt = pic.cpu().numpy(), count_bits(cnt)
    for i, j in enumerate(jobs):
        want = exp.get(j, pairs, mvs, errs, strength, filt, key, thresh)
        bad = np.flatnonzero(got_cnt[i] != want[1])
        assert not bad.size, (what, j, "count", bad[:8].tolist(), got_cnt[i][bad[:8]].tolist(), want[1][bad[:8]].tolist())
        bad = np.flatnonzero(got_pic[i] != want[0])
        assert not bad.size, (what, j, "picture", bad[:8].tolist(), got_pic[i][bad[:8]].tolist(), want[0][bad[:8]].tolist())
    return got_pic, got_cnt


def fixture_inputs(kind, weights, ctx, npairs, seed):
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    mvs = None if kind == "zero" else [TR.fixture_mv(kind, rows, cols, seed, k) for k in range(npairs)]
    errs = None if weights == "two" else [TR.fixture_err(weights, rows, cols, seed, k) for k in range(npairs)]
    return mvs, errs


def raw_call(ctx, P, jobs, pairs, strength=3, filt=0, lo=10000, hi=20000, mv=None, mv_stride=0, err=None, err_stride=0, dst=None, dst_stride=0, cnt=None,
             cnt_stride=0, n=None, npairs=None):
    """vp8hip_frames_tfilter_async itself, on pointers: -> its status"""
    jarr = (P.TfilterJob * max(len(jobs), 1))(*jobs)
    parr = (P.HistJob * max(len(pairs), 1))(*pairs)
    vp = ctypes.c_void_p
    p = P.TfilterParams(strength, filt, lo, hi)
    return ctx.L.vp8hip_frames_tfilter_async(ctx.h, jarr, len(jobs) if n is None else n, parr, len(pairs) if npairs is None else npairs, ctypes.byref(p),
                                             vp(mv) if mv else None, mv_stride, vp(err) if err else None, err_stride, vp(dst) if dst else None,
                                             dst_stride, vp(cnt) if cnt else None, cnt_stride)


def upload_pictures(ctx, seed):
    """the nineteen frame buffers, each picture's three coded planes inside a frame buffer image of other bytes -- the raster borders
    hold garbage, which must not reach any output; -> the coded planes as downloaded"""
    g = ctx.g
    aw, ah = g.aligned_w, g.aligned_h
    rng = np.random.default_rng(seed)
    centre, sources = TR.sequence(aw, ah, seed, 15)
    pics = sources + [TR.picture("flat90", aw, ah, 0), TR.picture("flat97", aw, ah, 0), TR.picture("noise", aw, ah, seed + 9), TR.picture("flat200", aw, ah, 0)]
    assert len(pics) == NFB and pics[0] is centre
    for k, p in enumerate(pics):
        ctx.upload_frame(k, picture_into(rng.integers(0, 256, g.frame_size, dtype=np.uint8), g, p))
    got = [coded(ctx, k) for k in range(NFB)]
    assert all(np.array_equal(a, b) for x, y in zip(got, pics) for a, b in zip(x, y))
    return got


@pytest.fixture(scope="module")
def raster(pkg):
    """one context per size with the nineteen pictures uploaded, and its expected values, shared by the tests of this module"""
    made = {}

    def get(size):
        if size not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], NFB, 1)
            made[size] = (ctx, Expected(upload_pictures(ctx, size[0] * 139 + size[1]), size))
        return made[size]
    yield get
    for ctx, _ in made.values():
        ctx.close()


@pytest.mark.parametrize("filt", TR.FILTERS)
@pytest.mark.parametrize("size", SIZES)
def test_jobs_from_raster(pkg, raster, size, filt):
    """uploaded frame buffers with garbage in their borders: the smallest picture (every macroblock on two picture edges), one that
    is not square, a display size below the coded one with odd chroma, and one of 99 macroblocks; counts 1, 2, 3 and 15, jobs that
    share pairs, a repeated job, a pair list longer than any job uses; no vectors and no errors, then vectors of every phase with
    errors on both sides of both thresholds at strengths 0 and 6, then all weights 0; the known answers"""
    ctx, exp = raster(size)
    w, h = size
    pic, cnt = check(ctx, exp, JOBS, PAIRS, (size, filt, "plain"), filt=filt)
    assert np.array_equal(pic[1], TR.pack(exp.pictures[0], w, h)) and (cnt[1] == 32).all()             # a picture over itself
    assert np.array_equal(pic[2], pic[4]) and np.array_equal(cnt[2], cnt[4])                           # the repeated job
    assert (cnt[3][:w * h].reshape(h, w) >= 32).all()                                                  # noise over (smooth, itself): itself at least
    mvs, errs = fixture_inputs("phases", "mixed", ctx, len(PAIRS), 5)
    for strength in (0, 6):
        pic, cnt = check(ctx, exp, JOBS, PAIRS, (size, filt, strength), mvs, errs, strength, filt, key="phases")
        assert int(cnt.max()) <= 480
    # flat 90 over (flat 97, itself, flat 200) at strength 6: 28 + 32 + 0, (28 * 97 + 32 * 90) / 60 -> 93, wherever the vectors point
    pic, cnt = check(ctx, exp, JOBS[5:6], PAIRS, (size, filt, "flat"), mvs, None, 6, filt, key="flat")
    assert (pic[0] == 93).all() and (cnt[0] == 60).all()
    _, none = fixture_inputs("zero", "none", ctx, len(PAIRS), 6)
    pic, cnt = check(ctx, exp, JOBS[:3], PAIRS, (size, filt, "no weight"), mvs, none, 3, filt, key="none")
    assert not pic.any() and not cnt.any()


@pytest.mark.parametrize("size", [(48, 32), (176, 144)])
def test_vectors(pkg, raster, size):
    """vectors alone (no errors) and errors alone (no vectors); negative odd vectors; vectors that carry the block wholly outside the
    picture; int16's ends; whole-pixel vectors (the copy path, also where only chroma is fractional)"""
    ctx, exp = raster(size)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    jobs = [(0, 0, 3), (0, 4, 2), (17, 15, 1)] if size == (48, 32) else [(0, 1, 2), (17, 15, 1)]
    for filt in TR.FILTERS:
        for kind in ("phases", "negodd", "outside"):
            mvs, _ = fixture_inputs(kind, "two", ctx, len(PAIRS), 21)
            check(ctx, exp, jobs, PAIRS, (size, filt, kind), mvs, None, 3, filt, key=kind)
        _, errs = fixture_inputs("zero", "mixed", ctx, len(PAIRS), 22)
        check(ctx, exp, jobs, PAIRS, (size, filt, "errors alone"), None, errs, 3, filt, key="errs")
        ends = []
        for k in range(len(PAIRS)):
            v = np.zeros((2, rows, cols), np.int64)
            v[0], v[1] = (32767, -32768, 32767, -32767)[k % 4], (-32768, 32767, 32766, 5)[k % 4]
            ends.append(v)
        check(ctx, exp, jobs, PAIRS, (size, filt, "int16's ends"), ends, None, 6, filt, key="ends")
        whole = [(TR.fixture_mv("phases", rows, cols, 23, k) >> 3 << 3) + np.array([8, 0]).reshape(2, 1, 1) * (k % 2) for k in range(len(PAIRS))]
        assert any((v & 15).any() for v in whole) and not any((v & 7).any() for v in whole)     # luma whole, chroma at half pixels somewhere
        check(ctx, exp, jobs, PAIRS, (size, filt, "whole pixels"), whole, None, 3, filt, key="whole")


def test_the_three_call_composition(pkg, raster):
    """frames_motion -> frames_subpel(planes=("val",)) -> frames_tfilter with the tensors passed on untouched"""
    ctx, exp = raster((176, 144))
    pairs = [(0, k) for k in range(7)] + [(17, 3), (17, 17)]
    jobs = [(0, 0, 7), (17, 7, 2), (0, 2, 3)]
    whole, _ = ctx.frames_motion(pairs, 4, planes=())
    mv, val = ctx.frames_subpel(pairs, start=whole, planes=("val",))
    assert tuple(val.shape) == (len(pairs), 1, 9, 11)
    got = ctx.frames_tfilter(jobs, pairs, mv, val, 3, want_count=True)
    again = ctx.frames_tfilter(jobs, pairs, mv, val[:, 0], 3, want_count=True)           # [npairs, rows, cols] is the same plane
    mvs, errs = list(mv.cpu().numpy().astype(np.int64)), list(val.cpu().numpy().view(np.uint32)[:, 0])
    weights = {TR.weight(e) for plane in errs for e in plane.ravel()}
    assert len(weights) >= 2 and any((v & 7).any() for v in mvs)                        # some source is trusted less, some vector is fractional
    for i, j in enumerate(jobs):
        want = exp.get(j, pairs, mvs, errs, 3, "sixtap", key="composition")
        assert np.array_equal(got[0].cpu().numpy()[i], want[0]) and np.array_equal(count_bits(got[1])[i], want[1]), j
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def test_determinism_and_many_jobs(pkg, raster):
    """the same call twice gives the same bytes; more jobs than one launch takes, by either of its limits (96 jobs, 480 sources), in
    any order with repeats"""
    ctx, exp = raster((32, 32))
    mvs, errs = fixture_inputs("phases", "mixed", ctx, len(PAIRS), 31)
    a = check(ctx, exp, JOBS, PAIRS, "once", mvs, errs, 3, key="det")
    b = check(ctx, exp, JOBS, PAIRS, "twice", mvs, errs, 3, key="det")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    kinds = [(0, 0, 15), (0, 3, 12), (0, 14, 1), (17, 15, 2), (15, 17, 3), (0, 7, 5), (0, 1, 14), (17, 16, 1)]
    rng = np.random.default_rng(32)
    many = [kinds[int(k)] for k in rng.integers(0, len(kinds), 300)]                     # ~ 2400 sources: the source limit cuts first
    check(ctx, exp, many, PAIRS, "300 jobs", mvs, errs, 3, key="det")
    ones = [kinds[2], kinds[7]] * 120                                                   # 240 jobs of one source: the job limit cuts
    check(ctx, exp, ones, PAIRS, "240 small jobs", mvs, errs, 6, "bilinear", key="det")


def test_outputs_and_strides(pkg, raster):
    """picture alone, count alone, both; at every alignment a byte and a uint16 allow, with and without bytes between the jobs: the
    values, and the bytes around them"""
    for size in ((37, 21), (48, 32)):
        ctx, exp = raster(size)
        psize, csize = pkg.tfilter_sizes(*size)
        jobs = [(0, 0, 3), (17, 15, 2), (0, 5, 1)]
        mvs, errs = fixture_inputs("phases", "mixed", ctx, len(PAIRS), 41)
        dmv, derr = mv_on_device(mvs), err_on_device(errs)
        for which, (off, pad), (coff, cpad) in (("both", (1, 0), (2, 0)), ("both", (3, 5), (6, 2)), ("picture", (7, 1), (0, 0)), ("count", (0, 0), (14, 10)),
                                               ("both", (16, 64), (4, 6))):
            out = out_count = None
            if which != "count":
                big, out = guarded(3, psize, pad, off)
            if which != "picture":
                cbig, cflat = guarded(3, csize, cpad, coff)
                out_count = cflat.view(torch.int16)
                assert out_count.data_ptr() % 16 == coff % 16 and out_count.stride(0) * 2 == csize + cpad
            if which == "count":                                                      # (the wrapper always asks for the picture)
                torch.cuda.synchronize()
                assert raw_call(ctx, pkg, jobs, PAIRS, 3, 0, mv=dmv.data_ptr(), mv_stride=dmv.stride(0) * 2, err=derr.data_ptr(), err_stride=derr.stride(0) * 4,
                                cnt=out_count.data_ptr(), cnt_stride=csize + cpad) == 0
                ctx.sync()
            else:
                got = ctx.frames_tfilter(jobs, PAIRS, dmv, derr, 3, out=out, out_count=out_count)
                assert (got[0] is out and got[1] is out_count) if which == "both" else got is out
            for i, j in enumerate(jobs):
                want = exp.get(j, PAIRS, mvs, errs, 3, "sixtap", key="strides")
                assert out is None or np.array_equal(out.cpu().numpy()[i], want[0]), (size, which, off, j)
                assert out_count is None or np.array_equal(count_bits(out_count)[i], want[1]), (size, which, coff, j)
            if out is not None:
                assert_guards_intact(big, 3, psize, pad, off, what=("picture", size, off, pad))
            if out_count is not None:
                assert_guards_intact(cbig, 3, csize, cpad, coff, what=("count", size, coff, cpad))


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_jobs_from_tiles(pkg, name, monkeypatch):
    """frames a large launch left as tiles: centre and sources as tiles, tiles mixed with an uploaded raster frame in both roles, a
    frame over itself, a frame buffer never written; no raster pool is made for them and the context's memory does not change.
    Expected values from pictures downloaded AFTER the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 4
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        before = ctx.memory_usage()
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        pairs = [(0, b) for b in range(n)] + [(1, 1), (1, n + 1), (n + 1, n + 1), (2, 3), (n + 1, 0)]
        jobs = [(0, 0, n), (1, n, 2), (n + 1, n + 2, 1), (2, n + 3, 1), (0, 1, 2), (n + 1, n + 4, 1)]
        mvs = [TR.fixture_mv("phases", rows, cols, 51, k) for k in range(len(pairs))]
        assert len(pairs) == 2 * n + 1
        dmv = mv_on_device(mvs)
        first = [ctx.frames_tfilter(jobs, pairs, m, None, 3, f, want_count=True) for m, f in ((None, "sixtap"), (dmv, "sixtap"), (dmv, "bilinear"))]
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        rnd = np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                                             # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        before = ctx.memory_usage()
        mixed_pairs = [(k, n) for k in range(n)] + [(n, k) for k in range(n)] + [(n, n)]
        mixed_jobs = [(k, k, 1) for k in range(n)] + [(n, n, n + 1), (n, 2 * n, 1)]
        mixed = ctx.frames_tfilter(mixed_jobs, mixed_pairs, dmv, None, 3, want_count=True)
        ctx.sync()
        assert ctx.memory_usage() == before
        never = [np.zeros((ctx.g.aligned_h >> s, ctx.g.aligned_w >> s), np.uint8) for s in (0, 1, 1)]
        w, h = ctx.width, ctx.height
        exp = Expected([coded(ctx, k) for k in range(n + 1)] + [never], (w, h))
        assert nsrc < 2 or not np.array_equal(exp.pictures[0][0], exp.pictures[1][0])
        for (pic, cnt), (m, f) in zip(first, ((None, "sixtap"), (mvs, "sixtap"), (mvs, "bilinear"))):
            pic, cnt = pic.cpu().numpy(), count_bits(cnt)
            for i, j in enumerate(jobs):
                want = exp.get(j, pairs, m, None, 3, f, key="tiles")
                assert np.array_equal(pic[i], want[0]) and np.array_equal(cnt[i], want[1]), (name, j, f, m is None)
        pic, cnt = first[0][0].cpu().numpy(), count_bits(first[0][1])
        assert not pic[2].any() and (cnt[2] == 32).all()                                             # never written: zeros over zeros
        pic, cnt = mixed[0].cpu().numpy(), count_bits(mixed[1])
        for i, j in enumerate(mixed_jobs):
            want = exp.get(j, mixed_pairs, mvs, None, 3, "sixtap", key="mixed")
            assert np.array_equal(pic[i], want[0]) and np.array_equal(cnt[i], want[1]), (name, j)
        check(ctx, exp, mixed_jobs, mixed_pairs, (name, "after the downloads"), mvs, None, 3, key="mixed")     # ... every frame in raster form
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["raster", "tiles"])
def test_decoded_content(pkg, form, monkeypatch):
    """consecutive frames of an inter stream as the decoder left them, each filtered over itself and its two neighbours, through
    the three calls; both forms give the same bits"""
    P = pkg
    ctx, shown = decode_stream(P, "p_odd_130x98", form, monkeypatch)
    try:
        pairs = [(shown[c], shown[c + d]) for c in (1, 2) for d in (-1, 0, 1)]
        jobs = [(shown[1], 0, 3), (shown[2], 3, 3)]
        whole, _ = ctx.frames_motion(pairs, 8, planes=())
        mv, val = ctx.frames_subpel(pairs, start=whole, planes=("val",))
        pic, cnt = ctx.frames_tfilter(jobs, pairs, mv, val, 3, want_count=True)
        ctx.sync()
        exp = Expected({k: coded(ctx, k) for k in set(shown)}, (ctx.width, ctx.height))
        mvs, errs = list(mv.cpu().numpy().astype(np.int64)), list(val.cpu().numpy().view(np.uint32)[:, 0])
        for i, j in enumerate(jobs):
            want = exp.get(j, pairs, mvs, errs, 3, "sixtap", key=form)
            assert np.array_equal(pic.cpu().numpy()[i], want[0]) and np.array_equal(count_bits(cnt)[i], want[1]), (form, j)
        assert (count_bits(cnt) >= 32).all()              # the centre is among its sources
    finally:
        ctx.close()


def test_the_wrapper(pkg, raster):
    """shapes and types, out / out_count filled and returned, the two shapes of err, what the wrapper and the call refuse"""
    P = pkg
    ctx, exp = raster((48, 32))
    psize, csize = P.tfilter_sizes(48, 32)
    assert (psize, csize) == (2304, 4608) and ctx.L.vp8hip_tfilter_count_size(ctx.h) == csize
    pairs, jobs = PAIRS[:4], [(0, 0, 3), (0, 2, 2)]
    alone = ctx.frames_tfilter(jobs, pairs)
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.uint8 and tuple(alone.shape) == (2, psize)
    out = torch.zeros((2, psize), dtype=torch.uint8, device="cuda:0")
    out_count = torch.zeros((2, psize), dtype=torch.int16, device="cuda:0")
    got = ctx.frames_tfilter(jobs, pairs, out=out, out_count=out_count)
    assert got[0] is out and got[1] is out_count and torch.equal(out, alone)
    want = exp.get(jobs[1], pairs)
    assert np.array_equal(out.cpu().numpy()[1], want[0]) and np.array_equal(count_bits(out_count)[1], want[1])
    y, u, v = P.split_i420(out, 48, 32)
    assert tuple(y.shape) == (2, 32, 48) and tuple(u.shape) == (2, 16, 24) == tuple(v.shape)
    mv = torch.zeros((4, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    err3, err4 = torch.zeros((4, 2, 3), dtype=torch.int32, device="cuda:0"), torch.zeros((4, 1, 2, 3), dtype=torch.int32, device="cuda:0")
    for e in (err3, err4):
        assert torch.equal(ctx.frames_tfilter(jobs, pairs, mv, e), alone)
    for bad in (lambda: ctx.frames_tfilter(jobs, pairs, out=out.to(torch.int16)), lambda: ctx.frames_tfilter(jobs, pairs, out=out[:1]),
                lambda: ctx.frames_tfilter(jobs, pairs, out_count=out_count.to(torch.int32)), lambda: ctx.frames_tfilter(jobs, pairs, mv=mv[:3]),
                lambda: ctx.frames_tfilter(jobs, pairs, mv=mv.to(torch.int32)), lambda: ctx.frames_tfilter(jobs, pairs, mv=mv.cpu()),
                lambda: ctx.frames_tfilter(jobs, pairs, err=err3.to(torch.int16)), lambda: ctx.frames_tfilter(jobs, pairs, err=err4[:, :, :1]),
                lambda: ctx.frames_tfilter(jobs, pairs, err=err3.cpu()), lambda: ctx.frames_tfilter(jobs, pairs, err=torch.zeros((4, 2, 2, 3), dtype=torch.int32,
                                                                                                                                  device="cuda:0"))):
        with pytest.raises(ValueError):
            bad()
    as_mv = out.view(torch.int16)[:, :24].reshape(2, 2, 2, 6)[:, :, :, :3]                # (not dense: refused by the wrapper)
    with pytest.raises(ValueError):
        ctx.frames_tfilter([(0, 0, 2)], pairs[:2], mv=as_mv)
    for bad in (lambda: ctx.frames_tfilter([(0, 0, 1)], [(0, NFB)]), lambda: ctx.frames_tfilter([(NFB, 0, 1)], [(NFB, 0)]),
                lambda: ctx.frames_tfilter(jobs, pairs, err=out_count.view(torch.int32)[:, :24].reshape(2, 4, 2, 3)[0], out_count=out_count)):
        with pytest.raises(RuntimeError):
            bad()


def test_refusals(pkg):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        psize, csize = P.tfilter_sizes(48, 32)
        msize = esize = 24
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dd = big.data_ptr()
        dc, dm, de = dd + (1 << 18), dd + (1 << 19), dd + (3 << 18)
        assert dd % 16 == 0
        pairs3 = [(0, 1), (0, 0), (0, 1)]

        def call(jobs=((0, 0, 2),), pairs=pairs3, st=3, f=0, lo=10000, hi=20000, mv=None, ms=msize, er=None, es=esize, dst=dd, ds=psize, cnt=dc, cs=csize,
                 n=None, npairs=None):
            return raw_call(ctx, P, list(jobs), list(pairs), st, f, lo, hi, mv, ms, er, es, dst, ds, cnt, cs, n, npairs)
        assert call(n=0) == -2 and call(n=-1) == -2 and call(npairs=0) == -2 and call(npairs=-3) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call(pairs=[(bad, 0), (0, 0), (0, 1)], jobs=[(0, 1, 2)]) == -2 and call(pairs=[(0, bad), (0, 0), (0, 1)], jobs=[(0, 1, 2)]) == -2, bad
            assert call(jobs=[(bad, 0, 1)]) == -2, bad
        for count in (0, -1, 16, 1 << 30, -(1 << 31)):
            assert call(jobs=[(0, 0, count)]) == -2, count
        for first, count in ((-1, 1), (3, 1), (2, 2), (0, 4), ((1 << 31) - 1, 2), (-(1 << 31), 1)):
            assert call(jobs=[(0, first, count)]) == -2, (first, count)
        assert call(pairs=[(0, 1), (1, 0), (0, 0)], jobs=[(0, 0, 2)]) == -2 and call(pairs=[(1, 1)], jobs=[(0, 0, 1)]) == -2      # a pair of another centre
        for st in (-1, 7, 1 << 20):
            assert call(st=st) == -2, st
        for f in (-1, 2, 1 << 20):
            assert call(f=f) == -2, f
        assert call(lo=10, hi=9) == -2 and call(lo=(1 << 32) - 1, hi=0) == -2
        assert call(dst=None, cnt=None) == -2                                # both outputs NULL
        assert call(ds=psize - 1) == -2 and call(cs=csize - 2) == -2 and call(mv=dm, ms=msize - 2) == -2 and call(er=de, es=esize - 4) == -2
        assert call(cnt=dc + 1) == -2 and call(cs=csize + 1) == -2           # cnt: multiples of 2
        assert call(mv=dm + 1) == -2 and call(mv=dm, ms=msize + 1) == -2     # mv: multiples of 2
        assert call(er=de + 2) == -2 and call(er=de, es=esize + 2) == -2     # err: multiples of 4
        assert call(cnt=dd + 8) == -2 and call(dst=dc + csize - 1) == -2     # dst and cnt overlap
        assert call(mv=dd) == -2 and call(mv=dd + psize - 2) == -2 and call(mv=dc + 4) == -2 and call(mv=dc, dst=None) == -2      # ... or the vectors
        assert call(er=dd) == -2 and call(er=dd + psize - 4) == -2 and call(er=dc + 4) == -2 and call(er=dc, dst=None) == -2      # ... or the errors
        one = lambda k: [(0, i, 1) for i in range(k)]
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), [(0, 1)] * k, dst=p, ds=s, cnt=None), dd, psize, 1)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), [(0, 1)] * k, dst=p, ds=s), dd, psize, 1, null=False)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), [(0, 1)] * k, dst=None, cnt=p, cs=s), dc, csize, 2)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), [(0, 1)] * k, cnt=p, cs=s), dc, csize, 2, null=False)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(1), [(0, 1)] * k, mv=p, ms=s), dm, msize, 2, null=False)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(1), [(0, 1)] * k, er=p, es=s), de, esize, 4, null=False)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                             # nothing was enqueued
        # the same calls into memory the test owns are accepted
        big[1 << 19:(1 << 19) + 3 * msize] = 0
        big[3 << 18:(3 << 18) + 3 * esize] = 0
        torch.cuda.synchronize()
        assert call() == 0 and call(cnt=None) == 0 and call(dst=None) == 0 and call(mv=dm) == 0 and call(er=de) == 0 and call(mv=dm, er=de) == 0
        assert call(st=0) == 0 and call(st=6, f=1) == 0 and call(lo=0, hi=0) == 0 and call(lo=5, hi=5) == 0 and call(lo=0, hi=(1 << 32) - 1) == 0
        assert call(jobs=[(0, 0, 3), (0, 1, 2), (0, 2, 1)]) == 0 and call(mv=dm, er=dm) == 0         # (inputs may be the same memory)
        ctx.sync()
    finally:
        ctx.close()


def test_ordering_against_decodes_into_the_same_frame_buffers(pkg):
    """frames_tfilter, then at once a decode of another frame into the centre's frame buffer, which is also a source: the picture
    is that of the frames that were there at the call; and an earlier decode is seen without a sync"""
    P = pkg
    ctx, parser = two_key_frames_queued(P)
    try:
        pairs, jobs = [(0, 0), (0, 1)], [(0, 0, 2)]
        out = ctx.frames_tfilter(jobs, pairs, strength=6, want_count=True)     # behind the decode of frame 0 ...
        ctx.decode([(1, 0, None)], P.STAGE_ALL)                               # ... and in front of the decode of frame 1 into the same frame buffer
        got_pic, got_cnt = out[0].cpu().numpy(), count_bits(out[1])
        after = ctx.frames_tfilter(jobs, pairs, strength=6, want_count=True)
        after_pic, after_cnt = after[0].cpu().numpy(), count_bits(after[1])
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        exp = Expected([coded(ctx, 0), coded(ctx, 1)], (ctx.width, ctx.height))
        assert not np.array_equal(exp.pictures[0][0], exp.pictures[1][0])
        want = exp.get(jobs[0], pairs, strength=6)
        assert np.array_equal(got_pic[0], want[0]) and np.array_equal(got_cnt[0], want[1])
        assert np.array_equal(after_pic[0], TR.pack(exp.pictures[1], ctx.width, ctx.height)) and (after_cnt == 64).all()
    finally:
        parser.close()
        ctx.close()


def test_no_new_device_memory_and_sources_untouched(pkg):
    """the call adds no device memory; no frame buffer and no input tensor is written"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        w, h = 130, 98
        ctx.configure(w, h, 3, 1)
        rng = np.random.default_rng(98)
        bufs = [rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8) for _ in range(3)]
        for k, b in enumerate(bufs):
            ctx.upload_frame(k, b)
        ctx.sync()
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        size = P.tfilter_sizes(w, h)[0]
        out = torch.empty((2, size), dtype=torch.uint8, device="cuda:0")
        out_count = torch.empty((2, size), dtype=torch.int16, device="cuda:0")
        mv = torch.full((3, 2, rows, cols), 21, dtype=torch.int16, device="cuda:0")
        err = torch.full((3, rows, cols), 12000, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        md5 = [hashlib.md5(ctx.download_full(k).tobytes()).hexdigest() for k in range(3)]
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        for filt in TR.FILTERS:
            ctx.frames_tfilter([(0, 0, 2), (1, 2, 1)], [(0, 1), (0, 2), (1, 1)], mv, err, 4, filt, out=out, out_count=out_count)
            ctx.sync()
            assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            got = ctx.download_full(k)
            assert np.array_equal(got, b) and hashlib.md5(got.tobytes()).hexdigest() == md5[k]
        assert (mv.cpu().numpy() == 21).all() and (err.cpu().numpy() == 12000).all()
    finally:
        ctx.close()
