"""GPU (-m gpu): the structural similarity of picture pairs in device memory (vp8hip_frames_ssim_async; Vp8Hip.frames_ssim;
csrc/hip/vp8_ssim.hip), bit for bit against the numpy restatement (tests/ssim_reference.py) applied to the planes
vp8hip_frame_download gives: the Q32 totals and counts, and the F32 / F16 maps.  torch is imported here, before the package loads
libvpx's library: one HIP runtime per process."""
import ctypes
import itertools
import math

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import (assert_destinations_refused, assert_guards_intact, decode_stream, guarded, large_launch, picture_into,
                              two_key_frames_queued)
import scale_reference as SC
import ssim_reference as SR

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 33), (25, 9), (9, 9), (67, 45), (130, 98), (8208, 16), (24, 1037)]
PLANE_SETS = [("y", "u", "v"), ("y",), ("u", "v"), 5, ("v",), 3]
TORCH_DTYPE = {1: torch.float16, 2: torch.float32}


def map_bits(t):
    """a map tensor on the device -> its bit patterns"""
    return t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32)


def ref_bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


class Expected:
    """the restatement over downloaded planes, each pair computed once: all three planes' scores and F32 values"""

    def __init__(self, planes):
        self.planes, self.memo = planes, {}

    def pair(self, a, b):
        if (a, b) not in self.memo:
            vals = [SR.values(self.planes[a][p], self.planes[b][p]) for p in range(3)]
            self.memo[(a, b)] = (np.array([[int(SR.q32(v).sum(dtype=np.int64)), v.size] for v in vals], np.int64), vals)
        return self.memo[(a, b)]

    def scores(self, job, which):
        mask = SR.mask_of(which)
        return self.pair(*job)[0][[p for p in range(3) if mask >> p & 1]]

    def map(self, job, which, dt):
        mask = SR.mask_of(which)
        flat = np.concatenate([self.pair(*job)[1][p].astype(np.float32).ravel() for p in range(3) if mask >> p & 1])
        return ref_bits(flat if dt == 2 else flat.astype(np.float16))


def check(ctx, exp, jobs, which, dt, what):
    """frames_ssim over `jobs` twice: the same bits, and those of the restatement"""
    first = ctx.frames_ssim(jobs, which, None if not dt else TORCH_DTYPE[dt])
    again = ctx.frames_ssim(jobs, which, None if not dt else TORCH_DTYPE[dt])
    sc, mp = first if dt else (first, None)
    sc2, mp2 = again if dt else (again, None)
    assert sc.dtype == torch.int64 and tuple(sc.shape) == (len(jobs), bin(SR.mask_of(which)).count("1"), 2)
    got = sc.cpu().numpy()
    assert np.array_equal(got, sc2.cpu().numpy()), what
    for i, j in enumerate(jobs):
        assert np.array_equal(got[i], exp.scores(j, which)), (what, which, j, got[i], exp.scores(j, which))
    if dt:
        assert mp.dtype == TORCH_DTYPE[dt] and mp.dim() == 2 and mp.shape[0] == len(jobs)
        bits = map_bits(mp)
        assert np.array_equal(bits, map_bits(mp2)), what
        for i, j in enumerate(jobs):
            assert np.array_equal(bits[i], exp.map(j, which, dt)), (what, which, dt, j)
    return got


def raw_call(ctx, P, jobs, mask, dt, scores=None, scores_stride=0, mp=None, map_stride=0, n=None):
    """vp8hip_frames_ssim_async itself, on pointers: -> its status"""
    arr = (P.HistJob * max(len(jobs), 1))(*jobs)
    vp = ctypes.c_void_p
    return ctx.L.vp8hip_frames_ssim_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(P.SsimParams(mask, dt)),
                                          vp(scores) if scores else None, scores_stride, vp(mp) if mp else None, map_stride)


def upload_pictures(ctx, w, h, seed):
    """six frame buffers: noise, other noise, the first perturbed by a few levels, flat 0, flat 255, a ramp -- each picture inside a
    border of other bytes, which must not be read into any sum; -> the planes as downloaded"""
    g = ctx.g
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rng = np.random.default_rng(seed)
    shapes = ((h, w), (ch, cw), (ch, cw))
    bufs = [rng.integers(0, 256, g.frame_size, dtype=np.uint8), rng.integers(0, 256, g.frame_size, dtype=np.uint8)]
    noise = [SC.planes(bufs[0], g)[p][:s[0], :s[1]].astype(np.int16) for p, s in enumerate(shapes)]
    pert = [np.clip(n + rng.integers(-3, 4, n.shape), 0, 255).astype(np.uint8) for n in noise]
    bufs.append(picture_into(rng.integers(0, 256, g.frame_size, dtype=np.uint8), g, pert))
    bufs.append(picture_into(np.full(g.frame_size, 0x77, np.uint8), g, [np.zeros(s, np.uint8) for s in shapes]))
    bufs.append(picture_into(np.full(g.frame_size, 0x31, np.uint8), g, [np.full(s, 255, np.uint8) for s in shapes]))
    bufs.append(picture_into(np.full(g.frame_size, 200, np.uint8), g,
                             [(np.arange(s[0] * s[1]) * k % 256).astype(np.uint8).reshape(s) for k, s in zip((1, 3, 7), shapes)]))
    for k, b in enumerate(bufs):
        ctx.upload_frame(k, b)
    planes = [ctx.download_planes(k) for k in range(len(bufs))]
    assert not planes[3][0].any() and (planes[4][0] == 255).all() and np.array_equal(planes[2][0], pert[0])
    return planes


@pytest.mark.parametrize("size", SIZES)
def test_pairs_from_raster(pkg, size):
    """uploaded frame buffers at sizes with and without chroma windows, widths that are no multiple of 4, one window row, more strips
    than one (8208) and many bands (1037 rows: the seams between workgroups); noise / noise, noise / perturbed, flat 0 / flat 255,
    ramp / noise and a frame against itself; the plane sets in rotation; scores alone, map alone, both; F32 and F16; every call twice"""
    P = pkg
    w, h = size
    sets = itertools.cycle(PLANE_SETS)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 6, 1)
        exp = Expected(upload_pictures(ctx, w, h, w * 137 + h))
        jobs = [(0, 1), (0, 2), (3, 4), (5, 0), (0, 0), (1, 0), (4, 3), (0, 2)]
        cw, ch = (w + 1) // 2, (h + 1) // 2
        counts = [a * b if a and b else 0 for a, b in (SR.windows(w, h), SR.windows(cw, ch), SR.windows(cw, ch))]
        for dt in (0, 2, 1):
            which = next(sets)
            mask = SR.mask_of(which)
            if dt and not SR.map_elems(w, h, mask):      # (no window in any plane asked for: the map is refused, the scores are not)
                with pytest.raises(ValueError):
                    ctx.frames_ssim(jobs, which, TORCH_DTYPE[dt])
                dt = 0
            got = check(ctx, exp, jobs, which, dt, (size, which, dt))
            assert (got[:, :, 1] == [c for b, c in enumerate(counts) if mask >> b & 1]).all()
            assert (got[4, :, 0] == got[4, :, 1] << 32).all()                      # a frame against itself: count << 32 exactly
            assert np.array_equal(got[0], got[5]) and np.array_equal(got[2], got[6])           # symmetric in (fb, ref_fb)
        if counts[1] == 0:
            assert (check(ctx, exp, jobs, ("u", "v"), 0, size) == 0).all()          # no chroma windows: count 0, total 0
        # the map alone, through the call itself
        for dt in (2, 1):
            elems = SR.map_elems(w, h, 1)
            out = torch.full((len(jobs), elems), -7, dtype=TORCH_DTYPE[dt], device="cuda:0")
            torch.cuda.synchronize()
            assert raw_call(ctx, P, jobs, 1, dt, mp=out.data_ptr(), map_stride=elems * out.element_size()) == 0
            ctx.sync()
            bits = map_bits(out)
            for i, j in enumerate(jobs):
                assert np.array_equal(bits[i], exp.map(j, 1, dt)), (size, dt, j)
    finally:
        ctx.close()


def test_both_reduction_shapes(pkg):
    """one job at 352x288 -- its pieces shared by workgroups, which add to scores the fill kernel has set --; 300 jobs there, each
    shared by a few workgroups whose pieces come from all three planes; 2100 jobs, more than eight launches and a remainder, each
    owned by one workgroup, which walks all the job's pieces and stores; 600 jobs of 16x16, one piece each.  Which shape a call
    takes is the plan's arithmetic (vp8hip_ssim_share), asserted here so that neither goes untested silently"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        w, h = 352, 288
        ctx.configure(w, h, 6, 1)
        exp = Expected(upload_pictures(ctx, w, h, 352))
        rng = np.random.default_rng(288)
        assert ctx.ssim_share(1) == 16 and ctx.ssim_share(1, ("y",)) == 10 and ctx.ssim_share(1, ("u", "v")) == 6
        for j in ((0, 1), (0, 2), (3, 4), (2, 2)):
            check(ctx, exp, [j], 7, 2, ("one job", j))
        check(ctx, exp, [(5, 0)], ("u",), 0, "one job, one chroma plane")
        for n, share in ((300, 7), (2100, 1)):
            assert ctx.ssim_share(n) == share
            jobs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 6, n), rng.integers(0, 6, n))]
            check(ctx, exp, jobs, 7, 1 if n == 300 else 0, (n, share))
        assert ctx.ssim_share(0) == 0 and ctx.ssim_share(5, 8) == 0
    finally:
        ctx.close()
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(16, 16, 6, 1)
        exp = Expected(upload_pictures(ctx, 16, 16, 16))
        assert ctx.ssim_share(1) == 1 and ctx.ssim_share(600) == 1
        rng = np.random.default_rng(16)
        jobs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 6, 600), rng.integers(0, 6, 600))]
        check(ctx, exp, jobs, 7, 2, "16x16")
        check(ctx, exp, jobs[:1], ("y",), 1, "16x16, one job")
        # the owning workgroup's 16-byte store into scores that are aligned to 8 and no further
        big, flat = guarded(5, 48, 8, 8)
        out = flat.view(torch.int64).unflatten(1, (3, 2))
        assert out.data_ptr() % 16 == 8 and ctx.frames_ssim(jobs[:5], out_scores=out) is out
        got = out.cpu().numpy()
        for i, j in enumerate(jobs[:5]):
            assert np.array_equal(got[i], exp.scores(j, 7)), j
        assert_guards_intact(big, 5, 48, 8, 8)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_pairs_from_tiles(pkg, name, monkeypatch):
    """frames a large launch left as tiles: tiles against tiles, tiles against an uploaded raster frame in both orders, a frame against
    itself; no raster pool is made for them and the context's memory does not change.  Expected values from planes downloaded AFTER
    the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 6
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        before = ctx.memory_usage()
        tiles = [(a, b) for a in range(n) for b in range(n) if (a + 2 * b) % 3 == 0]
        both = ctx.frames_ssim(tiles, ("y", "v"), torch.float32)
        alone = ctx.frames_ssim(tiles)
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        rnd = np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                                             # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        before = ctx.memory_usage()
        mixed_jobs = [(k, n) for k in range(n)] + [(n, k) for k in range(n)] + [(n, n)]
        mixed = ctx.frames_ssim(mixed_jobs, 7, torch.float16)
        ctx.sync()
        assert ctx.memory_usage() == before
        exp = Expected([ctx.download_planes(k) for k in range(n + 1)])
        assert nsrc < 2 or not np.array_equal(exp.planes[0][0], exp.planes[1][0])
        sc, mp = both[0].cpu().numpy(), map_bits(both[1])
        for i, j in enumerate(tiles):
            assert np.array_equal(sc[i], exp.scores(j, 5)) and np.array_equal(mp[i], exp.map(j, 5, 2)), (name, j)
            if j[0] == j[1]:
                assert (sc[i, :, 0] == sc[i, :, 1] << 32).all()
        sc = alone.cpu().numpy()
        for i, j in enumerate(tiles):
            assert np.array_equal(sc[i], exp.scores(j, 7)), (name, j)
        sc, mp = mixed[0].cpu().numpy(), map_bits(mixed[1])
        for i, j in enumerate(mixed_jobs):
            assert np.array_equal(sc[i], exp.scores(j, 7)) and np.array_equal(mp[i], exp.map(j, 7, 1)), (name, j)
        assert np.array_equal(sc[0], sc[n])                                  # symmetric, whichever of the two is tiles
        check(ctx, exp, mixed_jobs, 7, 2, (name, "after the downloads"))     # ... and with every frame in raster form
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["raster", "tiles"])
def test_decoded_content(pkg, form, monkeypatch):
    """consecutive frames of an inter stream, frame k against frame k - 1, as the decoder left them"""
    P = pkg
    ctx, shown = decode_stream(P, "p_odd_130x98", form, monkeypatch)
    try:
        jobs = [(shown[k], shown[k - 1]) for k in range(1, len(shown))]
        assert len(jobs) >= 3
        sc, mp = ctx.frames_ssim(jobs, 7, torch.float32)
        ctx.sync()
        exp = Expected({k: ctx.download_planes(k) for k in set(shown)})
        got, bits = sc.cpu().numpy(), map_bits(mp)
        for i, j in enumerate(jobs):
            assert np.array_equal(got[i], exp.scores(j, 7)) and np.array_equal(bits[i], exp.map(j, 7, 2)), (form, j)
        mean = P.ssim_mean(sc)
        assert (np.abs(mean) <= 1).all() and not (mean == 1).all()
    finally:
        ctx.close()


def test_the_wrapper(pkg):
    """ssim_mean is NaN exactly where the count is 0 and within the header's bound of vp8_ssim2's way of summing; split_ssim_map's
    views; ssim_combined against the two formulas; out_scores / out_map are filled and returned"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        for (w, h) in ((16, 16), (67, 45)):
            ctx.configure(w, h, 6, 1)
            exp = Expected(upload_pictures(ctx, w, h, w))
            jobs = [(0, 1), (0, 2), (0, 0)]
            sc, mp = ctx.frames_ssim(jobs, map_dtype=torch.float32)
            mean = P.ssim_mean(sc)
            cnt = sc.cpu().numpy()[:, :, 1]
            assert mean.shape == (3, 3) and np.array_equal(np.isnan(mean), cnt == 0)
            assert (np.isnan(mean[:, 1:]).all()) == ((w, h) == (16, 16))
            for i, (a, b) in enumerate(jobs):
                for p in range(3):
                    if cnt[i, p]:
                        ref = SR.raster_mean(exp.planes[a][p], exp.planes[b][p])
                        assert abs(mean[i, p] - ref) <= 2.0 ** -33 + int(cnt[i, p]) * 2.0 ** -52
            assert (mean[2][~np.isnan(mean[2])] == 1.0).all()
            views = P.split_ssim_map(mp, w, h)
            cw, ch = (w + 1) // 2, (h + 1) // 2
            assert [tuple(v.shape) for v in views] == [(3,) + SR.windows(pw, ph)[::-1] if all(SR.windows(pw, ph)) else (3, 0, 0)
                                                       for pw, ph in ((w, h), (cw, ch), (cw, ch))]
            for p, v in enumerate(views):
                for i, j in enumerate(jobs):
                    assert np.array_equal(ref_bits(v[i].cpu().numpy().copy()), ref_bits(exp.pair(*j)[1][p].astype(np.float32)))
            if (w, h) == (67, 45):
                for how, f in (("ssimg", lambda a, b, c: (a * 4 + b + c) / 6), ("ssim", lambda a, b, c: a * .8 + .1 * (b + c))):
                    assert np.array_equal(P.ssim_combined(mean, how), f(mean[:, 0], mean[:, 1], mean[:, 2]))
                assert P.ssim_combined(mean)[2] == 1.0 and P.ssim_combined(mean)[0] < P.ssim_combined(mean)[1] < 1.0
                out_sc = torch.zeros((3, 2, 2), dtype=torch.int64, device="cuda:0")
                out_mp = torch.zeros((3, SR.map_elems(w, h, 6)), dtype=torch.float16, device="cuda:0")
                got = ctx.frames_ssim(jobs, ("v", "u"), torch.float16, out_scores=out_sc, out_map=out_mp)
                assert got[0] is out_sc and got[1] is out_mp
                assert np.array_equal(out_sc.cpu().numpy(), sc.cpu().numpy()[:, 1:]) and np.array_equal(map_bits(out_mp)[1], exp.map((0, 2), 6, 1))
                for bad in (lambda: ctx.frames_ssim(jobs, 7, None, out_map=out_mp), lambda: ctx.frames_ssim(jobs, 7, torch.float16, out_map=out_mp),
                            lambda: ctx.frames_ssim(jobs, 6, torch.float32, out_map=out_mp), lambda: ctx.frames_ssim(jobs, 7, out_scores=out_sc),
                            lambda: ctx.frames_ssim(jobs, 6, out_scores=out_sc.to(torch.int32))):
                    with pytest.raises(ValueError):
                        bad()
                for bad in (lambda: ctx.frames_ssim([(0, 6)]), lambda: ctx.frames_ssim([(6, 0)])):
                    with pytest.raises(RuntimeError):
                        bad()
    finally:
        ctx.close()


def test_guarded_destinations(pkg):
    """scores at offsets 8 and 16 of their allocation, 0, 8 and 24 bytes apart, and maps at every alignment their element allows:
    the values, and the bytes around them"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        w, h = 130, 98
        ctx.configure(w, h, 6, 1)
        exp = Expected(upload_pictures(ctx, w, h, 130))
        jobs = [(0, 1), (0, 2), (5, 0)]
        for which, dt, (off, pad), (moff, mpad) in ((7, 2, (8, 0), (4, 0)), (7, 1, (16, 8), (2, 2)), (5, 2, (8, 24), (16, 12)), (("u",), 1, (16, 0), (6, 6)),
                                                    (3, 1, (8, 8), (16, 0)), (("y",), 2, (24, 8), (12, 4))):
            mask = SR.mask_of(which)
            np_, es = bin(mask).count("1"), 2 * dt
            ssize, msize = 16 * np_, SR.map_elems(w, h, mask) * es
            assert (ssize, msize) == P.ssim_sizes(w, h, which, dt)
            sbig, sflat = guarded(3, ssize, pad, off)
            mbig, mflat = guarded(3, msize, mpad, moff)
            out_sc, out_mp = sflat.view(torch.int64).unflatten(1, (np_, 2)), mflat.view(TORCH_DTYPE[dt])
            assert out_sc.data_ptr() % 16 == off % 16 and out_mp.data_ptr() % 16 == moff % 16
            got = ctx.frames_ssim(jobs, which, TORCH_DTYPE[dt], out_scores=out_sc, out_map=out_mp)
            assert got[0] is out_sc and got[1] is out_mp
            sc, bits = out_sc.cpu().numpy(), map_bits(out_mp)
            for i, j in enumerate(jobs):
                assert np.array_equal(sc[i], exp.scores(j, which)) and np.array_equal(bits[i], exp.map(j, which, dt)), (which, dt, off, pad, j)
            assert_guards_intact(sbig, 3, ssize, pad, off, what=("scores", which, off, pad))
            assert_guards_intact(mbig, 3, msize, mpad, moff, what=("map", which, moff, mpad))
    finally:
        ctx.close()


def test_refusals(pkg):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    small = P.Vp8Hip(0)
    try:
        w, h = 67, 45
        ctx.configure(w, h, 2, 1)
        small.configure(16, 16, 1, 1)
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        small.upload_frame(0, rng.integers(0, 256, small.g.frame_size, dtype=np.uint8))
        ssize, msize = P.ssim_sizes(w, h, 7, 2)
        assert ssize == 48 and msize == 4 * SR.map_elems(w, h) and msize % 8 == 0
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        dm = d + (1 << 19)
        assert d % 16 == 0

        def call(jobs=((0, 1),), mask=7, dt=2, sc=d, ss=ssize, mp=dm, ms=msize, n=None, c=ctx):
            return raw_call(c, P, list(jobs), mask, dt, sc, ss, mp, ms, n)
        assert call(n=0) == -2 and call(n=-1) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call([(bad, 0)]) == -2 and call([(0, bad)]) == -2 and call([(0, 1), (1, bad)]) == -2, bad
        for mask in (0, 8, 64, 0xf, 1 << 31):
            assert call(mask=mask) == -2, mask
        assert call(sc=None, mp=None) == -2                                  # both destinations NULL
        assert call(dt=0) == -2 and call(dt=3) == -2 and call(dt=-1) == -2   # a map with no type; unknown types
        assert call(dt=3, mp=None) == -2 and call(dt=-1, mp=None) == -2      # ... also without a map
        assert call([(0, 0)], mask=6, ss=32, c=small) == -2                  # a map of planes without windows (16x16 chroma)
        assert call([(0, 0)], mask=6, ss=32, mp=None, dt=0, c=small) == 0    # (their scores alone are fine: count 0)
        assert call(ss=ssize - 8) == -2 and call(ms=msize - 4) == -2         # strides below the sizes
        assert call(mask=1, ss=8) == -2
        assert call(sc=d + 4) == -2 and call(ss=ssize + 4) == -2             # scores: multiples of 8
        assert call(mp=dm + 2) == -2 and call(ms=msize + 2) == -2            # an F32 map: multiples of 4
        assert call(dt=1, mp=dm + 1, ms=msize // 2) == -2 and call(dt=1, ms=msize // 2 + 1) == -2
        assert call(mp=d + 16) == -2 and call(sc=dm + msize - 8, n=1) == -2  # scores and map overlap
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, sc=p, ss=s, mp=None), d, ssize, 8)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, sc=p, ss=s), d, ssize, 8, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, sc=None, mp=p, ms=s), dm, msize, 4)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, mp=p, ms=s), dm, msize, 4, null=False)
        assert_destinations_refused(ctx, lambda n, p, s: call([(0, 1)] * n, dt=1, sc=None, mp=p, ms=s), dm, msize // 2, 2)
        ctx.sync()
        small.sync()
        torch.cuda.synchronize()
        a = big.cpu().numpy()
        assert (a[32:] == 0x5C).all()                                        # nothing was enqueued but the one accepted call
        assert a[:32].view(np.int64).tolist() == [0, 0, 0, 0]
        # the same calls into memory the test owns are accepted
        assert call() == 0 and call(sc=None) == 0 and call(mp=None, dt=0) == 0 and call(mp=None) == 0 and call(dt=1) == 0
        ctx.sync()
    finally:
        ctx.close()
        small.close()


def test_ordering_against_a_decode_into_the_same_frame_buffer(pkg):
    """frames_ssim, then at once a decode of another frame into one of the pair's frame buffers: the scores are those of the pictures
    that were there at the call; and an earlier decode is seen without a sync"""
    P = pkg
    ctx, parser = two_key_frames_queued(P)
    try:
        out = ctx.frames_ssim([(0, 1), (1, 0)], 7, torch.float32)        # behind the decode of frame 0 ...
        ctx.decode([(1, 0, None)], P.STAGE_ALL)                           # ... and in front of the decode of frame 1 into the same frame buffer
        got, bits = out[0].cpu().numpy(), map_bits(out[1])
        after = ctx.frames_ssim([(0, 1)]).cpu().numpy()
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        exp = Expected([ctx.download_planes(0), ctx.download_planes(1)])
        assert not np.array_equal(exp.planes[0][0], exp.planes[1][0])
        for i, j in enumerate(((0, 1), (1, 0))):
            assert np.array_equal(got[i], exp.scores(j, 7)) and np.array_equal(bits[i], exp.map(j, 7, 2)), j
        assert (after[0, :, 0] == after[0, :, 1] << 32).all() and not np.array_equal(after[0], got[0])
        assert not math.isnan(P.ssim_combined(P.ssim_mean(got))[0])
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
        out_sc = torch.empty((2, 3, 2), dtype=torch.int64, device="cuda:0")
        out_mp = torch.empty((2, SR.map_elems(w, h)), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        ctx.frames_ssim([(0, 1), (1, 1)], 7, torch.float32, out_scores=out_sc, out_map=out_mp)
        ctx.sync()
        assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            assert np.array_equal(ctx.download_full(k), b)
    finally:
        ctx.close()
