"""GPU (-m gpu): a trace inverted in device memory (vp8hip_trace_invert_async, vp8hip_trace_cover_async; Vp8Hip.trace_invert,
Vp8Hip.trace_cover; csrc/hip/vp8_trace_invert.hip), dword for dword and bit for bit against the numpy restatement
(tests/invert_reference.py).  Most cases need no decode: a context of the size and traces placed in the pool.  torch is imported
here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes
import functools
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import TORCH_DTYPE, assert_destinations_refused, assert_guards_intact, bits, equal_on_device, guarded
import invert_reference as I
import trace_reference as R
from trace_testlib import check_tensor as entry_check_tensor, dwords, random_trace, to_pool, traced_stream, whole_pixel_frame

pytestmark = pytest.mark.gpu

SCALES = [None, (1.0, 0.5), 1.0 / 255, (-1.0 / 3, 3.0e4), (1.0285249948501587, 1e-3)]
PLANE_SETS = [("count", "seen"), ("seen",), 1, ("seen", "count"), 2]
GRIDS = lambda w, h: ((0, 0), (224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h))     # noqa: E731
FILL = 0xA5A5A5A5


count_dwords = dwords                                         # int32 [..., h, w] on the device -> numpy uint32 [..., h, w]
to_count = functools.partial(to_pool, dtype=np.int32)         # numpy uint32 [h, w] -> int32 [h, w] on the device
# entries idx of the COUNT pool through trace_cover against the restatement on `want` (their counts, numpy)
check_tensor = functools.partial(entry_check_tensor, "trace_cover", I.tensor, 2)


def three_hops(P, rng, w, h):
    """a key frame's trace and three hops of whole_pixel_frame chained behind it, references mixed; -> the four traces"""
    t = [R.identity(w, h)]
    for _ in range(3):
        hdr, mbs, mvs = whole_pixel_frame(P, w, h, rng)
        t.append(R.trace(hdr, mbs, mvs, [t[-1], t[0], t[max(len(t) - 2, 0)]]))
    return t


def crafted(P, w, h):
    """the traces of the crafted cases: identity, constant, seeded random positions, raw random dwords (negative and far outside: every
    one clamped), positions a few pixels past every edge, and the three hops of a chain"""
    rng = np.random.default_rng(7)
    return [R.identity(w, h), np.full((h, w), R.pack(0, 0), np.uint32), random_trace(rng, w, h),
            rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32),
            R.pack(rng.integers(-5, w + 5, (h, w)), rng.integers(-5, h + 5, (h, w)))] + three_hops(P, rng, w, h)[1:]


@pytest.mark.parametrize("size", [(16, 16), (17, 9), (130, 98), (20, 20), (67, 45), (176, 144)])
def test_crafted_traces_both_paths_every_output_set(pkg, size):
    """the crafted traces in a guarded pool, inverted into guarded pools with a guard entry on both sides of every destination: FIRST
    only, COUNT only and both; pools on 16 bytes and 4 bytes off them, with strides that are and are not multiples of 16 -- the two
    paths of the fill, and of the -DINVERT_LANE_QUADS variant's load, which d_w % 4 of 1 and 2 also send down the dword path.
    Nothing but the destinations is written and the trace pool is unchanged; a tensor of each COUNT entry, sizes, types, planes and
    scales in rotation"""
    P = pkg
    w, h = size
    traces = crafted(P, w, h)
    want = [I.invert(t, w, h) for t in traces]
    m = len(traces)
    every = np.stack([c for _, c in want])
    assert (every == 0).any() and (every == 1).any() and (every >= 2).any() and (w * h <= 255 or (every > 255).any())
    assert want[1][1][0, 0] == w * h and want[1][0][0, 0] == 0 and (want[1][1].ravel()[1:] == 0).all()
    assert np.array_equal(want[0][0], traces[0]) and (want[0][1] == 1).all()
    esize = 4 * w * h
    nout = 2 * m + 1
    jobs = [(k, 2 * k + 1) for k in range(m)]
    sweep = itertools.cycle(itertools.product(GRIDS(w, h), ("u8", "f32", "f16")))
    scales, plane_sets = itertools.cycle(SCALES), itertools.cycle(PLANE_SETS)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        before = ctx.memory_usage()
        for off, pad in ((16, 0), (4, 4), (16, 16), (4, 12)):
            tbig, tflat = guarded(m, esize, pad, off)
            pool = tflat.view(torch.int16).unflatten(1, (h, w, 2))
            assert pool.data_ptr() % 16 == off % 16 and pool.stride(0) * 2 == esize + pad
            for k in range(m):
                pool[k] = to_pool(traces[k])
            for outputs in ("both", "first", "count"):
                fbig, fflat = guarded(nout, esize, pad, off)
                cbig, cflat = guarded(nout, esize, pad, off)
                first = fflat.view(torch.int16).unflatten(1, (h, w, 2)) if outputs != "count" else None
                count = cflat.view(torch.int32).unflatten(1, (h, w)) if outputs != "first" else None
                got = ctx.trace_invert(pool, jobs, first, count)
                assert got[0] is first and got[1] is count
                if first is not None:
                    f = dwords(first)
                    for k in range(m):
                        assert np.array_equal(f[2 * k + 1], want[k][0]), (size, off, pad, outputs, k)
                    assert (f[0::2] == FILL).all(), (size, off, pad, outputs)
                if count is not None:
                    c = count_dwords(count)
                    for k in range(m):
                        assert np.array_equal(c[2 * k + 1], want[k][1]), (size, off, pad, outputs, k)
                    assert (c[0::2] == FILL).all(), (size, off, pad, outputs)
                    (dw, dh), dtype = next(sweep)
                    check_tensor(ctx, count, [2 * k + 1 for k in range(m)], [cw for _, cw in want], dw, dh, dtype, next(plane_sets), next(scales),
                                 what=(size, off, pad))
                assert_guards_intact(fbig, nout, esize, pad, off, what=(size, off, pad, outputs, "first"))
                assert_guards_intact(cbig, nout, esize, pad, off, what=(size, off, pad, outputs, "count"))
                if outputs == "first":
                    assert (cbig == 0xA5).all()
                if outputs == "count":
                    assert (fbig == 0xA5).all()
            t = dwords(pool)
            for k in range(m):
                assert np.array_equal(t[k], traces[k]), (size, off, pad, k)
            assert_guards_intact(tbig, m, esize, pad, off, what=(size, off, pad, "traces"))
        ctx.sync()
        assert ctx.memory_usage() == before
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["tiles", "raster"])
@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98"])
def test_streams_inverted_right_behind_the_trace(pkg, name, form, monkeypatch):
    """every frame of the stream decoded and traced, and its trace inverted in the call queued right behind frames_trace with no
    synchronisation between the two; every frame's FIRST and COUNT against the restatement on trace_reference's traces"""
    P = pkg
    traced = P.Vp8Hip.frames_trace
    made = {}

    def traced_then_inverted(self, jobs, pool):
        out = traced(self, jobs, pool)
        if "pools" not in made:
            made["pools"] = self.cover_pools(pool.shape[0])
            assert made["pools"][0].shape == pool.shape and made["pools"][0].dtype == pool.dtype
            assert made["pools"][1].shape == pool.shape[:3] and made["pools"][1].dtype == torch.int32
        self.trace_invert(pool, [(dst, dst) for _, dst, _ in jobs], *made["pools"])
        return out
    monkeypatch.setattr(P.Vp8Hip, "frames_trace", traced_then_inverted)
    ctx, pool, mine, shown, types = traced_stream(P, name, form, monkeypatch)
    try:
        w, h = ctx.width, ctx.height
        nf = len(types)
        assert types[0] == 0 and sum(types) > 0 and nf > 2
        first, count = made["pools"]
        f, c = dwords(first), count_dwords(count)
        moved = 0
        for i in range(nf):
            wf, wc = I.invert(mine[i], w, h)
            assert np.array_equal(f[i], wf) and np.array_equal(c[i], wc), (name, form, i)
            assert np.array_equal(dwords(pool[i]), mine[i]), (name, form, i)
            moved += int((wc != 1).any())
        assert moved > 0
        sweep = itertools.cycle(itertools.product(GRIDS(w, h), ("u8", "f32", "f16")))
        for i in range(0, nf, 3):
            (dw, dh), dtype = next(sweep)
            check_tensor(ctx, count, [i], [c[i]], dw, dh, dtype, PLANE_SETS[i % 5], SCALES[i % 5], what=(name, form, i))
    finally:
        ctx.close()


def test_batch_of_600_jobs(pkg):
    """600 jobs in one call -- more than one launch's worth and a remainder --, traces drawn with repeats from eight entries, the
    destinations permuted; then a tensor call over 700 indices with repeats"""
    P = pkg
    w, h, nsrc, n = 48, 32, 8, 600
    rng = np.random.default_rng(600)
    traces = crafted(P, w, h)[:nsrc]
    assert len(traces) == nsrc
    inv = [I.invert(t, w, h) for t in traces]
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        pool = ctx.trace_pool(nsrc)
        for k in range(nsrc):
            pool[k] = to_pool(traces[k])
        first, count = ctx.cover_pools(n)
        src = rng.integers(0, nsrc, n)
        dst = rng.permutation(n)
        ctx.trace_invert(pool, [(int(src[i]), int(dst[i])) for i in range(n)], first, count)
        which = np.empty(n, int)
        which[dst] = src
        assert equal_on_device(first.view(torch.int32), [f.reshape(h, w, 1) for f, _ in inv], which.tolist(), "f32") == []
        assert equal_on_device(count, [c for _, c in inv], which.tolist(), "f32") == []
        idx = [int(i) for i in rng.integers(0, n, 700)]
        sc = (0.5, 1.0 / 255)
        out = ctx.trace_cover(count, idx, 45, 37, dtype=torch.float16, scale=sc)
        tens = [I.tensor(c, 45, 37, 3, "f16", sc) for _, c in inv]
        assert equal_on_device(out, tens, [int(which[i]) for i in idx], "f16") == []
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(20, 20), (67, 45)])
def test_tensor_every_size_type_and_plane_set(pkg, size):
    """COUNT entries of every kind of value -- 0, 1, small, 254, 255, 256 and beyond -- as tensors: the five sizes, the three types, the
    plane sets and scales in rotation, into guarded destinations"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w + h)
    counts = [rng.choice(np.array([0, 0, 1, 2, 7, 254, 255, 256, 400, 1 << 27], np.uint32), (h, w)), I.invert(random_trace(rng, w, h), w, h)[1]]
    scales, plane_sets = itertools.cycle(SCALES), itertools.cycle(PLANE_SETS)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        _, pool = ctx.cover_pools(3)
        for k in range(2):
            pool[k + 1] = to_count(counts[k])
        for (dw, dh), dtype in itertools.product(GRIDS(w, h), ("u8", "f32", "f16")):
            gw, gh = (w, h) if dw == 0 else (dw, dh)
            es = {"u8": 1, "f16": 2, "f32": 4}[dtype]
            planes, scale = next(plane_sets), next(scales)
            fsize = bin(I.plane_mask(planes)).count("1") * gh * gw * es
            for off, pad in ((16, 0), (4, 4)):
                off += 1 if dtype == "u8" and pad else 0            # (bytes at an odd address: element by element)
                big, flat = guarded(2, fsize, pad, off, 0x3C)
                out = flat.view(TORCH_DTYPE[dtype]).unflatten(1, (-1, gh, gw))
                check_tensor(ctx, pool, [2, 1], [counts[1], counts[0]], dw, dh, dtype, planes, scale, what=(size, off, pad), out=out)
                assert_guards_intact(big, 2, fsize, pad, off, 0x3C, what=(size, dw, dh, dtype, off, pad))
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(67, 45), (130, 98)])
def test_composition_with_flow_and_gather(pkg, size):
    """a FIRST pool is a pool of traces in the other direction: trace_flow reads it as trace_reference.flow does; the COUNT entry
    gathered along the frame's own trace is at least 1 everywhere; FIRST gathered along the trace is at most the pixel's own packed
    position, with equality on as many pixels as there are anchor pixels with a descendant"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 3 + h)
    traces = [random_trace(rng, w, h)] + three_hops(P, rng, w, h)[2:]
    m = len(traces)
    inv = [I.invert(t, w, h) for t in traces]
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        pool = ctx.trace_pool(m)
        for k in range(m):
            pool[k] = to_pool(traces[k])
        first, count = ctx.trace_invert(pool, [(k, k) for k in range(m)], *ctx.cover_pools(m))
        for (dw, dh), dtype in (((0, 0), "i16"), ((224, 224), "f32"), ((w + 1, h - 1), "f16")):
            sz = {} if dw == 0 else dict(width=dw, height=dh)
            flow = ctx.trace_flow(first, list(range(m)), dtype=TORCH_DTYPE[dtype], scale=None if dtype == "i16" else (0.5, 0.25), **sz).cpu().numpy()
            for k in range(m):
                ref = R.flow(inv[k][0], dw, dh, dtype, (1.0, 1.0) if dtype == "i16" else (0.5, 0.25))
                assert np.array_equal(bits(flow[k], dtype), bits(ref, dtype)), (size, k, dw, dh, dtype)
        jobs = [(k, k) for k in range(m)]
        shared = ctx.trace_gather(pool, jobs, count.unsqueeze(1)).cpu().numpy().view(np.uint32)
        mine = ctx.trace_gather(pool, jobs, first.view(torch.int32).squeeze(-1).unsqueeze(1)).cpu().numpy().view(np.uint32)
        own = R.identity(w, h)
        for k in range(m):
            ax, ay = R.clamped(traces[k], w, h)
            assert np.array_equal(shared[k, 0], inv[k][1][ay, ax]) and (shared[k, 0] >= 1).all(), (size, k)
            assert (mine[k, 0] <= own).all() and int((mine[k, 0] == own).sum()) == int((inv[k][1] > 0).sum()), (size, k)
    finally:
        ctx.close()


def test_same_bits_twice(pkg):
    """one call with two jobs on one trace and two destinations: the two destinations are equal"""
    P = pkg
    w, h = 176, 144
    rng = np.random.default_rng(2)
    t = three_hops(P, rng, w, h)[3]
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        pool = ctx.trace_pool(1)
        pool[0] = to_pool(t)
        first, count = ctx.trace_invert(pool, [(0, 2), (0, 0)], *ctx.cover_pools(3))
        assert torch.equal(first[0], first[2]) and torch.equal(count[0], count[2])
        wf, wc = I.invert(t, w, h)
        assert np.array_equal(dwords(first[2]), wf) and np.array_equal(count_dwords(count[0]), wc)
    finally:
        ctx.close()


def test_refusals(pkg):
    P = pkg
    w, h = 130, 98
    ctx = P.Vp8Hip(0)
    L = ctx.L
    try:
        ctx.configure(w, h, 1, 1)
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        size = 4 * w * h
        assert d % 16 == 0 and L.vp8hip_trace_size(ctx.h) == size and 8 * size < 1 << 20
        dp, df, dc, dt = d, d + (1 << 20), d + (2 << 20), d + (3 << 20)          # traces, FIRST, COUNT, tensors
        ptr = lambda p: ctypes.c_void_p(p) if p else None                        # noqa: E731

        def said(rc, who):
            """-2, and the error text names the call"""
            return rc == -2 and who in L.vp8hip_last_error(ctx.h).decode()

        def inv(jobs, n=None, pool=dp, pstride=size, frames=8, first=df, fstride=size, count=dc, cstride=size, out=8):
            arr = (P.InvertJob * max(len(jobs), 1))(*jobs)
            rc = L.vp8hip_trace_invert_async(ctx.h, arr, len(jobs) if n is None else n, ptr(pool), pstride, frames, ptr(first), fstride,
                                             ptr(count), cstride, out)
            assert rc == 0 or said(rc, "vp8hip_trace_invert_async"), L.vp8hip_last_error(ctx.h)
            return rc
        ok = (1, 3)
        assert inv([ok], n=0) == -2 and inv([ok], n=-1) == -2
        for frames in (0, -1):
            assert inv([ok], frames=frames) == -2 and inv([ok], out=frames) == -2
            assert inv([ok], out=frames, first=None) == -2 and inv([ok], out=frames, count=None) == -2
        for bad in (-1, 8, 1 << 20):                                             # a trace, a destination out of range
            assert inv([(bad, 3)]) == -2 and inv([(1, bad)]) == -2 and inv([ok, (bad, 4)]) == -2 and inv([ok, (2, bad)]) == -2, bad
        assert inv([ok, (2, 3)]) == -2 and inv([(0, 5), ok, (0, 5)]) == -2       # two jobs, one destination
        assert inv([ok], first=None, count=None) == -2                           # both outputs null
        assert inv([ok], pool=None) == -2
        # any two of the three byte ranges overlapping: the same memory, one entry shared at either end, one dword shared
        assert inv([ok], first=dc) == -2 and inv([ok], first=dp, count=None) == -2 and inv([ok], count=dp, first=None) == -2
        assert inv([ok], first=dp + 7 * size) == -2 and inv([ok], count=dp - 7 * size + (1 << 20), pool=dp + (1 << 20), first=None) == -2
        assert inv([ok], first=dp + 8 * size - 4, count=None) == -2 and inv([ok], count=df + 8 * size - 4) == -2
        assert inv([ok], pool=df + 4, count=None) == -2 and inv([ok], pool=dc - 8 * size + 4) == -2
        # each of the three pools, as every call refuses a pool (one entry: a job that needs no more)
        job = lambda n: [(n - 1, n - 1)]                                          # noqa: E731
        assert_destinations_refused(ctx, lambda n, dst, stride: inv(job(n), pool=dst, pstride=stride, frames=n), dp, size, 4)
        assert_destinations_refused(ctx, lambda n, dst, stride: inv(job(n), first=dst, fstride=stride, out=n, count=None, frames=3), df, size, 4)
        assert_destinations_refused(ctx, lambda n, dst, stride: inv(job(n), count=dst, cstride=stride, out=n, first=None, frames=3), dc, size, 4)
        assert_destinations_refused(ctx, lambda n, dst, stride: inv(job(n), first=dst, fstride=stride, out=n, frames=3), df, size, 4, null=False)
        assert_destinations_refused(ctx, lambda n, dst, stride: inv(job(n), count=dst, cstride=stride, out=n, frames=3), dc, size, 4, null=False)

        def prm(dw=34, dh=23, dtype=0, planes=3):
            return P.TraceCoverParams(dw, dh, dtype, planes)

        def tens(idx, p, n=None, pool=dc, pstride=size, frames=8, dst=dt, stride=None):
            arr = (ctypes.c_int * len(idx))(*idx)
            fsize = int(L.vp8hip_trace_cover_size(ctx.h, ctypes.byref(p)))
            rc = L.vp8hip_trace_cover_async(ctx.h, arr, len(idx) if n is None else n, ctypes.byref(p), ptr(pool), pstride, frames, ptr(dst),
                                            fsize if stride is None else stride)
            assert rc == 0 or said(rc, "vp8hip_trace_cover_async"), L.vp8hip_last_error(ctx.h)
            return rc
        assert L.vp8hip_trace_cover_size(ctx.h, ctypes.byref(prm())) == 2 * 23 * 34
        assert L.vp8hip_trace_cover_size(ctx.h, ctypes.byref(prm(0, 0, 2, 1))) == h * w * 4
        assert tens([0, 1, 2], prm(), n=0) == -2 and tens([0, 1, 2], prm(), n=-1) == -2
        for bad in (-1, 8, 1 << 20):
            assert tens([0, bad], prm()) == -2, bad
        for frames in (0, -1):
            assert tens([0], prm(), frames=frames) == -2
        for dw, dh in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert tens([0, 1, 2], prm(dw, dh), stride=1 << 19) == -2, (dw, dh)
        for dty in (-1, 3):
            assert tens([0, 1, 2], prm(dtype=dty), stride=1 << 19) == -2
        for planes in (0, 4, 7, 1 << 31):                                         # no plane; bits that are no plane
            assert tens([0, 1, 2], prm(planes=planes), stride=1 << 19) == -2, planes
        for dtype, es in ((0, 1), (1, 2), (2, 4)):          # the destination, each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: tens([0, 1, 2][:n], prm(dtype=dtype), dst=dst, stride=stride), dt,
                                        2 * 23 * 34 * es, es)
        assert_destinations_refused(ctx, lambda n, dst, stride: tens([0, 1, 2][:n], prm(), pool=dst, pstride=stride, frames=n), dc, size, 4)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                                   # nothing was enqueued
        # the same calls into memory the test owns are accepted: the destinations and nothing else are written
        assert inv([ok, (1, 4)]) == 0
        assert inv([(0, 6)], count=None) == 0 and inv([(0, 7)], first=None) == 0
        assert tens([4, 3, 4], prm()) == 0
        ctx.sync()
        a = big.cpu().numpy()
        fill = np.full((h, w), 0x5C5C5C5C, np.uint32)
        wf, wc = I.invert(fill, w, h)
        region = lambda base, k: a[base - d + k * size:base - d + (k + 1) * size].tobytes()      # noqa: E731
        for k in (3, 4, 6):
            assert region(df, k) == wf.tobytes(), k
        for k in (3, 4, 7):
            assert region(dc, k) == wc.tobytes(), k
        untouched = np.ones(a.size, bool)
        for base, ks in ((df, (3, 4, 6)), (dc, (3, 4, 7))):
            for k in ks:
                untouched[base - d + k * size:base - d + (k + 1) * size] = False
        fsize = 2 * 23 * 34
        untouched[dt - d:dt - d + 3 * fsize] = False
        assert (a[untouched] == 0x5C).all()
        assert a[dt - d:dt - d + 3 * fsize].tobytes() == I.tensor(wc, 34, 23).tobytes() * 3
        # the Python wrapper refuses what it can see before the call
        pool = ctx.trace_pool(4)
        first, count = ctx.cover_pools(4)
        with pytest.raises(ValueError):
            ctx.trace_invert(pool, [(0, 0)])                                      # neither output
        with pytest.raises(ValueError):
            ctx.trace_invert(pool, [(0, 0)], count, first)                        # a COUNT pool is no FIRST pool, nor the other way round
        with pytest.raises(ValueError):
            ctx.trace_invert(count, [(0, 0)], first, count)
        with pytest.raises(ValueError):
            ctx.trace_invert(pool, [(0, 0)], first, ctx.cover_pools(3)[1])        # pools of different lengths
        with pytest.raises(ValueError):
            ctx.trace_invert(pool, [(0, 0, 0)], first, count)
        with pytest.raises(ValueError):
            ctx.trace_invert(pool, [(0, 0)], torch.empty((4, h, w + 2, 2), dtype=torch.int16, device="cuda:0")[:, :, :w])
        with pytest.raises(ValueError):
            ctx.trace_cover(pool, [0])                                            # a trace pool is no COUNT pool
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], width=34)
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], dtype=torch.int16)
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], planes=())
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], planes=("count", "nope"))
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], planes=4)
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], dtype=torch.float32, scale=(1.0, 2.0, 3.0))
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0], dtype=torch.float32, scale="pixels")
        with pytest.raises(ValueError):
            ctx.trace_cover(count, [0, 1], 34, 23, out=torch.empty((2, 2, 23, 36), dtype=torch.uint8, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError, match="vp8hip_trace_invert_async"):
            ctx.trace_invert(pool, [(4, 0)], first, count)
        with pytest.raises(RuntimeError, match="vp8hip_trace_invert_async"):
            ctx.trace_invert(pool, [(0, 1), (2, 1)], first, count)
        with pytest.raises(RuntimeError, match="vp8hip_trace_invert_async"):
            ctx.trace_invert(pool, [(0, 1)], pool, count)                         # the trace pool as its own FIRST pool
        with pytest.raises(RuntimeError, match="vp8hip_trace_cover_async"):
            ctx.trace_cover(count, [4])
    finally:
        ctx.close()
