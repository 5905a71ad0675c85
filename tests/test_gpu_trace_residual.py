"""GPU (-m gpu): the accumulated residual in device memory (vp8hip_trace_residual_async; Vp8Hip.trace_residual;
csrc/hip/vp8_trace_residual.hip), bit for bit against the numpy restatement (tests/trace_residual_reference.py) applied to the frames
as they are downloaded or were uploaded and to the traces as the pool holds them: frames in both forms, every type, sizes that are
and are not the display size.  torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path, oracle_decode_ivf
from handover_testlib import TORCH_DTYPE, assert_destinations_refused, assert_guards_intact, bits, equal_on_device, guarded, large_launch
import scale_reference as S
import trace_reference as T
import trace_residual_reference as R
from trace_testlib import dwords, random_trace, to_pool, traced_stream

pytestmark = pytest.mark.gpu

SCALES = [(1.0, 1.0, 1.0), 0.5, (0.125, -3.0, 1.0 / 255), (-1.0 / 3, 1e-3, 2.0)]
DTYPE_NAMES = ("i16", "f32", "f16")
MATRICES = ("bt601", "bt601-full", "bt709")
ORDERS = ("rgb", "bgr")


def sweep_sizes(w, h):
    return ((0, 0), (224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h))


def combo(i, w, h):
    """the i-th of a rotation through sizes, types, matrices, orders and scales"""
    return dict(size=sweep_sizes(w, h)[i % 5], dtype=DTYPE_NAMES[i % 3], matrix=MATRICES[(i // 3) % 3], order=ORDERS[(i // 2) % 2],
                scale=SCALES[(i // 4) % 4])


def scale3(scale):
    return (1.0, 1.0, 1.0) if scale is None else (scale,) * 3 if np.ndim(scale) == 0 else tuple(scale)


def call(ctx, pool, jobs, size=(0, 0), dtype="i16", matrix="bt601", order="rgb", scale=None, out=None):
    kw = {} if size == (0, 0) else dict(width=size[0], height=size[1])
    return ctx.trace_residual(pool, jobs, dtype=TORCH_DTYPE[dtype], matrix=matrix, order=order, scale=scale, out=out, **kw)


def want(cur, anc, t, w, h, size=(0, 0), dtype="i16", matrix="bt601", order="rgb", scale=None):
    return R.residual(cur, anc, t, w, h, size[0], size[1], dtype, matrix, order, scale3(scale))


def packed_frame(buf, g, w, h):
    """the display-size picture in a frame buffer image (numpy) as packed I420"""
    return S.scale_frame(buf, g, w, h, w, h, 0)


def downloaded(ctx, fb):
    return R.pack_i420(*ctx.download_planes(fb))


def random_fb(rng, g):
    """a whole frame buffer of random bytes: borders and what lies past the display size included"""
    return rng.integers(0, 256, g.frame_size, dtype=np.uint8)


def check(ctx, pool, jobs, packed, traces, what=None, out=None, **kw):
    """jobs through trace_residual against the restatement; packed: frame buffer -> packed I420, traces: entry -> numpy trace"""
    got = call(ctx, pool, jobs, out=out, **kw)
    w, h = ctx.width, ctx.height
    uniq = sorted(set(jobs))
    refs = [want(packed[f], packed[a], traces[e], w, h, **kw) for f, e, a in uniq]
    dtype = kw.get("dtype", "i16")
    assert got.shape == (len(jobs),) + refs[0].shape and got.dtype == TORCH_DTYPE[dtype]
    assert equal_on_device(got, refs, [uniq.index(j) for j in jobs], dtype) == [], (what, kw)
    return got


@pytest.mark.parametrize("form", ["tiles", "raster"])
@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98", "p_split_352x288"])
def test_streams_end_to_end(pkg, name, form, monkeypatch):
    """every frame of a stream into a frame buffer of its own, the pool numbered like the frame buffers and traced with the decode
    jobs; then every frame against frame 0's buffer, the parameters in rotation.  Expected values from planes downloaded AFTER the
    calls: a download gives a tiled frame its raster form, which the reader would then take"""
    ctx, pool, _, _, types = traced_stream(pkg, name, form, monkeypatch)
    try:
        w, h, nf = ctx.width, ctx.height, len(types)
        assert types[0] == 0 and sum(types) > 0
        outs = [call(ctx, pool, [(i, i, 0)], **combo(i, w, h)) for i in range(nf)]
        ctx.sync()
        if form == "tiles":
            assert ctx.memory_usage()["raster_pool"] == 0          # read as tiles: no raster form was made
        packed = [downloaded(ctx, i) for i in range(nf)]
        traces = dwords(pool)
        nonzero = 0
        for i in range(nf):
            kw = combo(i, w, h)
            ref = want(packed[i], packed[0], traces[i], w, h, **kw)
            got = outs[i].cpu().numpy()[0]
            assert got.shape == ref.shape and np.array_equal(bits(got, kw["dtype"]), bits(ref, kw["dtype"])), (name, form, i, kw)
            nonzero += bool(ref.any())
        assert not want(packed[0], packed[0], traces[0], w, h).any() and nonzero > nf // 2
    finally:
        ctx.close()


def test_the_four_form_pairs_in_one_call(pkg, monkeypatch):
    """frames a large launch left as tiles beside uploaded (raster-only) frames: tiles/tiles, tiles/raster, raster/tiles and
    raster/raster as (frame, anchor) in one call; at the display size also against frames_rgb's bytes put through torch's gather
    and subtraction"""
    P = pkg
    n = 10
    _, kept = oracle_decode_ivf("kf_640x360", keep_frames=True)
    ctx = P.Vp8Hip(0)
    try:
        large_launch(P, ctx, "kf_640x360", n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0
        g, w, h = ctx.g, ctx.width, ctx.height
        rng = np.random.default_rng(31)
        rnd = [random_fb(rng, g) for _ in range(2)]
        for k in range(2):
            ctx.upload_frame(n + k, rnd[k])                # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        packed = {n: packed_frame(rnd[0], g, w, h), n + 1: packed_frame(rnd[1], g, w, h)}
        for fb in (0, 4, 9):
            packed[fb] = packed_frame(kept[fb][4], g, w, h)
        traces = [random_trace(rng, w, h) for _ in range(3)]
        pool = ctx.trace_pool(3)
        for k in range(3):
            pool[k] = to_pool(traces[k])
        jobs = [(4, 0, 0), (4, 1, n), (n, 2, 9), (n + 1, 0, n), (9, 1, 9), (n, 1, n + 1)]
        for kw in (dict(), dict(size=(224, 224), dtype="f32", matrix="bt709", order="bgr", scale=(1 / 255, 0.5, -2.0)),
                   dict(size=(w + 1, h - 1), dtype="f16", matrix="bt601-full", scale=0.25)):
            got = check(ctx, pool, jobs, packed, traces, **kw)
        got = call(ctx, pool, jobs)
        rgb = ctx.frames_rgb([f for j in jobs for f in (j[0], j[2])]).to(torch.int32)          # [2n, 3, h, w], read in the same forms
        for k, (f, e, a) in enumerate(jobs):
            tx, ty = T.unpack(traces[e])
            flat = torch.from_numpy((ty.astype(np.int64) * w + tx.astype(np.int64)).ravel()).to("cuda:0")
            snippet = rgb[2 * k] - rgb[2 * k + 1].flatten(1)[:, flat].view(3, h, w)
            assert torch.equal(got[k].to(torch.int32), snippet), k
        assert ctx.memory_usage()["tile_pool"] > 0 and ctx.rgb_scratch_bytes() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45), (130, 98)])
def test_small_and_odd_shapes_into_guarded_destinations(pkg, size):
    """uploaded random frames and random traces; destinations at offsets 2, 4 and 16 of their allocation with strides that are and are
    not multiples of 16, every type, output widths that are and are not multiples of 4: the tensors and the bytes around them
    (the kernel sizes nothing by the frame width and stages no rows: no wide frame here)"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 37 + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 3, 1)
        g = ctx.g
        bufs = [random_fb(rng, g) for _ in range(2)]
        for k in range(2):
            ctx.upload_frame(k, bufs[k])
        packed = {k: packed_frame(bufs[k], g, w, h) for k in range(2)}
        traces = [random_trace(rng, w, h) for _ in range(2)]
        pool = ctx.trace_pool(2)
        for k in range(2):
            pool[k] = to_pool(traces[k])
        jobs = [(0, 0, 1), (1, 1, 0), (1, 0, 1)]
        sizes = ((0, 0), (24, 10), (13, 7), (w + 3, h + 1), (4 * ((w + 3) // 4), 3))
        for i, ((off, pad), dtype, out_size) in enumerate(itertools.product(((2, 4), (4, 12), (16, 0), (16, 16), (16, 8)), DTYPE_NAMES, sizes)):
            gw, gh = (w, h) if out_size == (0, 0) else out_size
            es = 4 if dtype == "f32" else 2
            fsize = 3 * gh * gw * es
            foff, fpad = off // es * es, pad // es * es
            big, flat = guarded(len(jobs), fsize, fpad, foff, 0x3C)
            out = flat.view(TORCH_DTYPE[dtype]).unflatten(1, (3, gh, gw))
            assert out.data_ptr() % 16 == foff % 16 and out.stride(0) * es == fsize + fpad
            kw = dict(size=out_size, dtype=dtype, matrix=MATRICES[i % 3], order=ORDERS[i % 2], scale=SCALES[i % 4])
            check(ctx, pool, jobs, packed, traces, what=(size, off, pad), out=out, **kw)
            assert_guards_intact(big, len(jobs), fsize, fpad, foff, 0x3C, what=(size, off, pad, dtype, out_size))
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(67, 45), (130, 98)])
def test_the_clamp_on_the_device(pkg, size):
    """trace values up to 8 pixels outside the picture on every side, in jobs whose anchor is a raster-form frame buffer that is not
    the context's last: a kernel that forgot the clamp reads a byte of the frame's own 32-pixel border, which is random here, and
    fails the comparison"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 3, 1)
        g = ctx.g
        bufs = [random_fb(rng, g) for _ in range(2)]
        for k in range(2):
            ctx.upload_frame(k, bufs[k])
        packed = {k: packed_frame(bufs[k], g, w, h) for k in range(2)}
        tx, ty = rng.integers(-8, w + 8, (h, w)), rng.integers(-8, h + 8, (h, w))
        run = rng.random((h, w)) < 0.5                       # half of them as rows of neighbours that run over the edges
        ys, xs = np.mgrid[0:h, 0:w]
        tx[run] = (xs + rng.integers(-8, 9, (h, 1)))[run]
        ty[run] = (ys + rng.integers(-8, 9, (h, 1)))[run]
        t = T.pack(tx, ty)
        outside = (tx < 0) | (tx >= w) | (ty < 0) | (ty >= h)
        assert outside.sum() > h * w // 10 and tx.min() == -8 and ty.min() == -8 and tx.max() == w + 7 and ty.max() == h + 7
        pool = ctx.trace_pool(1)
        pool[0] = to_pool(t)
        for kw in (dict(), dict(size=(w + 5, h + 2), dtype="f32", scale=0.5), dict(size=(40, 24), dtype="f16", matrix="bt709")):
            check(ctx, pool, [(1, 0, 0), (0, 0, 1), (0, 0, 0)], packed, [t], what=size, **kw)
    finally:
        ctx.close()


def test_float_types_on_every_difference(pkg):
    """grey chroma, the full-range matrix and two luma ramps: the luma of both pictures is the column, and the trace of pixel (y, x)
    names column 255 - y (in row x), so every channel is x + y - 255: every value in -255 .. 255.  Against scales that make the float land on ties of
    the halves (the half is the FLOAT rounded: two roundings), powers of two, negative ones and denormals"""
    P = pkg
    w = h = 256
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 3, 1)
        g = ctx.g
        ys, xs = np.mgrid[0:h, 0:w]
        bufs = []
        for _ in range(2):
            buf = np.full(g.frame_size, 128, np.uint8)
            S.planes(buf, g)[0][:] = xs
            bufs.append(buf)
            ctx.upload_frame(len(bufs) - 1, buf)
        packed = {k: packed_frame(bufs[k], g, w, h) for k in range(2)}
        t = T.pack(255 - ys, xs)
        pool = ctx.trace_pool(1)
        pool[0] = to_pool(t)
        a = xs + ys - 255
        i16 = want(packed[0], packed[1], t, w, h, matrix="bt601-full")
        assert all(np.array_equal(i16[c], a) for c in range(3)) and set(np.unique(a).tolist()) == set(range(-255, 256))
        check(ctx, pool, [(0, 0, 1)], packed, [t], matrix="bt601-full")
        differ = 0
        for scale in ((1.8145380020141602, 0.2483258992433548, 1.2147321701049805), (1.0, 0.125, -1.0 / 3), (1e-3, 1e-42, -3e-41),
                      (2.0 ** -24, 65504.0 / 255, 3.0e4), (1e30, 1.0 / 255, 1.0 / (255 * 0.229))):
            scale = tuple(float(np.float32(s)) for s in scale)
            for dtype in ("f32", "f16"):
                check(ctx, pool, [(0, 0, 1)], packed, [t], what=scale, dtype=dtype, matrix="bt601-full", order="bgr", scale=scale)
            with np.errstate(over="ignore"):
                once = (a.astype(np.float64) * np.float64(np.float32(scale[0]))).astype(np.float16)
            differ += int((once != want(packed[0], packed[1], t, w, h, dtype="f16", matrix="bt601-full", scale=scale)[0]).sum())
        assert differ > 0                               # (the sweep holds values one rounding would get wrong)
    finally:
        ctx.close()


def test_batch_of_300_jobs(pkg):
    """300 jobs in one call -- two launches' worth of 128 and a remainder --, repeats and permutations of eight frame buffers and
    eight pool entries"""
    P = pkg
    w, h, nfb, n = 176, 144, 8, 300
    rng = np.random.default_rng(300)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, nfb + 1, 1)
        g = ctx.g
        packed = {}
        for k in range(nfb):
            buf = random_fb(rng, g)
            ctx.upload_frame(k, buf)
            packed[k] = packed_frame(buf, g, w, h)
        traces = [random_trace(rng, w, h) for _ in range(nfb)]
        pool = ctx.trace_pool(nfb)
        for k in range(nfb):
            pool[k] = to_pool(traces[k])
        some = [tuple(int(v) for v in rng.integers(0, nfb, 3)) for _ in range(40)]
        jobs = [some[int(i)] for i in rng.integers(0, len(some), n)]
        assert len(set(jobs)) > 30
        check(ctx, pool, jobs, packed, traces, size=(45, 37), dtype="f16", matrix="bt709", order="bgr", scale=(0.5, 0.25, -1.0))
        check(ctx, pool, jobs, packed, traces)
    finally:
        ctx.close()


def test_refusals(pkg):
    P = pkg
    w, h = 130, 98
    rng = np.random.default_rng(98)
    ctx = P.Vp8Hip(0)
    L = ctx.L
    try:
        ctx.configure(w, h, 3, 1)
        g = ctx.g
        bufs = [random_fb(rng, g) for _ in range(2)]
        for k in range(2):
            ctx.upload_frame(k, bufs[k])
        packed = {k: packed_frame(bufs[k], g, w, h) for k in range(2)}
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        d2 = d + (1 << 21)
        assert d % 16 == 0
        size = 4 * w * h
        assert 8 * size < 1 << 21

        def prm(dw=34, dh=23, dtype=0, matrix=0, order=0):
            return P.TraceResidualParams(dw, dh, matrix, order, dtype)

        def run(jobs, p, n=None, pool=d, pstride=size, frames=8, dst=d2, stride=None):
            arr = (P.AnchorJob * len(jobs))(*jobs)
            fsize = int(L.vp8hip_trace_residual_size(ctx.h, ctypes.byref(p)))
            return L.vp8hip_trace_residual_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(p), ctypes.c_void_p(pool) if pool else None,
                                                 pstride, frames, ctypes.c_void_p(dst) if dst else None, fsize if stride is None else stride)
        ok = [(0, 0, 1), (1, 1, 0), (0, 2, 0)]
        assert L.vp8hip_trace_residual_size(ctx.h, ctypes.byref(prm())) == 3 * 23 * 34 * 2
        assert L.vp8hip_trace_residual_size(ctx.h, ctypes.byref(prm(0, 0, 2))) == 3 * h * w * 4
        assert run(ok, prm(), n=0) == -2 and run(ok, prm(), n=-1) == -2
        for bad in (-1, 3, 1 << 20):                       # a frame buffer out of range: the frame's, the anchor's
            assert run([(0, 0, 1), (bad, 0, 1)], prm()) == -2, bad
            assert run([(0, 0, 1), (0, 0, bad)], prm()) == -2, bad
        for frames in (0, -1):
            assert run(ok, prm(), frames=frames) == -2
        for bad in (-1, 8, 1 << 20):                       # a trace outside the pool
            assert run([(0, 0, 1), (0, bad, 1)], prm()) == -2, bad
        assert run(ok, prm(), frames=2) == -2
        for dw, dh in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert run(ok, prm(dw, dh), stride=1 << 19) == -2, (dw, dh)
        for bad in (-1, 3):
            assert run(ok, prm(dtype=bad), stride=1 << 19) == -2
            assert run(ok, prm(matrix=bad), stride=1 << 19) == -2
        for bad in (-1, 2):
            assert run(ok, prm(order=bad), stride=1 << 19) == -2
        for dtype, es in ((0, 2), (1, 2), (2, 4)):          # the destination, each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: run(ok[:n], prm(dtype=dtype), dst=dst, stride=stride), d2, 3 * 23 * 34 * es, es)
        assert_destinations_refused(ctx, lambda n, dst, stride: run(ok[:n], prm(), pool=dst, pstride=stride, frames=n), d, size, 4)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()            # nothing was enqueued
        # the same call into memory the test owns is accepted: the destinations and nothing else are written
        assert run(ok, prm()) == 0
        ctx.sync()
        a = big.cpu().numpy()
        fill = np.full((h, w), 0x5C5C5C5C, np.uint32)       # (an entry nobody wrote: clamped, garbage, in bounds)
        fsize = 3 * 23 * 34 * 2
        for k, (f, e, an) in enumerate(ok):
            ref = R.residual(packed[f], packed[an], fill, w, h, 34, 23)
            assert a[(1 << 21) + k * fsize:(1 << 21) + (k + 1) * fsize].tobytes() == ref.tobytes(), k
        assert (a[:1 << 21] == 0x5C).all() and (a[(1 << 21) + 3 * fsize:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        pool = ctx.trace_pool(4)
        pool.zero_()
        with pytest.raises(ValueError):
            ctx.trace_residual(pool.view(torch.float16), [(0, 0, 1)])
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], width=34)
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], dtype=torch.int8)
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], matrix="nope")
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], order="grb")
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], scale="pixels")
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], scale=(1.0, 2.0))
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0)])
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1)], 16384, 2)
        with pytest.raises(ValueError):
            ctx.trace_residual(pool, [(0, 0, 1), (1, 1, 0)], 34, 23, out=torch.empty((2, 3, 23, 36), dtype=torch.int16, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError):
            ctx.trace_residual(pool, [(3, 0, 1)])
        with pytest.raises(RuntimeError):
            ctx.trace_residual(pool, [(0, 4, 1)])
        assert ctx.trace_residual(pool, [(0, 0, 1)], 34, 23).shape == (1, 3, 23, 34)
    finally:
        ctx.close()


def test_ordering_against_a_later_decode(pkg):
    """the call, then at once the decode of another frame into the frame buffer it reads, then the tensor read on torch's stream: it
    holds the frame that was there at the call"""
    P = pkg
    w, h, frames = P.read_ivf(ivf_path("kf_640x360"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 3, 3)
        for i in range(3):
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, frames[i], i)
            assert hdr.frame_type == 0
            parser.swap(hdr)
        ctx.decode([(0, 0, None), (1, 1, None)], P.STAGE_ALL)
        ctx.sync()
        rng = np.random.default_rng(5)
        t = random_trace(rng, w, h)
        pool = ctx.trace_pool(1)
        pool[0] = to_pool(t)
        old = {k: downloaded(ctx, k) for k in range(2)}
        jobs = [(1, 0, 0)] * 24
        got = call(ctx, pool, jobs, dtype="f32", scale=0.5)
        ctx.decode([(2, 1, None)], P.STAGE_ALL)              # no wait in between
        res = got.cpu().numpy()                              # .cpu() on torch's current stream
        ref = want(old[1], old[0], t, w, h, dtype="f32", scale=0.5)
        for k in range(len(jobs)):
            assert np.array_equal(bits(res[k], "f32"), bits(ref, "f32")), k
        ctx.sync()
        # ... and the frame buffer now holds the later frame
        new = downloaded(ctx, 1)
        assert not np.array_equal(new, old[1])
        check(ctx, pool, [(1, 0, 0)], {0: old[0], 1: new}, [t])
    finally:
        parser.close()
        ctx.close()


@pytest.mark.parametrize("form", ["tiles", "raster"])
def test_nothing_else_is_touched(pkg, form, monkeypatch):
    """no device memory is added, and the frame buffers and the pool are bit-identical before and after"""
    P = pkg
    monkeypatch.setenv("VP8HIP_RECON", "simt" if form == "tiles" else "wave")
    w, h, frames = P.read_ivf(ivf_path("p_odd_130x98"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 4, 1)
        pool = ctx.trace_pool(4)
        pool.zero_()
        jobs = []
        for data in frames[:2]:
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            jobs.append((0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx)))
            ctx.decode(jobs[-1:], P.STAGE_ALL)
            ctx.frames_trace(jobs[-1:], pool)
            parser.swap(hdr)
        anchor, fb = jobs[0][1], jobs[1][1]
        assert hdr.frame_type == 1 and anchor != fb
        ctx.sync()
        rgb_before = ctx.frames_rgb([anchor, fb])           # (read in the form the frames have: nothing is converted)
        before = ctx.memory_usage()
        pool_before = pool.clone()
        outs = [call(ctx, pool, [(fb, fb, anchor), (anchor, anchor, anchor)], **kw)
                for kw in (dict(), dict(size=(224, 224), dtype="f32", scale=1 / 255), dict(size=(31, 17), dtype="f16"))]
        ctx.sync()
        assert ctx.memory_usage() == before
        if form == "tiles":
            assert before["raster_pool"] == 0
        assert ctx.rgb_scratch_bytes() == 0
        assert torch.equal(ctx.frames_rgb([anchor, fb]), rgb_before)
        assert torch.equal(pool, pool_before)
        full_before = [ctx.download_full(k) for k in (anchor, fb)]
        packed = {anchor: downloaded(ctx, anchor), fb: downloaded(ctx, fb)}
        traces = dwords(pool)
        assert np.array_equal(traces[anchor], T.identity(w, h)) and (traces[fb] != traces[anchor]).any()
        for got, kw in zip(outs, (dict(), dict(size=(224, 224), dtype="f32", scale=1 / 255), dict(size=(31, 17), dtype="f16"))):
            for k, (f, a) in enumerate(((fb, anchor), (anchor, anchor))):
                ref = want(packed[f], packed[a], traces[f], w, h, **kw)
                assert np.array_equal(bits(got[k].cpu().numpy(), kw.get("dtype", "i16")), bits(ref, kw.get("dtype", "i16"))), (kw, k)
        # the raster form the downloads made is left alone too
        call(ctx, pool, [(fb, fb, anchor)])
        ctx.sync()
        assert all(np.array_equal(ctx.download_full(k), b) for k, b in zip((anchor, fb), full_before))
    finally:
        parser.close()
        ctx.close()


def test_one_1080p_frame(pkg):
    """several workgroups a frame: the display size as halves, 224x224 as floats"""
    P = pkg
    w, h, frames = P.read_ivf(ivf_path("p_1920x1080"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 4, 1)
        pool = ctx.trace_pool(4)
        pool.zero_()
        for data in frames[:2]:
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            job = (0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))
            if hdr.frame_type == 0:
                anchor = r.new_idx
            ctx.decode([job], P.STAGE_ALL)
            ctx.frames_trace([job], pool)
            parser.swap(hdr)
        fb = job[1]
        assert hdr.frame_type == 1 and fb != anchor
        packed = {anchor: downloaded(ctx, anchor), fb: downloaded(ctx, fb)}
        traces = dwords(pool)
        assert (traces[fb] != T.identity(w, h)).any()
        check(ctx, pool, [(fb, fb, anchor)], packed, traces, dtype="f16", scale=(1 / 255, 1 / 255, 1 / 255))
        check(ctx, pool, [(fb, fb, anchor)], packed, traces, size=(224, 224), dtype="f32", matrix="bt709", scale=0.5)
    finally:
        parser.close()
        ctx.close()
