"""GPU (-m gpu): the gather along the trace in device memory (vp8hip_trace_gather_async; Vp8Hip.trace_gather;
csrc/hip/vp8_trace_gather.hip) against the numpy restatement (tests/trace_gather_reference.py) applied to the source tensors as they
were uploaded and to the traces as trace_reference makes them or as the pool holds them: NEAREST bit for bit, BILINEAR within the
bound include/vp8hip.h derives; both layouts, every element size, source and output grids that are and are not the display size.
torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path
from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded
import trace_reference as T
import trace_gather_reference as G
from trace_testlib import dwords, random_trace, to_pool, traced_stream

pytestmark = pytest.mark.gpu

LAYOUTS = ("planar", "channels_last")
FIXTURES = ("p_arf_176x144", "p_odd_130x98", "p_split_352x288")
NP_OF = {"u8": np.uint8, "i16": np.int16, "f16": np.float16, "f32": np.float32, "i32": np.int32}


def random_src(rng, m, C, sh, sw, dtype):
    """seeded values [m, C, sh, sw]: floats finite with |v| <= 1000, integers over their type"""
    dt = NP_OF[dtype]
    if dtype in ("f16", "f32"):
        return rng.uniform(-1000.0, 1000.0, (m, C, sh, sw)).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, (m, C, sh, sw), dtype=np.int64).astype(dt)


def on_device(a, layout, off=0):
    """numpy [m, C, h, w] -> a device tensor of that shape in `layout`, its first element `off` elements into its allocation"""
    m, C, h, w = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a if layout == "planar" else a.transpose(0, 2, 3, 1)))
    flat = torch.zeros(a.size + off, dtype=t.dtype, device="cuda:0")
    flat[off:] = t.flatten().to("cuda:0")
    v = flat[off:]
    return v.view(m, C, h, w) if layout == "planar" else v.view(m, h, w, C).permute(0, 3, 1, 2)


def out_view(flat, dtype, layout, C, gh, gw):
    """guarded()'s uint8 frames [n, bytes] as the tensor [n, C, gh, gw] in `layout`"""
    v = flat.view(getattr(torch, np.dtype(NP_OF[dtype]).name))
    return v.unflatten(1, (C, gh, gw)) if layout == "planar" else v.unflatten(1, (gh, gw, C)).permute(0, 3, 1, 2)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check(ctx, pool, jobs, src_t, src_np, traces, size=(0, 0), filt="nearest", out=None, what=None):
    """jobs through trace_gather against the restatement; src_np: what src_t holds; traces: entry -> numpy trace"""
    kw = {} if size == (0, 0) else dict(width=size[0], height=size[1])
    got_t = ctx.trace_gather(pool, jobs, src_t, filter=filt, out=out, **kw)
    got = got_t.cpu().numpy()
    w, h = ctx.width, ctx.height
    gw, gh = (w, h) if size == (0, 0) else size
    assert got.shape == (len(jobs), src_np.shape[1], gh, gw) and got.dtype == src_np.dtype, what
    assert got_t.dtype == src_t.dtype and got_t.device == src_t.device
    seen = {}
    for k, (e, s) in enumerate(jobs):
        if (e, s) not in seen:
            seen[(e, s)] = G.nearest(src_np[s], traces[e], w, h, *size) if filt == "nearest" else G.bilinear(src_np[s], traces[e], w, h, *size)
        ref = seen[(e, s)]
        if filt == "nearest":
            assert np.array_equal(as_bytes(got[k]), as_bytes(ref)), (what, k, size, filt)
        else:
            excess = G.bilinear_excess(got[k], *ref)
            assert np.isfinite(got[k]).all() and excess <= 0.0, (what, k, size, filt, excess)
    return got_t


@pytest.mark.parametrize("form", ["tiles", "raster"])
@pytest.mark.parametrize("name", FIXTURES)
def test_streams_end_to_end(pkg, name, form, monkeypatch):
    """the shown frames of a stream in one call each: an int16 source of the display size and a float16 one of an eighth of it, both
    layouts, both filters where allowed, against the restatement on trace_reference's traces; and the anchor's RGB bytes gathered at
    the display size against frames_rgb minus trace_residual"""
    ctx, pool, mine, shown, types = traced_stream(pkg, name, form, monkeypatch)
    try:
        w, h = ctx.width, ctx.height
        assert types[0] == 0 and sum(types) > 0 and len(shown) > 2
        assert np.array_equal(dwords(pool)[:len(types)], np.stack(mine[:len(types)]))
        rng = np.random.default_rng(len(name) + w)
        jobs = [(i, k % 2) for k, i in enumerate(shown)]
        labels = random_src(rng, 2, 5, h, w, "i16")
        sw8, sh8 = -(-w // 8), -(-h // 8)
        feats = random_src(rng, 2, 16, sh8, sw8, "f16")
        for layout in LAYOUTS:
            check(ctx, pool, jobs, on_device(labels, layout), labels, mine, what=(name, form, layout))
            ft = on_device(feats, layout)
            for filt in ("nearest", "bilinear"):
                check(ctx, pool, jobs, ft, feats, mine, size=(sw8, sh8), filt=filt, what=(name, form, layout))
                check(ctx, pool, jobs[:3], ft, feats, mine, filt=filt, what=(name, form, layout))
        # against the calls that exist: rgb(anchor) at the trace == rgb(frame) - accumulated residual
        anchor = ctx.frames_rgb([0])
        moved = ctx.trace_gather(pool, [(i, 0) for i in shown], anchor)
        want = ctx.frames_rgb(shown).to(torch.int16) - ctx.trace_residual(pool, [(i, i, 0) for i in shown])
        assert moved.dtype == torch.uint8 and torch.equal(moved.to(torch.int16), want)
        assert not torch.equal(moved, anchor.expand(len(shown), -1, -1, -1))
    finally:
        ctx.close()


ELEMS = (1, 2, 4)
CHANNELS = (1, 3, 5, 16, 21)
OFFSETS = ((1, 0), (3, 1), (16, 0), (16, 16), (32, 8), (5, 3))          # (the first element's offset, the padding between outputs), in elements


def src_grids(w, h):
    return ((1, 1), (7, 5), (w, h), (-(-w // 8), -(-h // 8)), (2 * w + 1, 2 * h + 1))


OUT_GRIDS = ((0, 0), (1, 1), (224, 224), (45, 67))


def shape_cases(w, h, count=36):
    """a rotation that shows every value of every axis, then a seeded sample of the whole product"""
    axes = (ELEMS, LAYOUTS, CHANNELS, src_grids(w, h), OUT_GRIDS)
    cases = [tuple(ax[i % len(ax)] for ax in axes) for i in range(5)]
    every = list(itertools.product(*axes))
    rng = np.random.default_rng(w * 1000 + h)
    cases += [every[int(i)] for i in rng.permutation(len(every))[:count]]
    return axes, cases


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45), (130, 98)])
def test_small_and_odd_shapes_into_guarded_destinations(pkg, size):
    """random traces; every element size, both layouts, channel counts that do and do not make whole 16-byte rows, source and
    output grids from one cell to twice the display; destinations that start on an odd element or on 16 bytes, with and without
    padding between outputs; sources on and off 16 bytes: the tensors and the bytes around them"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 37 + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        traces = [random_trace(rng, w, h) for _ in range(2)]
        pool = ctx.trace_pool(2)
        for k in range(2):
            pool[k] = to_pool(traces[k])
        jobs = [(0, 1), (1, 0), (1, 1)]
        axes, cases = shape_cases(w, h)
        for ax, col in zip(axes, zip(*cases)):
            assert set(col) == set(ax)                       # every value of every axis is there
        bilinear = 0
        for i, (es, layout, C, (sw, sh), out_size) in enumerate(cases):
            gw, gh = (w, h) if out_size == (0, 0) else out_size
            off_el, pad_el = OFFSETS[i % len(OFFSETS)]
            foff, fpad = off_el * es, pad_el * es
            fsize = C * gh * gw * es
            for dtype, filt in {1: (("u8", "nearest"),), 2: (("i16", "nearest"), ("f16", "bilinear")), 4: (("f32", "nearest"), ("f32", "bilinear"))}[es]:
                src = random_src(rng, 2, C, sh, sw, dtype)
                src_t = on_device(src, layout, off=i % 3)
                big, flat = guarded(len(jobs), fsize, fpad, foff, 0x3C)
                out = out_view(flat, dtype, layout, C, gh, gw)
                assert out.data_ptr() % 16 == foff % 16 and out.stride(0) * es == fsize + fpad
                what = (size, es, layout, C, (sw, sh), out_size, off_el, pad_el, dtype, filt)
                check(ctx, pool, jobs, src_t, src, traces, size=out_size, filt=filt, out=out, what=what)
                assert_guards_intact(big, len(jobs), fsize, fpad, foff, 0x3C, what=what)
                bilinear += filt == "bilinear"
        assert bilinear > 10
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(67, 45), (130, 98)])
def test_the_clamp_on_the_device(pkg, size):
    """pool entries of random int16 over the whole range -- ordinary input: the call clamps it --; the source tensors lie between two
    guard tensors of a value no source holds, which a read outside the job's tensor would bring into the output"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        t = T.pack(rng.integers(-32768, 32768, (h, w)), rng.integers(-32768, 32768, (h, w)))
        tx, ty = T.unpack(t)
        assert ((tx < 0) | (tx >= w) | (ty < 0) | (ty >= h)).mean() > 0.9 and ((tx >= 0) & (tx < w)).any()
        pool = ctx.trace_pool(1)
        pool[0] = to_pool(t)
        axes = (((w, h), (-(-w // 8), -(-h // 8)), (2 * w + 1, 2 * h + 1), (1, 1)), LAYOUTS,
                (("i16", "nearest"), ("f16", "bilinear"), ("f32", "bilinear"), ("u8", "nearest")), ((0, 0), (45, 67)))
        picks = [ix for ix in itertools.product(*(range(len(a)) for a in axes)) if sum(ix) % 2 == 0]       # half of the product
        assert all(set(col) == set(range(len(a))) for a, col in zip(axes, zip(*picks)))
        for i, ix in enumerate(picks):
            (sw, sh), layout, (dtype, filt), out_size = (a[k] for a, k in zip(axes, ix))
            C = (5, 8, 16)[i % 3]
            src = random_src(rng, 4, C, sh, sw, dtype)
            if dtype in ("u8", "i16"):
                src[src == 77] = 78
            mark = 77 if dtype in ("u8", "i16") else 2048.0       # (no source value, and above every blend of source values)
            src[0] = src[3] = mark
            src_t = on_device(src, layout)
            got = check(ctx, pool, [(0, 1), (0, 0), (0, 1)], src_t[1:3], src[1:3], [t], size=out_size, filt=filt, what=(size, sw, sh, layout, dtype))
            assert not (got == mark).any()
    finally:
        ctx.close()


def test_bilinear_properties(pkg):
    """a source grid of the display's size: every weight is zero and BILINEAR is NEAREST bit for bit; a constant source comes out
    within the bound at every grid"""
    P = pkg
    w, h = 130, 98
    rng = np.random.default_rng(1309)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        traces = [random_trace(rng, w, h), T.pack(rng.integers(-40, w + 40, (h, w)), rng.integers(-40, h + 40, (h, w)))]
        pool = ctx.trace_pool(2)
        for k in range(2):
            pool[k] = to_pool(traces[k])
        jobs = [(0, 0), (1, 1), (1, 0)]
        for dtype, layout in itertools.product(("f16", "f32"), LAYOUTS):
            C = 8 if layout == "planar" else 5
            src = random_src(rng, 2, C, h, w, dtype)
            src[0, 0, 0, :7] = (-0.0, 0.0, 1000.0, -1000.0, 6e-8, -6e-8, 1.0)       # signed zeros and (halves) a subnormal survive
            src_t = on_device(src, layout)
            for out_size in ((0, 0), (45, 67)):
                kw = {} if out_size == (0, 0) else dict(width=out_size[0], height=out_size[1])
                near = ctx.trace_gather(pool, jobs, src_t, **kw)
                lin = check(ctx, pool, jobs, src_t, src, traces, size=out_size, filt="bilinear", what=(dtype, layout))
                view = torch.int16 if dtype == "f16" else torch.int32
                assert torch.equal(near.contiguous().view(view), lin.contiguous().view(view)), (dtype, layout, out_size)
            for value in (1000.0, -0.333251953125, 3.0):
                for sw, sh in ((7, 5), (17, 13), (261, 197)):
                    const = np.full((1, C, sh, sw), value, NP_OF[dtype])
                    got = check(ctx, pool, [(0, 0), (1, 0)], on_device(const, layout), const, traces, filt="bilinear", what=(dtype, layout, value))
                    lim = 8 * 2.0 ** -24 * abs(value) + (2.0 ** -11 * abs(value) + 2.0 ** -25 if dtype == "f16" else 0.0)
                    assert float((got.double() - float(const[0, 0, 0, 0])).abs().max()) <= lim
    finally:
        ctx.close()


def test_batch_of_300_jobs(pkg):
    """300 jobs in one call -- a launch's worth of 256 and a remainder --, repeats and permutations of eight pool entries and six
    source tensors"""
    P = pkg
    w, h, n = 16, 16, 300
    rng = np.random.default_rng(300)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        traces = [random_trace(rng, w, h) for _ in range(8)]
        pool = ctx.trace_pool(8)
        for k in range(8):
            pool[k] = to_pool(traces[k])
        some = [(int(rng.integers(0, 8)), int(rng.integers(0, 6))) for _ in range(40)]
        jobs = [some[int(i)] for i in rng.integers(0, len(some), n)]
        assert len(set(jobs)) > 25 and jobs != sorted(jobs)
        for layout in LAYOUTS:
            src = random_src(rng, 6, 3, 9, 11, "i16")
            check(ctx, pool, jobs, on_device(src, layout), src, traces, size=(45, 37), what=layout)
            src = random_src(rng, 6, 8, 16, 16, "f16")
            check(ctx, pool, jobs, on_device(src, layout), src, traces, filt="bilinear", what=layout)
            src = random_src(rng, 6, 8, 5, 3, "f32")
            check(ctx, pool, jobs, on_device(src, layout), src, traces, filt="bilinear", what=layout)
    finally:
        ctx.close()


def test_refusals(pkg):
    P = pkg
    w, h = 130, 98
    rng = np.random.default_rng(98)
    who = "vp8hip_trace_gather_async"
    ctx = P.Vp8Hip(0)
    L = ctx.L
    try:
        ctx.configure(w, h, 1, 1)
        big = torch.full((3 << 21,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()                                  # the pool
        s = d + (1 << 21)                                   # the sources
        d2 = d + (2 << 21)                                  # the destinations
        assert d % 16 == 0
        tsize = 4 * w * h
        assert 8 * tsize < 1 << 21
        C, sw, sh, gw, gh = 5, 17, 13, 34, 23

        def prm(dw=gw, dh=gh, srw=sw, srh=sh, ch=C, elem=2, layout=0, filt=0):
            return P.TraceGatherParams(dw, dh, srw, srh, ch, elem, layout, filt)

        def run(jobs, p, n=None, pool=d, pstride=tsize, frames=8, src=s, sstride=None, sframes=3, dst=d2, stride=None):
            arr = (P.GatherJob * len(jobs))(*jobs)
            ssize = p.channels * p.src_h * p.src_w * p.elem
            fsize = int(L.vp8hip_trace_gather_size(ctx.h, ctypes.byref(p)))
            void = ctypes.c_void_p
            rc = L.vp8hip_trace_gather_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(p), void(pool) if pool else None, pstride, frames,
                                             void(src) if src else None, ssize if sstride is None else sstride, sframes,
                                             void(dst) if dst else None, fsize if stride is None else stride)
            if rc:
                assert L.vp8hip_last_error(ctx.h).decode().startswith(who), L.vp8hip_last_error(ctx.h)
            return rc
        ok = [(0, 1), (1, 0), (2, 2)]
        assert L.vp8hip_trace_gather_size(ctx.h, ctypes.byref(prm())) == C * gh * gw * 2
        assert L.vp8hip_trace_gather_size(ctx.h, ctypes.byref(prm(0, 0, elem=4))) == C * h * w * 4
        assert run(ok, prm(), n=0) == -2 and run(ok, prm(), n=-1) == -2
        for frames in (0, -1):
            assert run(ok, prm(), frames=frames) == -2
        for bad in (-1, 8, 1 << 20):                        # a trace outside the pool
            assert run([(0, 0), (bad, 0)], prm()) == -2, bad
        assert run(ok, prm(), frames=2) == -2
        for bad in (-1, 3, 1 << 20):                        # a source tensor that is not there
            assert run([(0, 0), (0, bad)], prm()) == -2, bad
        assert run(ok, prm(), sframes=2) == -2
        for sframes in (0, -1):
            assert run([(0, 0)], prm(), sframes=sframes) == -2
        for dw, dh in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert run(ok, prm(dw, dh), stride=1 << 19) == -2, (dw, dh)
        for srw, srh in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-3, 5), (0, 0)):
            assert run(ok, prm(srw=srw, srh=srh), sstride=1 << 19, stride=1 << 19) == -2, (srw, srh)
        for ch in (0, -1, 4097):
            assert run(ok, prm(ch=ch), sstride=1 << 19, stride=1 << 19) == -2
        for elem in (0, 3, 8, -1):
            assert run(ok, prm(elem=elem), sstride=1 << 19, stride=1 << 19) == -2
        for bad in (-1, 2):
            assert run(ok, prm(layout=bad), stride=1 << 19) == -2
            assert run(ok, prm(filt=bad), stride=1 << 19) == -2
        assert run(ok, prm(elem=1, filt=1), sstride=1 << 19, stride=1 << 19) == -2         # BILINEAR on bytes
        for elem in (1, 2, 4):                              # the destination and the source, each element size: also the alignment to it
            for layout in (0, 1):
                p = prm(elem=elem, layout=layout)
                assert_destinations_refused(ctx, lambda n, dst, stride: run(ok[:n], p, dst=dst, stride=stride), d2, C * gh * gw * elem, elem)
                assert_destinations_refused(ctx, lambda n, src, stride: run([(0, k) for k in range(n)], p, src=src, sstride=stride, sframes=n),
                                            s, C * sh * sw * elem, elem)
        assert_destinations_refused(ctx, lambda n, dst, stride: run([(k, 0) for k in range(n)], prm(), pool=dst, pstride=stride, frames=n), d, tsize, 4)
        # the sources and the destinations overlap: the same memory, one inside the other, by one element at either end
        ssize, fsize = C * sh * sw * 2, C * gh * gw * 2
        assert run(ok, prm(), dst=s) == -2 and run(ok, prm(), src=d2) == -2
        assert run(ok, prm(), dst=s + 3 * ssize - 2) == -2
        assert run(ok, prm(), src=d2 + 3 * fsize - 2) == -2
        assert run(ok, prm(), dst=s + ssize, stride=fsize + 64) == -2
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()            # nothing was enqueued
        # ... and side by side they are accepted: the destinations and nothing else are written
        assert run(ok, prm(), dst=s + 3 * ssize) == 0
        assert run(ok, prm()) == 0
        ctx.sync()
        a = big.cpu().numpy()
        fill_t = np.full((h, w), 0x5C5C5C5C, np.uint32)     # (an entry nobody wrote: clamped, garbage, in bounds)
        fill_s = np.full((C, sh, sw), 0x5C5C, np.uint16)
        ref = G.nearest(fill_s, fill_t, w, h, gw, gh)
        for base in ((1 << 21) + 3 * ssize, 2 << 21):
            assert a[base:base + 3 * fsize].tobytes() == ref.tobytes() * 3
        assert (a[:(1 << 21) + 3 * ssize] == 0x5C).all() and (a[(1 << 21) + 3 * ssize + 3 * fsize:2 << 21] == 0x5C).all()
        assert (a[(2 << 21) + 3 * fsize:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        pool = ctx.trace_pool(4)
        pool.zero_()
        src = torch.zeros((2, C, sh, sw), dtype=torch.float16, device="cuda:0")
        with pytest.raises(ValueError):
            ctx.trace_gather(pool.view(torch.float16), [(0, 0)], src)
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src, width=34)
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src, filter="cubic")
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0, 0)], src)
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src[0])
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src.cpu())
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src[:, :, :, ::2])
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src.permute(0, 1, 3, 2))
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src.double())
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src.view(torch.int16), filter="bilinear")
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src.to(torch.uint8), filter="bilinear")
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src, 16384, 2)
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src, 34, 23, out=torch.empty((1, C, 23, 34), dtype=torch.float16, device="cuda:0",
                                                                         memory_format=torch.channels_last))
        with pytest.raises(ValueError):
            ctx.trace_gather(pool, [(0, 0)], src, 34, 23, out=torch.empty((1, C, 23, 34), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RuntimeError):
            ctx.trace_gather(pool, [(4, 0)], src)
        with pytest.raises(RuntimeError):
            ctx.trace_gather(pool, [(0, 2)], src)
        with pytest.raises(RuntimeError):
            ctx.trace_gather(pool, [], src)
        got = ctx.trace_gather(pool, [(0, 0)], src, 34, 23, filter="bilinear")
        assert got.shape == (1, C, 23, 34) and got.is_contiguous()
        one = torch.as_strided(src, (1, C, sh, sw), (0, sh * sw, sw, 1))          # (a single tensor: its stride(0) is nobody's business)
        assert torch.equal(ctx.trace_gather(pool, [(0, 0)], one, 34, 23), ctx.trace_gather(pool, [(0, 0)], src, 34, 23))
        got = ctx.trace_gather(pool, [(0, 1)], src.contiguous(memory_format=torch.channels_last), 34, 23)
        assert got.shape == (1, C, 23, 34) and got.is_contiguous(memory_format=torch.channels_last) and not got.is_contiguous()
    finally:
        ctx.close()


def test_ordering_against_a_later_trace(pkg):
    """the gather, then at once a frames_trace that rewrites the pool entry it reads, then the tensor read on torch's stream: it was
    made of the trace that was there at the call; a gather queued after the rewrite sees the new one"""
    P = pkg
    w, h, frames = P.read_ivf(ivf_path("p_odd_130x98"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 1, 2)
        hdrs = []
        for i in range(2):
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, frames[i], i)
            parser.swap(hdr)
            hdrs.append(hdr)
        assert hdrs[0].frame_type == 0 and hdrs[1].frame_type == 1
        rng = np.random.default_rng(7)
        old = random_trace(rng, w, h)
        pool = ctx.trace_pool(2)
        ctx.frames_trace([(0, 0, None)], pool)
        pool[1] = to_pool(old)
        src = random_src(rng, 2, 16, 13, 17, "f32")
        src_t = on_device(src, "planar")
        jobs = [(1, 0), (1, 1)] * 12
        got = ctx.trace_gather(pool, jobs, src_t, filter="bilinear")
        ctx.frames_trace([(1, 1, (0, -1, -1))], pool)       # no wait in between
        later = ctx.trace_gather(pool, jobs[:2], src_t, filter="bilinear")
        res, res_later = got.cpu().numpy(), later.cpu().numpy()       # .cpu() on torch's current stream
        new = dwords(pool[1])
        assert np.array_equal(dwords(pool[0]), T.identity(w, h)) and (new != old).any() and (new != T.identity(w, h)).any()
        for k, (_, sidx) in enumerate(jobs):
            assert G.bilinear_excess(res[k], *G.bilinear(src[sidx], old, w, h)) <= 0.0, k
        for k in range(2):
            assert G.bilinear_excess(res_later[k], *G.bilinear(src[k], new, w, h)) <= 0.0, k
            assert np.array_equal(res_later[k], res[k]) is False
        # NEAREST, where "the old trace" is a matter of bits
        pool[1] = to_pool(old)
        got = ctx.trace_gather(pool, jobs, src_t, 45, 37)
        ctx.frames_trace([(1, 1, (0, -1, -1))], pool)
        res = got.cpu().numpy()
        for k, (_, sidx) in enumerate(jobs):
            assert np.array_equal(res[k], G.nearest(src[sidx], old, w, h, 45, 37)), k
    finally:
        parser.close()
        ctx.close()


@pytest.mark.parametrize("form", ["tiles", "raster"])
def test_nothing_else_is_touched(pkg, form, monkeypatch):
    """no device memory is added, and the pool, the sources and every frame buffer are bit-identical before and after"""
    ctx, pool, mine, shown, types = traced_stream(pkg, "p_odd_130x98", form, monkeypatch)
    try:
        w, h = ctx.width, ctx.height
        nfb = len(types)
        rng = np.random.default_rng(11)
        srcs = [(random_src(rng, 2, 5, h, w, "u8"), "planar", "nearest"), (random_src(rng, 2, 16, 13, 17, "f16"), "channels_last", "bilinear"),
                (random_src(rng, 2, 3, 25, 33, "f32"), "planar", "bilinear")]
        src_ts = [on_device(a, layout) for a, layout, _ in srcs]
        rgb_before = ctx.frames_rgb(list(range(nfb)))       # (read in the form the frames have: nothing is converted)
        ctx.sync()
        before, scratch = ctx.memory_usage(), ctx.rgb_scratch_bytes()
        pool_before = pool.clone()
        src_before = [t.clone() for t in src_ts]
        jobs = [(len(types) - 1, 0), (1, 1), (0, 0)]
        for (a, layout, filt), t in zip(srcs, src_ts):
            for out_size in ((0, 0), (224, 224)):
                check(ctx, pool, jobs, t, a, mine, size=out_size, filt=filt, what=(form, layout, filt))
        ctx.sync()
        assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == scratch
        if form == "tiles":
            assert before["raster_pool"] == 0
        assert torch.equal(pool, pool_before)
        assert all(torch.equal(t, b) for t, b in zip(src_ts, src_before))
        assert torch.equal(ctx.frames_rgb(list(range(nfb))), rgb_before)
        # ... and the whole frame buffers, borders included: downloaded (which gives tiled frames their raster form), then once more
        full_before = [ctx.download_full(k) for k in range(nfb)]
        check(ctx, pool, jobs, src_ts[0], srcs[0][0], mine)
        ctx.sync()
        assert all(np.array_equal(ctx.download_full(k), b) for k, b in enumerate(full_before))
    finally:
        ctx.close()


def test_one_1080p_frame(pkg):
    """several workgroups a job: float16 feature maps at an eighth of 1080p in both layouts with both filters, a label map of bytes at
    the display size"""
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
            ctx.frames_trace([job], pool)
            parser.swap(hdr)
        fb = job[1]
        assert hdr.frame_type == 1
        traces = dwords(pool)
        assert (traces[fb] != T.identity(w, h)).any()
        rng = np.random.default_rng(1080)
        feats = random_src(rng, 1, 8, 135, 240, "f16")
        for layout in LAYOUTS:
            ft = on_device(feats, layout)
            for filt in ("nearest", "bilinear"):
                check(ctx, pool, [(fb, 0)], ft, feats, traces, size=(240, 135), filt=filt, what=(layout, filt))
        labels = random_src(rng, 1, 1, h, w, "u8")
        check(ctx, pool, [(fb, 0)], on_device(labels, "planar"), labels, traces)
    finally:
        parser.close()
        ctx.close()
