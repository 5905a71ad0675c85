"""GPU (-m gpu): accumulated motion in device memory (vp8hip_frames_trace_async, vp8hip_trace_flow_async; Vp8Hip.frames_trace,
Vp8Hip.trace_flow; csrc/hip/vp8_trace.hip), dword for dword against the numpy restatement (tests/trace_reference.py) applied to the
slot as vp8hip_ir_fetch / vp8hip_ir_fetch_mvs read it back and to the restatement's own pool, for slots written by the host parser
and by the device's entropy decoder.  torch is imported here, before the package loads libvpx's library: one HIP runtime per
process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path
from handover_testlib import (TORCH_DTYPE, Producer, assert_destinations_refused, assert_guards_intact, bits, equal_on_device, guarded,
                              later_writers_producer, write_later_frames)
import trace_reference as R
from trace_testlib import dwords, random_trace, slot_ir, to_pool

pytestmark = pytest.mark.gpu

SCALES = [(1.0, 1.0), "pixels", (0.125, -3.0), (-1.0 / 3, 1e-3)]


def refs_as_the_parser_numbers_them(prod):
    """-> a dict whose "refs" is (new, last, golden, alt) of the frame Producer.put just placed: vp8_refs as it stood before the swap"""
    seen = {}
    swap = prod.parser.swap

    def noting(hdr):
        r = prod.parser.refs
        seen["refs"] = (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx)
        swap(hdr)
    prod.parser.swap = noting
    return seen


def check_flow(ctx, pool, idx, want, dw, dh, dtype, scale, what=None, **kw):
    """entries idx of the pool through trace_flow against the restatement on `want` (their traces, numpy)"""
    size = {} if dw == 0 else dict(width=dw, height=dh)
    got = ctx.trace_flow(pool, idx, dtype=TORCH_DTYPE[dtype], scale=scale, **size, **kw).cpu().numpy()
    w, h = ctx.width, ctx.height
    sc = R.pixel_scale(w, h, dw, dh) if scale == "pixels" else (1.0, 1.0) if scale is None else scale
    assert got.shape[0] == len(idx)
    for k, t in enumerate(want):
        ref = R.flow(t, dw, dh, dtype, sc)
        assert got[k].shape == ref.shape and np.array_equal(bits(got[k], dtype), bits(ref, dtype)), (what, k, dw, dh, dtype, scale)


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98", "p_split_352x288"])
def test_streams_every_frame_every_producer(pkg, name, how):
    """every frame of the stream through slot 0, its trace made with the parser's own reference numbers as entries of a pool of four
    (hidden frames, golden and altref updates included); every third frame as a flow tensor, types and sizes in rotation"""
    P = pkg
    prod = Producer(P, name, how)
    ctx, w, h = prod.ctx, prod.w, prod.h
    seen = refs_as_the_parser_numbers_them(prod)
    sweep = itertools.cycle(itertools.product(((0, 0), (224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h)), ("i16", "f32", "f16")))
    scales = itertools.cycle(SCALES)
    try:
        assert ctx.L.vp8hip_trace_size(ctx.h) == 4 * w * h == P.trace_size(w, h)
        pool = ctx.trace_pool(4)
        assert pool.shape == (4, h, w, 2) and pool.dtype == torch.int16
        pool.zero_()
        mine = [np.zeros((h, w), np.uint32) for _ in range(4)]
        n_inter = n_hidden = 0
        for i in range(len(prod.frames)):
            hdr = prod.put(i)
            new, lst, gld, alt = seen["refs"]
            assert ctx.frames_trace([(0, new, (lst, gld, alt))], pool) is pool
            mbs, mvs = slot_ir(ctx, 0)
            mine[new] = R.trace(hdr, mbs, mvs, [mine[lst], mine[gld], mine[alt]])
            assert np.array_equal(dwords(pool[new]), mine[new]), (name, how, i)
            n_inter += hdr.frame_type != 0
            n_hidden += not hdr.show_frame
            if i % 3 == 0:
                (dw, dh), dtype = next(sweep)
                check_flow(ctx, pool, [new], [mine[new]], dw, dh, dtype, next(scales), what=(name, how, i))
        assert n_inter > 0
        if name == "p_arf_176x144":
            assert n_hidden == 5
        for k in range(4):                               # nothing but the destinations was written
            assert np.array_equal(dwords(pool[k]), mine[k])
    finally:
        prod.close()


def test_batch_of_600_jobs(pkg):
    """600 jobs in one call -- more than two launches' worth and a remainder --, slots repeated and permuted, destinations distinct,
    references drawn from eight entries of seeded random positions, some -1"""
    P = pkg
    nsrc, nref, n = 30, 8, 600
    prod = Producer(P, "p_seg_176x144", "host", nslots=nsrc)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        hdrs = [prod.put(i, i) for i in range(nsrc)]
        irs = [slot_ir(ctx, i) for i in range(nsrc)]
        rng = np.random.default_rng(600)
        pool = ctx.trace_pool(nref + n)
        given = [random_trace(rng, w, h) for _ in range(nref)]
        for k in range(nref):
            pool[k] = to_pool(given[k])
        slots = rng.integers(0, nsrc, n)
        dsts = nref + rng.permutation(n)
        refs = np.where(rng.random((n, 3)) < 0.2, -1, rng.integers(0, nref, (n, 3)))
        jobs = [(int(slots[i]), int(dsts[i]), tuple(int(r) for r in refs[i])) for i in range(n)]
        ctx.frames_trace(jobs, pool)
        want = [None] * n
        for s, d, r in jobs:
            want[d - nref] = R.trace(hdrs[s], irs[s][0], irs[s][1], [given[q] if q >= 0 else None for q in r]).reshape(h, w, 1)
        assert equal_on_device(pool[nref:], want, list(range(n)), "f32") == []
        assert equal_on_device(pool[:nref], [g.reshape(h, w, 1) for g in given], list(range(nref)), "f32") == []
        # a flow call over more entries than one launch carries, with repeats
        idx = [int(i) for i in rng.integers(0, nref + n, 700)]
        fl = ctx.trace_flow(pool, idx, 45, 37, dtype=torch.float16, scale=(0.5, 0.25))
        every = given + [t.reshape(h, w) for t in want]
        flows = {i: R.flow(every[i], 45, 37, "f16", (0.5, 0.25)) for i in set(idx)}
        order = sorted(flows)
        assert equal_on_device(fl, [flows[i] for i in order], [order.index(i) for i in idx], "f16") == []
    finally:
        prod.close()


def _random_ir(rng, nmb):
    mbs = np.zeros((nmb, 64), np.uint8)
    mbs[:, 0] = rng.integers(0, 10, nmb)
    mbs[:, R.O_REF] = np.where(mbs[:, 0] < 5, 0, rng.integers(1, 4, nmb))
    mbs[:, 3] = rng.integers(0, 4, nmb)
    mbs[:, 5] = rng.integers(0, 4, nmb)
    mvs = rng.integers(-32768, 32768, (nmb, 16, 2)).astype(np.int16)
    ties = rng.random((nmb, 16, 2)) < 0.25              # exactly half-way between two pixels, and small whole steps
    mvs[ties] = rng.choice(np.array([4, -4, 12, -12, 8, -8, 0, 3, -5], np.int16), int(ties.sum()))
    return mbs, mvs


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45), (130, 98), (8208, 16)])
def test_random_ir_wild_vectors(pkg, size):
    """random records (every ref_frame and y_mode) with vectors over all of int16 and on the ties, an inter and a key header, into a
    pool at offsets 4 and 16 of its allocation with strides that are and are not multiples of 16: the traces, and the bytes around
    the entries (8208x16: one macroblock row of 513)"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 31 + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 2)
        nmb = ctx.nmb
        coef = np.zeros((nmb, 400), np.int16)
        hdrs, irs = [], []
        for slot, ft in enumerate((1, 0)):
            hdr = P.FrameHdr()
            hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows, hdr.frame_type = w, h, (w + 15) // 16, (h + 15) // 16, ft
            mbs, mvs = _random_ir(rng, nmb)
            ctx.fill_slot(slot, hdr, mbs, coef, mvs)
            ir = slot_ir(ctx, slot)
            assert np.array_equal(ir[0][:, :8], mbs[:, :8])
            if ft:
                assert np.array_equal(ir[1].reshape(mvs.shape), mvs)
            hdrs.append(hdr)
            irs.append(ir)
        assert set(np.unique(irs[0][0][:, R.O_REF]).tolist()) == {0, 1, 2, 3} or nmb < 60
        size_b = 4 * w * h
        n = 6
        for off, pad in ((4, 4), (16, 0), (16, 8), (4, 12), (16, 16)):
            big, flat = guarded(n, size_b, pad, off)
            pool = flat.view(torch.int16).unflatten(1, (h, w, 2))
            assert pool.data_ptr() % 16 == off % 16 and pool.stride(0) * 2 == size_b + pad
            given = [random_trace(rng, w, h) for _ in range(3)]
            for k in range(3):
                pool[k] = to_pool(given[k])
            ctx.frames_trace([(0, 3, (0, 1, 2)), (1, 4, (2, -1, 0))], pool)
            ctx.frames_trace([(0, 5, (1, -1, 3))], pool)                  # chained off entry 3, golden missing
            got = dwords(pool)
            t3 = R.trace(hdrs[0], *irs[0], given)
            assert np.array_equal(got[3], t3), (size, off, pad)
            assert np.array_equal(got[4], R.identity(w, h)), (size, off, pad)
            assert np.array_equal(got[5], R.trace(hdrs[0], *irs[0], [given[1], None, t3])), (size, off, pad)
            for k in range(3):
                assert np.array_equal(got[k], given[k])
            assert_guards_intact(big, n, size_b, pad, off, what=(size, off, pad))
            # the same entries as flow tensors into guarded destinations, the pool where it is
            for dtype, (dw, dh) in (("i16", (0, 0)), ("f32", (min(w + 1, 16383), h + 3)), ("f16", (max(1, w // 3), 5))):
                gw, gh = (w, h) if dw == 0 else (dw, dh)
                es = 4 if dtype == "f32" else 2
                fsize = 2 * gh * gw * es
                foff, fpad = off // es * es, pad // es * es
                fbig, fflat = guarded(2, fsize, fpad, foff, 0x3C)
                out = fflat.view(TORCH_DTYPE[dtype]).unflatten(1, (2, gh, gw))
                check_flow(ctx, pool, [5, 3], [got[5], got[3]], dw, dh, dtype, (0.25, -0.5), what=(size, off, pad), out=out)
                assert_guards_intact(fbig, 2, fsize, fpad, foff, 0x3C, what=(size, off, pad, dtype))
    finally:
        ctx.close()


def test_one_1080p_frame(pkg):
    """several groups of macroblock rows a frame"""
    P = pkg
    prod = Producer(P, "p_1920x1080", "host")
    ctx, w, h = prod.ctx, prod.w, prod.h
    seen = refs_as_the_parser_numbers_them(prod)
    try:
        pool = ctx.trace_pool(4)
        pool.zero_()
        mine = [np.zeros((h, w), np.uint32) for _ in range(4)]
        for i in range(2):
            hdr = prod.put(i)
            new, lst, gld, alt = seen["refs"]
            ctx.frames_trace([(0, new, (lst, gld, alt))], pool)
            mbs, mvs = slot_ir(ctx, 0)
            mine[new] = R.trace(hdr, mbs, mvs, [mine[lst], mine[gld], mine[alt]])
            assert np.array_equal(dwords(pool[new]), mine[new]), i
        assert hdr.frame_type == 1 and (mine[new] != R.identity(w, h)).any()
        check_flow(ctx, pool, [new], [mine[new]], 224, 224, "f32", "pixels")
        check_flow(ctx, pool, [new], [mine[new]], 0, 0, "f16", (1.0, 1.0))
    finally:
        prod.close()


def test_refusals(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host", nslots=4)
    ctx, w, h = prod.ctx, prod.w, prod.h
    L = ctx.L
    try:
        hdrs = [prod.put(i, i) for i in range(3)]       # slot 3 is never filled
        irs = [slot_ir(ctx, i) for i in range(3)]
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        d2 = d + (1 << 21)
        assert d % 16 == 0
        size = 4 * w * h
        assert L.vp8hip_trace_size(ctx.h) == size and 8 * size < 1 << 21

        def jobs_of(*jobs):
            arr = (P.Job * len(jobs))()
            for i, (slot, dst, refs) in enumerate(jobs):
                arr[i].ir_slot, arr[i].dst_fb = slot, dst
                arr[i].ref_fb[0] = -1
                for k in range(3):
                    arr[i].ref_fb[k + 1] = refs[k]
            return arr

        def trace(jobs, n=None, pool=d, stride=size, frames=8):
            arr = jobs_of(*jobs)
            return L.vp8hip_frames_trace_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.c_void_p(pool) if pool else None, stride, frames)
        ok = (1, 3, (0, 1, 2))
        assert trace([ok], n=0) == -2 and trace([ok], n=-1) == -2
        for bad in (-1, 4, 1 << 20):
            assert trace([(bad, 3, (0, 1, 2))]) == -2, bad
        assert trace([(3, 3, (0, 1, 2))]) == -2                                        # never filled
        assert trace([ok, (3, 4, (0, 1, 2))]) == -2
        for frames in (0, -1):
            assert trace([ok], frames=frames) == -2
        for dst in (-1, 8, 1 << 20):                                                   # the destination outside the pool
            assert trace([(1, dst, (0, 1, 2))]) == -2, dst
        for ref in (-2, 8, 1 << 20):                                                   # a reference neither -1 nor in range
            for q in range(3):
                refs = [0, 1, 2]
                refs[q] = ref
                assert trace([(1, 3, tuple(refs))]) == -2, (ref, q)
        for q in range(3):                                                             # the destination a reference of its own job ...
            refs = [0, 1, 2]
            refs[q] = 3
            assert trace([(1, 3, tuple(refs))]) == -2, q
        assert trace([(0, 3, (-1, -1, -1)), (1, 3, (0, 1, 2))]) == -2                  # ... a key frame's too
        assert trace([ok, (2, 4, (0, 3, -1))]) == -2                                   # ... of another job, after it and before it
        assert trace([(2, 4, (0, 3, -1)), ok]) == -2
        assert trace([ok, (2, 3, (0, 1, 2))]) == -2                                    # two jobs, one destination
        # the pool itself: three entries, a job that needs them all (one entry: a job that needs none)
        assert_destinations_refused(ctx, lambda n, dst, stride: trace([(1, 0, (1, 2, -1) if n == 3 else (-1, -1, -1))], pool=dst, stride=stride,
                                                                      frames=n), d, size, 4)

        def prm(dw=34, dh=23, dtype=0):
            return P.TraceFlowParams(dw, dh, dtype)

        def flow(idx, p, n=None, pool=d, pstride=size, frames=8, dst=d2, stride=None):
            arr = (ctypes.c_int * len(idx))(*idx)
            fsize = int(L.vp8hip_trace_flow_size(ctx.h, ctypes.byref(p)))
            return L.vp8hip_trace_flow_async(ctx.h, arr, len(idx) if n is None else n, ctypes.byref(p), ctypes.c_void_p(pool) if pool else None,
                                             pstride, frames, ctypes.c_void_p(dst) if dst else None, fsize if stride is None else stride)
        assert L.vp8hip_trace_flow_size(ctx.h, ctypes.byref(prm())) == 2 * 23 * 34 * 2
        assert L.vp8hip_trace_flow_size(ctx.h, ctypes.byref(prm(0, 0, 2))) == 2 * h * w * 4
        assert flow([0, 1, 2], prm(), n=0) == -2 and flow([0, 1, 2], prm(), n=-1) == -2
        for bad in (-1, 8, 1 << 20):
            assert flow([0, bad], prm()) == -2, bad
        for frames in (0, -1):
            assert flow([0], prm(), frames=frames) == -2
        for dw, dh in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert flow([0, 1, 2], prm(dw, dh), stride=1 << 19) == -2, (dw, dh)
        for dt in (-1, 3):
            assert flow([0, 1, 2], prm(dtype=dt), stride=1 << 19) == -2
        for dtype, es in ((0, 2), (1, 2), (2, 4)):          # the destination, each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: flow([0, 1, 2][:n], prm(dtype=dtype), dst=dst, stride=stride), d2,
                                        2 * 23 * 34 * es, es)
        assert_destinations_refused(ctx, lambda n, dst, stride: flow([0, 1, 2][:n], prm(), pool=dst, pstride=stride, frames=n), d, size, 4)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                                       # nothing was enqueued
        # the same calls into memory the test owns are accepted: the destinations and nothing else are written
        assert trace([(0, 3, (0, 1, 2)), (1, 4, (0, -1, 2))]) == 0
        assert flow([4, 3, 4], prm()) == 0
        ctx.sync()
        a = big.cpu().numpy()
        fill = np.full((h, w), 0x5C5C5C5C, np.uint32)
        t3 = R.trace(hdrs[0], *irs[0], [fill] * 3)
        t4 = R.trace(hdrs[1], *irs[1], [fill, None, fill])
        assert hdrs[0].frame_type == 0 and hdrs[1].frame_type == 1
        assert a[3 * size:4 * size].tobytes() == t3.tobytes() and a[4 * size:5 * size].tobytes() == t4.tobytes()
        fsize = 2 * 23 * 34 * 2
        for k, t in enumerate((t4, t3, t4)):
            assert a[(1 << 21) + k * fsize:(1 << 21) + (k + 1) * fsize].tobytes() == R.flow(t, 34, 23).tobytes()
        assert (a[:3 * size] == 0x5C).all() and (a[5 * size:1 << 21] == 0x5C).all() and (a[(1 << 21) + 3 * fsize:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        pool = ctx.trace_pool(4)
        with pytest.raises(ValueError):
            ctx.frames_trace([(0, 0, None)], pool.view(torch.float16))
        with pytest.raises(ValueError):
            ctx.frames_trace([(0, 0, None)], torch.empty((4, h, w + 2, 2), dtype=torch.int16, device="cuda:0")[:, :, :w])
        with pytest.raises(ValueError):
            ctx.trace_flow(pool, [0], width=34)
        with pytest.raises(ValueError):
            ctx.trace_flow(pool, [0], dtype=torch.int8)
        with pytest.raises(ValueError):
            ctx.trace_flow(pool, [0], scale="nope")
        with pytest.raises(ValueError):
            ctx.trace_flow(pool, [0, 1], 34, 23, out=torch.empty((2, 2, 23, 36), dtype=torch.int16, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError):
            ctx.frames_trace([(3, 0, None)], pool)
        with pytest.raises(RuntimeError):
            ctx.frames_trace([(1, 0, (0, 1, 2))], pool)
        with pytest.raises(RuntimeError):
            ctx.trace_flow(pool, [4])
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the pool read on torch's stream: the traces are those of the frames that were there at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        irs = [slot_ir(ctx, i) for i in range(n)]
        rng = np.random.default_rng(4)
        given = [random_trace(rng, w, h) for _ in range(3)]
        pool = ctx.trace_pool(n + 3)
        for k in range(3):
            pool[n + k] = to_pool(given[k])
        jobs = [(i, i, (n, n + 1, n + 2)) for i in range(n)]
        old = [R.trace(hdrs[i], *irs[i], given) for i in range(n)]
        ctx.frames_trace(jobs, pool)
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        got = dwords(pool)                               # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(got[i], old[i]), i
        ctx.sync()
        # ... and the slots now hold the later frames
        changed = 0
        ctx.frames_trace(jobs, pool)
        got = dwords(pool)
        for i in range(n):
            ir = slot_ir(ctx, i)
            assert np.array_equal(got[i], R.trace(new_hdrs[i], *ir, given)), i
            changed += not np.array_equal(ir[1], irs[i][1])
        assert changed > 0
    finally:
        prod.close()


def test_float_types_on_every_difference(pkg):
    """a pool entry crafted so that T - p takes every value in -16383 .. 16383 on both channels, against scales that make the float
    land on ties of the halves (the half is the FLOAT rounded: two roundings), powers of two, negative ones and denormals"""
    P = pkg
    w, h = 1024, 64                                     # 65536 pixels for 32767 differences, twice
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        a = (np.arange(w * h) % 32767 - 16383).reshape(h, w)
        ys, xs = np.mgrid[0:h, 0:w]
        t = R.pack(xs + a, ys + a[::-1, ::-1])           # (data, not positions: what lies outside the picture is carried all the same)
        pool = ctx.trace_pool(2)
        pool[1] = to_pool(t)
        i16 = R.flow(t)
        assert np.array_equal(i16[0], a) and np.array_equal(i16[1], a[::-1, ::-1])
        assert set(np.unique(i16[0]).tolist()) == set(range(-16383, 16384)) == set(np.unique(i16[1]).tolist())
        check_flow(ctx, pool, [1], [t], 0, 0, "i16", None)
        differ = 0
        for sx, sy in ((1.0285249948501587, 1.9014227390289307), (0.2968776226043701, 0.6305446028709412), (1.0, 0.125), (-1.0 / 3, 1e-3),
                       (1e-42, -3e-41), (2.0 ** -24, 65504.0 / 16383), (3.0e4, 1e30), (224 / 1920, 224 / 1080)):
            scale = (np.float32(sx), np.float32(sy))
            for dtype in ("f32", "f16"):
                check_flow(ctx, pool, [1], [t], 0, 0, dtype, scale, what=(sx, sy))
            with np.errstate(over="ignore"):
                once = (a.astype(np.float64) * np.float64(scale[0])).astype(np.float16)
            differ += int((once != R.flow(t, dtype="f16", scale=scale)[0]).sum())
        assert differ > 0                               # (the sweep holds values one rounding would get wrong)
    finally:
        ctx.close()


def test_no_new_device_memory_and_frame_buffers_untouched(pkg):
    P = pkg
    w, h, frames = P.read_ivf(ivf_path("p_odd_130x98"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 4, 1)
        pool = ctx.trace_pool(4)
        jobs = []
        for data in frames[:2]:
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            jobs.append((0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx)))
            ctx.decode(jobs[-1:], P.STAGE_ALL)
            if len(jobs) == 1:
                ctx.frames_trace(jobs[-1:], pool)
            parser.swap(hdr)
        fb = jobs[-1][1]
        before_fb = ctx.download_full(fb)
        before = ctx.memory_usage()
        ctx.frames_trace(jobs[-1:], pool)
        for size in ({}, dict(width=224, height=224)):
            ctx.trace_flow(pool, [fb], dtype=torch.float32, scale="pixels", **size)
        ctx.sync()
        assert ctx.memory_usage() == before
        assert ctx.rgb_scratch_bytes() == 0
        assert np.array_equal(ctx.download_full(fb), before_fb)
        mbs, mvs = slot_ir(ctx, 0)
        assert hdr.frame_type == 1
        _, lst, gld, alt = jobs[-1][1], *jobs[-1][2]
        ident = R.identity(w, h)
        assert lst == gld == alt == jobs[0][1]
        assert np.array_equal(dwords(pool[fb]), R.trace(hdr, mbs, mvs, [ident] * 3))
    finally:
        parser.close()
        ctx.close()
