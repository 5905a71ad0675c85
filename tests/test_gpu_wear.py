"""GPU (-m gpu): trace wear in device memory (vp8hip_frames_wear_async, vp8hip_trace_wear_async; Vp8Hip.frames_wear,
Vp8Hip.trace_wear; csrc/hip/vp8_trace_wear.hip), dword for dword and bit for bit against the numpy restatement
(tests/wear_reference.py) applied to the slot as vp8hip_ir_fetch / vp8hip_ir_fetch_mvs read it back and to the restatement's own
pool, for slots written by the host parser and by the device's entropy decoder.  torch is imported here, before the package loads
libvpx's library: one HIP runtime per process."""
import ctypes
import functools
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path
from handover_testlib import (TORCH_DTYPE, Producer, assert_destinations_refused, assert_guards_intact, bits, equal_on_device, guarded,
                              later_writers_producer, write_later_frames)
import trace_reference as R
import wear_reference as W
from trace_testlib import check_tensor as entry_check_tensor, dwords, slot_ir, to_pool

pytestmark = pytest.mark.gpu

SCALES = [None, (1.0, 0.5, 0.25, 2.0), 1.0 / 255, (-1.0 / 3, 1e-3, 1.0285249948501587, 3.0e4)]
PLANE_SETS = [("hops", "intra", "edge", "coded"), ("coded",), ("edge", "hops"), 14, ("intra",), 9]


wear_dwords = dwords                                          # uint8 [..., h, w, 4] on the device -> numpy uint32 [..., h, w]
to_wear_pool = functools.partial(to_pool, dtype=np.uint8)     # numpy uint32 [h, w] -> uint8 [h, w, 4] on the device
# entries idx of the pool through trace_wear against the restatement on `want` (their wear, numpy)
check_tensor = functools.partial(entry_check_tensor, "trace_wear", W.tensor, 4)


def random_wear(rng, w, h):
    """seeded random counters, a quarter of the bytes 254 or 255: the saturating add's cases"""
    c = rng.integers(0, 256, (4, h, w))
    high = rng.random((4, h, w)) < 0.25
    c[high] = rng.integers(254, 256, int(high.sum()))
    return W.pack(c)


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


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98", "p_split_352x288"])
def test_streams_every_frame_every_producer(pkg, name, how):
    """every frame of the stream through slot 0, its wear made with the parser's own reference numbers as entries of a pool of four
    (hidden frames, golden and altref updates included) and its trace into a trace pool beside it; every third frame as a tensor,
    sizes, types, planes and scales in rotation"""
    P = pkg
    prod = Producer(P, name, how)
    ctx, w, h = prod.ctx, prod.w, prod.h
    seen = refs_as_the_parser_numbers_them(prod)
    sweep = itertools.cycle(itertools.product(((0, 0), (224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h)), ("u8", "f32", "f16")))
    scales, plane_sets = itertools.cycle(SCALES), itertools.cycle(PLANE_SETS)
    try:
        pool, traces = ctx.wear_pool(4), ctx.trace_pool(4)
        assert pool.shape == (4, h, w, 4) and pool.dtype == torch.uint8 and pool[0].numel() == ctx.L.vp8hip_trace_size(ctx.h)
        pool.zero_()
        traces.zero_()
        mine = [np.zeros((h, w), np.uint32) for _ in range(4)]
        mine_t = [np.zeros((h, w), np.uint32) for _ in range(4)]
        top = np.zeros(4, int)
        for i in range(len(prod.frames)):
            hdr = prod.put(i)
            new, lst, gld, alt = seen["refs"]
            job = [(0, new, (lst, gld, alt))]
            assert ctx.frames_wear(job, pool) is pool
            ctx.frames_trace(job, traces)
            mbs, mvs = slot_ir(ctx, 0)
            mine[new] = W.wear(hdr, mbs, mvs, [mine[lst], mine[gld], mine[alt]])
            mine_t[new] = R.trace(hdr, mbs, mvs, [mine_t[lst], mine_t[gld], mine_t[alt]])
            assert np.array_equal(wear_dwords(pool[new]), mine[new]), (name, how, i)
            assert np.array_equal(dwords(traces[new]), mine_t[new]), (name, how, i)
            top = np.maximum(top, W.unpack(mine[new]).reshape(4, -1).max(1))
            if i % 3 == 0:
                (dw, dh), dtype = next(sweep)
                check_tensor(ctx, pool, [new], [mine[new]], dw, dh, dtype, next(plane_sets), next(scales), what=(name, how, i))
        assert (top > 0).all(), top
        for k in range(4):                               # nothing but the destinations was written
            assert np.array_equal(wear_dwords(pool[k]), mine[k]) and np.array_equal(dwords(traces[k]), mine_t[k])
    finally:
        prod.close()


def test_batch_of_600_jobs(pkg):
    """600 jobs in one call -- more than one launch's worth and a remainder --, slots repeated and permuted, destinations distinct,
    references drawn from eight entries of seeded random counters, some -1; then a tensor call over 700 indices with repeats"""
    P = pkg
    nsrc, nref, n = 30, 8, 600
    prod = Producer(P, "p_seg_176x144", "host", nslots=nsrc)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        hdrs = [prod.put(i, i) for i in range(nsrc)]
        irs = [slot_ir(ctx, i) for i in range(nsrc)]
        rng = np.random.default_rng(601)
        pool = ctx.wear_pool(nref + n)
        given = [random_wear(rng, w, h) for _ in range(nref)]
        for k in range(nref):
            pool[k] = to_wear_pool(given[k])
        slots = rng.integers(0, nsrc, n)
        dsts = nref + rng.permutation(n)
        refs = np.where(rng.random((n, 3)) < 0.2, -1, rng.integers(0, nref, (n, 3)))
        jobs = [(int(slots[i]), int(dsts[i]), tuple(int(r) for r in refs[i])) for i in range(n)]
        ctx.frames_wear(jobs, pool)
        want = [None] * n
        for s, d, r in jobs:
            want[d - nref] = W.wear(hdrs[s], irs[s][0], irs[s][1], [given[q] if q >= 0 else None for q in r])
        as32 = pool.view(torch.int32)                    # [entries, h, w, 1]: equal_on_device compares dwords
        assert equal_on_device(as32[nref:], [t.reshape(h, w, 1) for t in want], list(range(n)), "f32") == []
        assert equal_on_device(as32[:nref], [g.reshape(h, w, 1) for g in given], list(range(nref)), "f32") == []
        idx = [int(i) for i in rng.integers(0, nref + n, 700)]
        sc = (0.5, 0.25, 3.0, 1.0 / 255)
        out = ctx.trace_wear(pool, idx, 45, 37, planes=("hops", "edge", "coded"), dtype=torch.float16, scale=sc)
        every = given + want
        tens = {i: W.tensor(every[i], 45, 37, 13, "f16", sc) for i in set(idx)}
        order = sorted(tens)
        assert equal_on_device(out, [tens[i] for i in order], [order.index(i) for i in idx], "f16") == []
    finally:
        prod.close()


def _random_ir(rng, nmb):
    """records of every y_mode and ref_frame (a few beyond 3), flags, partitionings and eobs at random, vectors over all of int16 and
    on the ties"""
    mbs = np.zeros((nmb, 64), np.uint8)
    mbs[:, W.O_MODE] = rng.integers(0, 10, nmb)
    mbs[0, W.O_MODE] = rng.integers(5, 10)               # (an inter macroblock in every frame, and an intra one beside it)
    mbs[1:2, W.O_MODE] = rng.integers(0, 5)
    mbs[:, W.O_REF] = np.where(mbs[:, W.O_MODE] < 5, 0, rng.integers(1, 4, nmb))
    wild = (mbs[:, W.O_REF] != 0) & (rng.random(nmb) < 0.06) & (np.arange(nmb) > 0)
    mbs[wild, W.O_REF] = rng.integers(4, 256, int(wild.sum()))
    mbs[:, W.O_FLAGS] = rng.integers(0, 4, nmb)
    mbs[:, 5] = rng.integers(0, 4, nmb)
    mbs[:, W.O_EOBS:W.O_EOBS + 25] = rng.choice(np.array([0, 0, 1, 1, 2, 16], np.uint8), (nmb, 25))
    mvs = rng.integers(-32768, 32768, (nmb, 16, 2)).astype(np.int16)
    ties = rng.random((nmb, 16, 2)) < 0.25              # exactly half-way between two pixels, and small whole steps
    mvs[ties] = rng.choice(np.array([4, -4, 12, -12, 8, -8, 0, 3, -5], np.int16), int(ties.sum()))
    return mbs, mvs


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45), (130, 98), (8208, 16)])
def test_random_ir_wild_vectors(pkg, size):
    """random records with vectors over all of int16 and on the ties, an inter and a key header, references of random counters with
    bytes 254 and 255 among them, into a pool at offsets 4 and 16 of its allocation with strides that are and are not multiples of
    16: the wear, and the bytes around the entries (8208x16: one macroblock row of 513, wider than a four-row group's LDS)"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 37 + h)
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
            assert np.array_equal(ir[0][:, :8], mbs[:, :8]) and np.array_equal(ir[0][:, W.O_EOBS:W.O_EOBS + 25], mbs[:, W.O_EOBS:W.O_EOBS + 25])
            if ft:
                assert np.array_equal(ir[1].reshape(mvs.shape), mvs)
            hdrs.append(hdr)
            irs.append(ir)
        inc = W.incs(hdrs[0], *irs[0])
        assert inc[W.EDGE].any() and (nmb < 2 or (inc[W.INTRA].any() and not inc[W.INTRA].all()))
        assert nmb < 15 or all(inc[b].any() and not inc[b].all() for b in (W.EDGE, W.CODED))
        size_b = 4 * w * h
        n = 6
        for off, pad in ((4, 4), (16, 0), (16, 8), (4, 12), (16, 16)):
            big, flat = guarded(n, size_b, pad, off)
            pool = flat.unflatten(1, (h, w, 4))
            assert pool.data_ptr() % 16 == off % 16 and pool.stride(0) == size_b + pad
            given = [random_wear(rng, w, h) for _ in range(3)]
            for k in range(3):
                pool[k] = to_wear_pool(given[k])
            ctx.frames_wear([(0, 3, (0, 1, 2)), (1, 4, (2, -1, 0))], pool)
            ctx.frames_wear([(0, 5, (1, -1, 3))], pool)                   # chained off entry 3, golden missing
            got = wear_dwords(pool)
            t3 = W.wear(hdrs[0], *irs[0], given)
            assert np.array_equal(got[3], t3), (size, off, pad)
            assert not got[4].any(), (size, off, pad)
            assert np.array_equal(got[5], W.wear(hdrs[0], *irs[0], [given[1], None, t3])), (size, off, pad)
            for k in range(3):
                assert np.array_equal(got[k], given[k])
            assert_guards_intact(big, n, size_b, pad, off, what=(size, off, pad))
            # the same entries as tensors into guarded destinations, the pool where it is
            for dtype, (dw, dh), planes in (("u8", (0, 0), 15), ("f32", (min(w + 1, 16383), h + 3), ("edge", "coded")),
                                            ("f16", (max(1, w // 3), 5), 7), ("u8", (min(w + 3, 16383) // 4 * 4, 3), ("coded",))):
                gw, gh = (w, h) if dw == 0 else (dw, dh)
                es = {"u8": 1, "f16": 2, "f32": 4}[dtype]
                fsize = bin(W.plane_mask(planes)).count("1") * gh * gw * es
                foff, fpad = off // es * es, pad // es * es
                if dtype == "u8" and dw:                 # (bytes at an odd address: a width that is a multiple of 4, element by element)
                    foff += 1
                fbig, fflat = guarded(2, fsize, fpad, foff, 0x3C)
                out = fflat.view(TORCH_DTYPE[dtype]).unflatten(1, (-1, gh, gw))
                check_tensor(ctx, pool, [5, 3], [got[5], got[3]], dw, dh, dtype, planes, (0.25, -0.5, 3.0, 1.0 / 3), what=(size, off, pad), out=out)
                assert_guards_intact(fbig, 2, fsize, fpad, foff, 0x3C, what=(size, off, pad, dtype))
    finally:
        ctx.close()


def test_one_1080p_frame(pkg):
    """several groups of four macroblock rows a frame, the largest LDS"""
    P = pkg
    prod = Producer(P, "p_1920x1080", "host")
    ctx, w, h = prod.ctx, prod.w, prod.h
    seen = refs_as_the_parser_numbers_them(prod)
    try:
        pool = ctx.wear_pool(4)
        rng = np.random.default_rng(1080)
        mine = [random_wear(rng, w, h) for _ in range(4)]
        for k in range(4):
            pool[k] = to_wear_pool(mine[k])
        for i in range(2):
            hdr = prod.put(i)
            new, lst, gld, alt = seen["refs"]
            ctx.frames_wear([(0, new, (lst, gld, alt))], pool)
            mbs, mvs = slot_ir(ctx, 0)
            mine[new] = W.wear(hdr, mbs, mvs, [mine[lst], mine[gld], mine[alt]])
            assert np.array_equal(wear_dwords(pool[new]), mine[new]), i
        c = W.unpack(mine[new])
        assert hdr.frame_type == 1 and (c[W.HOPS] == 1).all() and c[W.CODED].any() and not c[W.CODED].all()
        check_tensor(ctx, pool, [new], [mine[new]], 224, 224, "f32", 15, (1.0, 0.5, 0.25, 1.0 / 255))
        check_tensor(ctx, pool, [new], [mine[new]], 0, 0, "u8", ("coded", "hops"), None)
        check_tensor(ctx, pool, [new], [mine[new]], 0, 0, "f16", ("edge",), 0.5)
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

        def wear(jobs, n=None, pool=d, stride=size, frames=8):
            arr = jobs_of(*jobs)
            return L.vp8hip_frames_wear_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.c_void_p(pool) if pool else None, stride, frames)
        ok = (1, 3, (0, 1, 2))
        assert wear([ok], n=0) == -2 and wear([ok], n=-1) == -2
        for bad in (-1, 4, 1 << 20):
            assert wear([(bad, 3, (0, 1, 2))]) == -2, bad
        assert wear([(3, 3, (0, 1, 2))]) == -2                                         # never filled
        assert wear([ok, (3, 4, (0, 1, 2))]) == -2
        for frames in (0, -1):
            assert wear([ok], frames=frames) == -2
        for dst in (-1, 8, 1 << 20):                                                   # the destination outside the pool
            assert wear([(1, dst, (0, 1, 2))]) == -2, dst
        for ref in (-2, 8, 1 << 20):                                                   # a reference neither -1 nor in range
            for q in range(3):
                refs = [0, 1, 2]
                refs[q] = ref
                assert wear([(1, 3, tuple(refs))]) == -2, (ref, q)
        for q in range(3):                                                             # the destination a reference of its own job ...
            refs = [0, 1, 2]
            refs[q] = 3
            assert wear([(1, 3, tuple(refs))]) == -2, q
        assert wear([(0, 3, (-1, -1, -1)), (1, 3, (0, 1, 2))]) == -2                   # ... a key frame's too
        assert wear([ok, (2, 4, (0, 3, -1))]) == -2                                    # ... of another job, after it and before it
        assert wear([(2, 4, (0, 3, -1)), ok]) == -2
        assert wear([ok, (2, 3, (0, 1, 2))]) == -2                                     # two jobs, one destination
        # the pool itself: three entries, a job that needs them all (one entry: a job that needs none)
        assert_destinations_refused(ctx, lambda n, dst, stride: wear([(1, 0, (1, 2, -1) if n == 3 else (-1, -1, -1))], pool=dst, stride=stride,
                                                                     frames=n), d, size, 4)

        def prm(dw=34, dh=23, dtype=0, planes=5):
            return P.TraceWearParams(dw, dh, dtype, planes)

        def tens(idx, p, n=None, pool=d, pstride=size, frames=8, dst=d2, stride=None):
            arr = (ctypes.c_int * len(idx))(*idx)
            fsize = int(L.vp8hip_trace_wear_size(ctx.h, ctypes.byref(p)))
            return L.vp8hip_trace_wear_async(ctx.h, arr, len(idx) if n is None else n, ctypes.byref(p), ctypes.c_void_p(pool) if pool else None,
                                             pstride, frames, ctypes.c_void_p(dst) if dst else None, fsize if stride is None else stride)
        assert L.vp8hip_trace_wear_size(ctx.h, ctypes.byref(prm())) == 2 * 23 * 34
        assert L.vp8hip_trace_wear_size(ctx.h, ctypes.byref(prm(0, 0, 2, 15))) == 4 * h * w * 4
        assert tens([0, 1, 2], prm(), n=0) == -2 and tens([0, 1, 2], prm(), n=-1) == -2
        for bad in (-1, 8, 1 << 20):
            assert tens([0, bad], prm()) == -2, bad
        for frames in (0, -1):
            assert tens([0], prm(), frames=frames) == -2
        for dw, dh in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert tens([0, 1, 2], prm(dw, dh), stride=1 << 19) == -2, (dw, dh)
        for dt in (-1, 3):
            assert tens([0, 1, 2], prm(dtype=dt), stride=1 << 19) == -2
        for planes in (0, 16, 0x13, 1 << 31):                                          # no plane; bits that are no counter
            assert tens([0, 1, 2], prm(planes=planes), stride=1 << 19) == -2, planes
        for dtype, es in ((0, 1), (1, 2), (2, 4)):          # the destination, each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: tens([0, 1, 2][:n], prm(dtype=dtype), dst=dst, stride=stride), d2,
                                        2 * 23 * 34 * es, es)
        assert_destinations_refused(ctx, lambda n, dst, stride: tens([0, 1, 2][:n], prm(), pool=dst, pstride=stride, frames=n), d, size, 4)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                                       # nothing was enqueued
        # the same calls into memory the test owns are accepted: the destinations and nothing else are written
        assert wear([(0, 3, (0, 1, 2)), (1, 4, (0, -1, 2))]) == 0
        assert tens([4, 3, 4], prm()) == 0
        ctx.sync()
        a = big.cpu().numpy()
        fill = np.full((h, w), 0x5C5C5C5C, np.uint32)
        t3 = W.wear(hdrs[0], *irs[0], [fill] * 3)
        t4 = W.wear(hdrs[1], *irs[1], [fill, None, fill])
        assert hdrs[0].frame_type == 0 and hdrs[1].frame_type == 1 and not t3.any() and t4.any()
        assert a[3 * size:4 * size].tobytes() == t3.tobytes() and a[4 * size:5 * size].tobytes() == t4.tobytes()
        fsize = 2 * 23 * 34
        for k, t in enumerate((t4, t3, t4)):
            assert a[(1 << 21) + k * fsize:(1 << 21) + (k + 1) * fsize].tobytes() == W.tensor(t, 34, 23, 5).tobytes()
        assert (a[:3 * size] == 0x5C).all() and (a[5 * size:1 << 21] == 0x5C).all() and (a[(1 << 21) + 3 * fsize:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        pool = ctx.wear_pool(4)
        with pytest.raises(ValueError):
            ctx.frames_wear([(0, 0, None)], ctx.trace_pool(4))                         # a trace pool is no wear pool ...
        with pytest.raises(ValueError):
            ctx.frames_trace([(0, 0, None)], pool)                                     # ... nor the other way round
        with pytest.raises(ValueError):
            ctx.frames_wear([(0, 0, None)], torch.empty((4, h, w + 2, 4), dtype=torch.uint8, device="cuda:0")[:, :, :w])
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], width=34)
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], dtype=torch.int16)
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], planes=())
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], planes=("hops", "nope"))
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], planes=16)
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], dtype=torch.float32, scale=(1.0, 2.0))
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0], dtype=torch.float32, scale="pixels")
        with pytest.raises(ValueError):
            ctx.trace_wear(pool, [0, 1], 34, 23, out=torch.empty((2, 4, 23, 36), dtype=torch.uint8, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError):
            ctx.frames_wear([(3, 0, None)], pool)
        with pytest.raises(RuntimeError):
            ctx.frames_wear([(1, 0, (0, 1, 2))], pool)
        with pytest.raises(RuntimeError):
            ctx.trace_wear(pool, [4])
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the pool read on torch's stream: the wear is that of the frames that were there at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        irs = [slot_ir(ctx, i) for i in range(n)]
        rng = np.random.default_rng(4)
        given = [random_wear(rng, w, h) for _ in range(3)]
        pool = ctx.wear_pool(n + 3)
        for k in range(3):
            pool[n + k] = to_wear_pool(given[k])
        jobs = [(i, i, (n, n + 1, n + 2)) for i in range(n)]
        old = [W.wear(hdrs[i], *irs[i], given) for i in range(n)]
        ctx.frames_wear(jobs, pool)
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        got = wear_dwords(pool)                          # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(got[i], old[i]), i
        ctx.sync()
        # ... and the slots now hold the later frames
        changed = 0
        ctx.frames_wear(jobs, pool)
        got = wear_dwords(pool)
        for i in range(n):
            ir = slot_ir(ctx, i)
            want = W.wear(new_hdrs[i], *ir, given)
            assert np.array_equal(got[i], want), i
            changed += not np.array_equal(want, old[i])
        assert changed > 0
    finally:
        prod.close()


def test_float_types_on_every_counter_value(pkg):
    """a pool entry that holds every byte value in every counter, against scales that make the float land on ties of the halves (the
    half is the FLOAT rounded: two roundings), powers of two, negative ones, denormals and overflow"""
    P = pkg
    w, h = 64, 16                                        # 1024 pixels: every byte value four times, the counters out of step
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        a = np.arange(w * h).reshape(h, w)
        t = W.pack([a % 256, (a + 85) % 256, (a * 7) % 256, 255 - a % 256])
        assert all(set(np.unique(c).tolist()) == set(range(256)) for c in W.unpack(t))
        pool = ctx.wear_pool(2)
        pool[1] = to_wear_pool(t)
        check_tensor(ctx, pool, [1], [t], 0, 0, "u8", 15, None)
        differ = 0
        for s in ((1.8958333730697632, 1.3541666269302368, 1.8938802480697632, 1.8365886211395264), (1.0, 0.125, -1.0 / 3, 1e-3),
                  (1e-42, -3e-41, 2.0 ** -24, 65504.0 / 255), (3.0e4, 1e30, 1.0 / 255, 224 / 1920)):
            scale = tuple(np.float32(v) for v in s)
            for dtype in ("f32", "f16"):
                check_tensor(ctx, pool, [1], [t], 0, 0, dtype, 15, scale, what=s)
                check_tensor(ctx, pool, [1], [t], 33, 7, dtype, ("coded", "intra"), scale, what=s)
            with np.errstate(over="ignore"):
                once = (W.unpack(t).astype(np.float64) * np.asarray(scale, np.float64)[:, None, None]).astype(np.float16)
            differ += int((bits(once, "f16") != bits(W.tensor(t, dtype="f16", scale=scale), "f16")).sum())
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
        pool = ctx.wear_pool(4)
        jobs = []
        for data in frames[:2]:
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            jobs.append((0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx)))
            ctx.decode(jobs[-1:], P.STAGE_ALL)
            if len(jobs) == 1:
                ctx.frames_wear(jobs[-1:], pool)
            parser.swap(hdr)
        fb = jobs[-1][1]
        before_fb = ctx.download_full(fb)
        before = ctx.memory_usage()
        ctx.frames_wear(jobs[-1:], pool)
        for size in ({}, dict(width=224, height=224)):
            ctx.trace_wear(pool, [fb], dtype=torch.float32, scale=1.0 / 255, **size)
        ctx.sync()
        assert ctx.memory_usage() == before
        assert ctx.rgb_scratch_bytes() == 0
        assert np.array_equal(ctx.download_full(fb), before_fb)
        mbs, mvs = slot_ir(ctx, 0)
        assert hdr.frame_type == 1
        _, lst, gld, alt = jobs[-1][1], *jobs[-1][2]
        zero = np.zeros((h, w), np.uint32)
        assert lst == gld == alt == jobs[0][1]
        want = W.wear(hdr, mbs, mvs, [zero] * 3)
        assert np.array_equal(wear_dwords(pool[fb]), want) and np.array_equal(want, W.pack(W.incs(hdr, mbs, mvs)))
    finally:
        parser.close()
        ctx.close()
