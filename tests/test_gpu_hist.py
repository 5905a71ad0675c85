"""GPU (-m gpu): byte histograms in device memory (vp8hip_frames_hist_async, vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async,
vp8hip_trace_cover_hist_async; Vp8Hip.frames_hist, slots_hist, trace_wear_hist, trace_cover_hist; csrc/hip/vp8_hist.hip), count for
count against the numpy restatement (tests/hist_reference.py) applied to the planes vp8hip_frame_download gives, to the slot as
vp8hip_ir_fetch / vp8hip_ir_fetch_mvs read it back, and to the pool entries as they lie.  torch is imported here, before the package
loads libvpx's library: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import (Producer, assert_destinations_refused, assert_guards_intact, guarded, large_launch, later_writers_producer,
                              picture_into, two_key_frames_queued, write_later_frames)
import hist_reference as H
import side_reference as S
import trace_reference as R
import wear_reference as W
from trace_testlib import dwords, make_hdr, slot_ir, to_pool

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (17, 33), (67, 45), (130, 98), (8208, 16)]
FRAME_PLANE_SETS = [("y", "u", "v"), ("y",), ("u", "v"), 5, ("v",), 3]
SLOT_PLANE_SETS = [("ref", "mvmag"), 127, ("mode", "coded", "mvmag"), ("skip", "segment", "mvmag"), 64, ("mvmag", "qindex", "ref")]
WEAR_PLANE_SETS = [15, ("coded",), ("edge", "hops"), 14, ("intra",), 9]
COVER_PLANE_SETS = [3, ("seen",), ("count",)]


def counts(t):
    """a histogram tensor on the device -> numpy uint32"""
    assert t.dtype == torch.int32 and t.shape[-1] == 256
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("size", SIZES)
def test_pictures_from_raster(pkg, size):
    """uploaded frame buffers in the geom() layout at sizes whose widths are and are not multiples of 4 and 16, with odd chroma widths
    and pixel counts that are no multiple of 64 or 256 (8208x16: one macroblock row of 513): seeded noise, a ramp that holds every
    byte value a plane has room for, a flat picture -- every lane on one bin, the count still w * h exactly -- inside a border of
    other bytes, which must not be counted; single frames and pairs, the plane sets in rotation"""
    P = pkg
    sets = itertools.cycle(FRAME_PLANE_SETS)
    ctx = P.Vp8Hip(0)
    try:
        w, h = size
        ctx.configure(w, h, 5, 1)
        g = ctx.g
        cw, ch = (w + 1) // 2, (h + 1) // 2
        rng = np.random.default_rng(w * 131 + h)
        ramp = [(np.arange(ph * pw) * k % 256).astype(np.uint8).reshape(ph, pw) for k, (pw, ph) in ((1, (w, h)), (3, (cw, ch)), (7, (cw, ch)))]
        flat = [np.full((h, w), 37, np.uint8), np.full((ch, cw), 255, np.uint8), np.full((ch, cw), 0, np.uint8)]
        bufs = [rng.integers(0, 256, g.frame_size, dtype=np.uint8),
                picture_into(np.full(g.frame_size, 0x77, np.uint8), g, ramp),
                picture_into(np.full(g.frame_size, 200, np.uint8), g, flat),
                rng.integers(0, 256, g.frame_size, dtype=np.uint8)]
        for k, b in enumerate(bufs):
            ctx.upload_frame(k, b)
        planes = [ctx.download_planes(k) for k in range(4)]
        assert all(np.array_equal(a, b) for a, b in zip(planes[2], flat))
        assert all(np.unique(p).size == min(256, p.size) for p in planes[1])
        jobs = [0, 1, 2, 3, (0, 3), (3, 0), (1, 2), (2, 2), (2, None), (0, 1), 0, (3, 0)]
        for _ in range(3):
            which = next(sets)
            got = counts(ctx.frames_hist(jobs, which))
            mask = H.mask_of(which, H.FRAME_PLANES)
            assert got.shape == (len(jobs), bin(mask).count("1"), 256)
            for i, j in enumerate(jobs):
                fb, ref = (j, None) if isinstance(j, int) else j
                want = H.frames(planes[fb], None if ref is None else planes[ref], which)
                assert np.array_equal(got[i], want), (w, h, which, j)
                assert (got[i].sum(1) == [n for b, n in enumerate((w * h, cw * ch, cw * ch)) if mask >> b & 1]).all()
        got = counts(ctx.frames_hist([2, (2, 2), (0, 0)]))
        assert got[0, 0, 37] == w * h and got[0, 1, 255] == cw * ch and got[0, 2, 0] == cw * ch            # flat: exactly w * h in one bin
        assert (got[1:, :, 0] == [w * h, cw * ch, cw * ch]).all() and not got[1:, :, 1:].any()            # fb == ref_fb: all in bin 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_pictures_from_tiles(pkg, name, monkeypatch):
    """frames a large launch left as tiles, every one alone and in pairs -- tiles against tiles, tiles against an uploaded raster frame
    in both orders, a frame against itself --; no raster pool is made for them and the context's memory does not change.  Expected
    values from planes downloaded AFTER the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 6
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        before = ctx.memory_usage()
        w, h = ctx.width, ctx.height
        alone = ctx.frames_hist(list(range(n)))
        tiles = [(a, b) for a in range(n) for b in range(n) if (a + 2 * b) % 3 == 0]
        both = ctx.frames_hist(tiles, ("y", "v"))
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        rnd = np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                                             # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        before = ctx.memory_usage()
        mixed_jobs = [(k, n) for k in range(n)] + [(n, k) for k in range(n)] + [(n, n), n]
        mixed = ctx.frames_hist(mixed_jobs)
        ctx.sync()
        assert ctx.memory_usage() == before
        planes = [ctx.download_planes(k) for k in range(n + 1)]
        assert nsrc < 2 or not np.array_equal(planes[0][0], planes[1][0])
        got = counts(alone)
        for k in range(n):
            assert np.array_equal(got[k], H.frames(planes[k])), (name, k)
        got = counts(both)
        for i, (a, b) in enumerate(tiles):
            assert np.array_equal(got[i], H.frames(planes[a], planes[b], 5)), (name, a, b)
            if a == b:
                assert (got[i][:, 0] == [w * h, ((w + 1) // 2) * ((h + 1) // 2)]).all()
        got = counts(mixed)
        for i, j in enumerate(mixed_jobs):
            a, b = (j, None) if isinstance(j, int) else j
            assert np.array_equal(got[i], H.frames(planes[a], None if b is None else planes[b])), (name, j)
        assert np.array_equal(got[0], got[n])                                # |a - b| == |b - a|
    finally:
        ctx.close()


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98", "p_split_352x288", "p_seg_176x144"])
def test_slots_every_producer(pkg, name, how):
    """the first frames of a stream through slot 0 by every producer, also on a context whose slots have no block streams; the plane
    sets in rotation, always with MVMAG, and with QINDEX on the segmented fixture (segments with quantisers of their own in one
    frame: test_slots_random_ir_wild_vectors)"""
    P = pkg
    prod = Producer(P, name, how)
    ctx = prod.ctx
    sets = itertools.cycle(SLOT_PLANE_SETS)
    try:
        moved = 0
        for i in range(min(len(prod.frames), 7)):
            hdr = prod.put(i)
            which = next(sets)
            mask = H.mask_of(which, H.SLOT_PLANES) | (16 if name.startswith("p_seg") else 0)
            got = counts(ctx.slots_hist([0], mask))
            mbs, mvs = slot_ir(ctx, 0)
            want = H.slots(hdr, mbs, mvs, mask)
            assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), (name, how, i, mask)
            assert (got[0].sum(1) == 16 * ctx.nmb).all()
            moved += int(want[-1][1:].sum())
        assert moved > 0
    finally:
        prod.close()


def _random_ir(rng, nmb):
    """records of every y_mode and ref_frame (a few beyond 3), flags, segments, sub-block modes and eobs at random, vectors over all of
    int16 and on the ties of the rounding: like _random_ir of test_gpu_wear.py"""
    mbs = np.zeros((nmb, 64), np.uint8)
    mbs[:, S.O_Y_MODE] = rng.integers(0, 10, nmb)
    mbs[:, S.O_REF] = np.where(mbs[:, S.O_Y_MODE] < 5, 0, rng.integers(1, 4, nmb))
    wild = (mbs[:, S.O_REF] != 0) & (rng.random(nmb) < 0.1)
    mbs[wild, S.O_REF] = rng.integers(4, 256, int(wild.sum()))
    mbs[:, S.O_FLAGS] = rng.integers(0, 4, nmb)
    mbs[:, S.O_SEGMENT] = rng.integers(0, 4, nmb)
    mbs[:, 5] = rng.integers(0, 4, nmb)
    mbs[:, S.O_EOBS:S.O_EOBS + 25] = rng.choice(np.array([0, 0, 1, 1, 2, 16], np.uint8), (nmb, 25))
    mbs[:, S.O_B_MODES:S.O_B_MODES + 16] = rng.integers(0, 10, (nmb, 16))
    mvs = rng.integers(-32768, 32768, (nmb, 16, 2)).astype(np.int16)
    ties = rng.random((nmb, 16, 2)) < 0.4
    mvs[ties] = rng.choice(np.array([4, -4, 12, -12, 8, -8, 0, 3, -5, 2036, 2035, -2044, -32768, 32767], np.int16), int(ties.sum()))
    return mbs, mvs


@pytest.mark.parametrize("size", [(16, 16), (67, 45), (130, 98), (8208, 16)])
def test_slots_random_ir_wild_vectors(pkg, size):
    """random records with vectors over all of int16 and on the ties, ref_frame above 3, segments with quantisers of their own, an
    inter and a key header (the key frame's vectors are stale and not read): all seven planes, one call for both slots, twice"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 41 + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 2)
        coef = np.zeros((ctx.nmb, 400), np.int16)
        want = []
        for slot, ft in enumerate((1, 0)):
            hdr = make_hdr(P, w, h, ft)
            hdr.base_qindex, hdr.segmentation_enabled, hdr.mb_segment_abs_delta = 40, 1, slot
            for s, q in enumerate((-50, 3, 90, 127) if slot == 0 else (0, 17, 126, 64)):
                hdr.segment_quant[s] = q
            mbs, mvs = _random_ir(rng, ctx.nmb)
            ctx.fill_slot(slot, hdr, mbs, coef, mvs)
            ir = slot_ir(ctx, slot)
            assert np.array_equal(ir[0][:, :8], mbs[:, :8])
            want.append(H.slots(hdr, *ir, 127))
        assert want[1][6][0] == 16 * ctx.nmb and (ctx.nmb < 4 or want[0][6][255] > 0)
        assert ctx.nmb < 4 or len(np.nonzero(want[0][4])[0]) > 1
        first = counts(ctx.slots_hist([0, 1, 1, 0], 127))
        again = counts(ctx.slots_hist([0, 1, 1, 0], 127))
        for i, s in enumerate((0, 1, 1, 0)):
            assert np.array_equal(first[i], want[s]), (size, i)
        assert np.array_equal(first, again)
        got = counts(ctx.slots_hist([1, 0], ("coded", "mvmag", "mode")))
        assert np.array_equal(got[0], want[1][[1, 5, 6]]) and np.array_equal(got[1], want[0][[1, 5, 6]])
    finally:
        ctx.close()


def random_wear(rng, w, h):
    c = rng.integers(0, 256, (4, h, w))
    high = rng.random((4, h, w)) < 0.25
    c[high] = rng.integers(254, 256, int(high.sum()))
    return W.pack(c)


@pytest.mark.parametrize("size", [(64, 16)] + SIZES)
def test_pool_entries_at_offsets(pkg, size):
    """wear entries -- at 64x16 one that holds every byte value in every counter, as the wear test builds it, else seeded random
    counters -- and COUNT entries made by trace_invert of a constant trace (one count of w * h, which saturates, the rest 0) and of an
    identity trace, in pools at offsets 4 and 16 of their allocations with strides that are and are not multiples of 16"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 43 + h)
    ctx = P.Vp8Hip(0)
    wsets, csets = itertools.cycle(WEAR_PLANE_SETS), itertools.cycle(COVER_PLANE_SETS)
    try:
        ctx.configure(w, h, 1, 1)
        size_b = 4 * w * h
        a = np.arange(w * h).reshape(h, w)
        every = W.pack([a % 256, (a + 85) % 256, (a * 7) % 256, 255 - a % 256])
        given = [every if size == (64, 16) else random_wear(rng, w, h), random_wear(rng, w, h), np.zeros((h, w), np.uint32)]
        if size == (64, 16):
            assert all(set(np.unique(c).tolist()) == set(range(256)) for c in W.unpack(every))
        traces = ctx.trace_pool(2)
        traces[0] = to_pool(np.full((h, w), R.pack(w - 1, h // 2), np.uint32))
        traces[1] = to_pool(R.identity(w, h))
        for off, pad in ((4, 4), (16, 0), (16, 8), (4, 12)):
            big, flat = guarded(3, size_b, pad, off)
            pool = flat.unflatten(1, (h, w, 4))
            assert pool.data_ptr() % 16 == off % 16 and pool.stride(0) == size_b + pad
            for k in range(3):
                pool[k] = to_pool(given[k], np.uint8)
            idx = [0, 2, 1, 0]
            for which in (15, next(wsets)):
                got = counts(ctx.trace_wear_hist(pool, idx, which))
                for i, e in enumerate(idx):
                    assert np.array_equal(got[i], H.wear(given[e], which)), (size, off, pad, which, e)
                assert (got.sum(2) == w * h).all()
            assert np.array_equal(dwords(pool), np.stack(given))
            assert_guards_intact(big, 3, size_b, pad, off, what=(size, off, pad))
            cbig, cflat = guarded(2, size_b, pad, off, 0x3C)
            count = cflat.view(torch.int32).unflatten(1, (h, w))
            ctx.trace_invert(traces, [(0, 1), (1, 0)], count=count)
            held = dwords(count)
            assert held[1, h // 2, w - 1] == w * h and held[1].sum() == w * h and (held[0] == 1).all()
            for which in (3, next(csets)):
                got = counts(ctx.trace_cover_hist(count, [1, 0, 1], which))
                for i, e in enumerate((1, 0, 1)):
                    assert np.array_equal(got[i], H.cover(held[e], which)), (size, off, pad, which, e)
            got = counts(ctx.trace_cover_hist(count, [1, 0]))
            assert got[0, 0, 0] == w * h - 1 and got[0, 0, min(w * h, 255)] >= 1 and got[0, 1, 1] == 1 and not got[:, 1, 2:].any()
            assert got[1, 0, 1] == w * h and got[1, 1, 1] == w * h
            assert np.array_equal(dwords(count), held)
            assert_guards_intact(cbig, 2, size_b, pad, off, 0x3C, what=(size, off, pad))
    finally:
        ctx.close()


def test_batches_and_both_write_outs(pkg):
    """600 jobs in one call -- more than two launches' worth and a remainder, with repeats, several workgroups to a job -- for
    pictures, slots and wear entries at 352x288; one-job calls there (a job shared by workgroups, which add with atomics) and at
    16x16 (one workgroup owns the output and stores it); every call twice: the same bits"""
    P = pkg
    prod = Producer(P, "p_split_352x288", "host", nslots=4)
    ctx, w, h = prod.ctx, prod.w, prod.h
    pix = P.Vp8Hip(0)                                                        # (the pictures: a context with four frame buffers)
    try:
        rng = np.random.default_rng(600)
        hdrs = [prod.put(i, i) for i in range(4)]
        irs = [slot_ir(ctx, i) for i in range(4)]
        pix.configure(w, h, 4, 1)
        for k in range(4):
            pix.upload_frame(k, rng.integers(0, 256 if k < 3 else 2, pix.g.frame_size, dtype=np.uint8))
        planes = [pix.download_planes(k) for k in range(4)]
        n = 600
        fbs, refs = rng.integers(0, 4, n), rng.integers(-1, 4, n)
        jobs = [(int(a), int(b)) for a, b in zip(fbs, refs)]
        got = counts(pix.frames_hist(jobs))
        again = counts(pix.frames_hist(jobs))
        want = {j: H.frames(planes[j[0]], None if j[1] < 0 else planes[j[1]]) for j in set(jobs)}
        assert len(want) == 20
        for i, j in enumerate(jobs):
            assert np.array_equal(got[i], want[j]), (i, j)
        assert np.array_equal(got, again)
        slots = [int(s) for s in rng.integers(0, 4, n)]
        got = counts(ctx.slots_hist(slots, 127))
        swant = [H.slots(hdrs[s], *irs[s], 127) for s in range(4)]
        for i, s in enumerate(slots):
            assert np.array_equal(got[i], swant[s]), (i, s)
        assert np.array_equal(got, counts(ctx.slots_hist(slots, 127)))
        given = [random_wear(rng, w, h) for _ in range(3)]
        pool = ctx.wear_pool(3)
        for k in range(3):
            pool[k] = to_pool(given[k], np.uint8)
        idx = [int(s) for s in rng.integers(0, 3, n)]
        got = counts(ctx.trace_wear_hist(pool, idx, ("hops", "coded")))
        wwant = [H.wear(g, 9) for g in given]
        for i, e in enumerate(idx):
            assert np.array_equal(got[i], wwant[e]), (i, e)
        assert np.array_equal(got, counts(ctx.trace_wear_hist(pool, idx, 9)))
        # one job on the largest fixture: its rows are shared by several workgroups
        for j in ((0, -1), (3, -1), (1, 2)):
            one = counts(pix.frames_hist([j]))
            assert np.array_equal(one[0], want[j]) and np.array_equal(one, counts(pix.frames_hist([j])))
        assert np.array_equal(counts(ctx.slots_hist([2], 127))[0], swant[2])
        assert np.array_equal(counts(ctx.trace_wear_hist(pool, [1]))[0], H.wear(given[1]))
        cnt = torch.from_numpy(rng.choice(np.array([0, 1, 2, 255, 256, 70000], np.int32), (1, h, w))).to("cuda:0")
        assert np.array_equal(counts(ctx.trace_cover_hist(cnt, [0]))[0], H.cover(dwords(cnt)[0]))
    finally:
        pix.close()
        prod.close()
    # ... and the smallest: one workgroup owns each output
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(16, 16, 1, 1)
        buf = np.random.default_rng(16).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(0, buf)
        one = counts(ctx.frames_hist([0]))
        assert np.array_equal(one[0], H.frames(ctx.download_planes(0))) and np.array_equal(one, counts(ctx.frames_hist([0])))
    finally:
        ctx.close()


def test_guarded_destinations(pkg):
    """outputs at offsets 4 and 16 of their allocation, 0, 4 and 12 bytes apart: the counts, and the bytes around them"""
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host")
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        prod.put(0)
        hdr = prod.put(1)
        ir = slot_ir(ctx, 0)
        rng = np.random.default_rng(130)
        ctx.upload_frame(0, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        planes = ctx.download_planes(0)
        given = random_wear(rng, w, h)
        pool = ctx.wear_pool(1)
        pool[0] = to_pool(given, np.uint8)
        cnt = torch.from_numpy(rng.integers(0, 300, (1, h, w)).astype(np.int32)).to("cuda:0")
        calls = [(3, lambda out: ctx.frames_hist([0, (0, 0), 0], out=out), [H.frames(planes), H.frames(planes, planes), H.frames(planes)]),
                 (1, lambda out: ctx.frames_hist([0, 0, 0], ("u",), out=out), [H.frames(planes, None, 2)] * 3),
                 (7, lambda out: ctx.slots_hist([0, 0, 0], 127, out=out), [H.slots(hdr, *ir, 127)] * 3),
                 (2, lambda out: ctx.slots_hist([0, 0, 0], ("mvmag", "mode"), out=out), [H.slots(hdr, *ir, 66)] * 3),
                 (4, lambda out: ctx.trace_wear_hist(pool, [0, 0, 0], out=out), [H.wear(given)] * 3),
                 (1, lambda out: ctx.trace_cover_hist(cnt, [0, 0, 0], ("seen",), out=out), [H.cover(dwords(cnt)[0], 2)] * 3)]
        for (off, pad), (np_, call, want) in itertools.product(((4, 0), (16, 0), (4, 4), (16, 12), (4, 12), (16, 4)), calls):
            size = P.hist_size(np_)
            big, flat = guarded(3, size, pad, off)
            out = flat.view(torch.int32).unflatten(1, (np_, 256))
            assert call(out) is out
            got = counts(out)
            for k in range(3):
                assert np.array_equal(got[k], want[k]), (off, pad, np_, k)
            assert_guards_intact(big, 3, size, pad, off, what=(off, pad, np_))
    finally:
        prod.close()


def test_refusals(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host", nslots=3)
    ctx, w, h = prod.ctx, prod.w, prod.h
    L = ctx.L
    try:
        for i in range(2):
            prod.put(i, i)                               # slot 2 is never filled
        ctx.sync()
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        d2 = d + (1 << 21)
        assert d % 16 == 0
        esize = 4 * w * h
        assert 8 * esize < 1 << 21
        vp = ctypes.c_void_p

        def frames(jobs, planes=7, n=None, dst=d2, stride=None):
            arr = (P.HistJob * len(jobs))(*jobs)
            return L.vp8hip_frames_hist_async(ctx.h, arr, len(jobs) if n is None else n, planes, vp(dst) if dst else None,
                                              P.hist_size(bin(planes & 0xffffffff).count("1")) if stride is None else stride)

        def slots(s, planes=127, n=None, dst=d2, stride=None):
            arr = (ctypes.c_int * len(s))(*s)
            return L.vp8hip_slots_hist_async(ctx.h, arr, len(s) if n is None else n, planes, vp(dst) if dst else None,
                                             P.hist_size(bin(planes & 0xffffffff).count("1")) if stride is None else stride)

        def entries(fn, idx, planes=1, n=None, pool=d, pstride=esize, frames=8, dst=d2, stride=None):
            arr = (ctypes.c_int * len(idx))(*idx)
            return fn(ctx.h, arr, len(idx) if n is None else n, planes, vp(pool) if pool else None, pstride, frames, vp(dst) if dst else None,
                      P.hist_size(bin(planes & 0xffffffff).count("1")) if stride is None else stride)
        assert ctx.num_fb == 1
        assert frames([(0, -1)], n=0) == -2 and frames([(0, -1)], n=-1) == -2
        for bad in (-1, 1, 1 << 20):
            assert frames([(bad, -1)]) == -2 and frames([(0, -1), (bad, 0)]) == -2, bad
        for bad in (-2, 1, 1 << 20, -(1 << 31)):
            assert frames([(0, bad)]) == -2 and frames([(0, 0), (0, bad)]) == -2, bad
        for planes in (0, 8, 64, 0xf, 1 << 31):
            assert frames([(0, -1)], planes, stride=4096) == -2, planes
        assert slots([0], n=0) == -2 and slots([0], n=-1) == -2
        for bad in (-1, 3, 1 << 20, 2):                  # out of range; never filled
            assert slots([bad]) == -2 and slots([0, bad]) == -2, bad
        for planes in (0, 128, 0x1ff, 1 << 31):
            assert slots([0], planes, stride=8192) == -2, planes
        assert L.vp8hip_frames_side_async(ctx.h, (ctypes.c_int * 1)(0), 1, ctypes.byref(P.SideParams(0, 0, 0, 64)), None, 0, vp(d2), 1 << 20) == -2
        for fn, unknown in ((L.vp8hip_trace_wear_hist_async, 16), (L.vp8hip_trace_cover_hist_async, 4)):
            assert entries(fn, [0], n=0) == -2 and entries(fn, [0], n=-1) == -2
            for bad in (-1, 8, 1 << 20):
                assert entries(fn, [bad]) == -2 and entries(fn, [0, bad]) == -2, bad
            for planes in (0, unknown, unknown | 1, 1 << 31):
                assert entries(fn, [0], planes, stride=4096) == -2, planes
            for fr in (0, -1):
                assert entries(fn, [0], frames=fr) == -2
            # the pool, as vp8hip_trace_flow_async refuses it (three entries and one)
            assert_destinations_refused(ctx, lambda n, p, s: entries(fn, [0, 1, 2][:n], pool=p, pstride=s, frames=n), d, esize, 4)
            # the destination
            assert_destinations_refused(ctx, lambda n, p, s: entries(fn, [0, 1, 2][:n], dst=p, stride=s), d2, 1024, 4)
            # ... overlapping the pool: inside it, straddling its end, around it
            assert entries(fn, [0, 1], dst=d + 4 * esize, stride=1024) == -2
            assert entries(fn, [0, 1], dst=d + 8 * esize - 1024, stride=1024) == -2
            assert entries(fn, [0, 1], frames=1, pool=d + esize, dst=d, stride=2 * esize) == -2
            assert entries(fn, [0, 1], dst=d + 8 * esize, stride=1024) == 0                 # (right behind the pool: accepted)
        assert_destinations_refused(ctx, lambda n, p, s: frames([(0, -1)] * n, dst=p, stride=s), d2, 3072, 4)
        assert_destinations_refused(ctx, lambda n, p, s: slots([0] * n, dst=p, stride=s), d2, 7168, 4)
        assert frames([(0, -1)], 1, stride=1020) == -2 and frames([(0, -1)], 7, stride=3068) == -2          # a stride below the size
        assert frames([(0, -1)], 1, dst=d2 + 2) == -2 and frames([(0, -1), (0, -1)], 1, stride=1026) == -2   # not a multiple of 4
        ctx.sync()
        torch.cuda.synchronize()
        a = big.cpu().numpy()
        assert (a[:8 * esize] == 0x5C).all() and (a[8 * esize + 2048:] == 0x5C).all()      # nothing was enqueued but the two accepted calls
        # the same calls into memory the test owns are accepted
        assert frames([(0, -1), (0, 0)]) == 0 and slots([1, 0]) == 0
        ctx.sync()
        # the Python wrappers refuse what they can see before the call, and raise the library's refusals
        pool = ctx.wear_pool(2)
        for call in (lambda: ctx.frames_hist([0], ("y", "nope")), lambda: ctx.frames_hist([]), lambda: ctx.slots_hist([0], ()),
                     lambda: ctx.slots_hist([0], 128), lambda: ctx.trace_wear_hist(pool, [0], 16), lambda: ctx.trace_wear_hist(pool, [2]),
                     lambda: ctx.trace_wear_hist(ctx.trace_pool(2), [0]), lambda: ctx.trace_cover_hist(pool, [0]),
                     lambda: ctx.frames_hist([0], out=torch.empty((1, 3, 256), dtype=torch.int64, device="cuda:0")),
                     lambda: ctx.frames_hist([0], out=torch.empty((1, 3, 512), dtype=torch.int32, device="cuda:0")[:, :, ::2])):
            with pytest.raises(ValueError):
                call()
        for call in (lambda: ctx.frames_hist([1]), lambda: ctx.frames_hist([(0, 5)]), lambda: ctx.slots_hist([2], 1),
                     lambda: ctx.trace_wear_hist(pool, [0], out=pool.view(torch.int32).flatten()[:1024].view(1, 4, 256))):
            with pytest.raises(RuntimeError):
                call()
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the histograms read on torch's stream: they are those of the frames that were there at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx = prod.ctx
    try:
        old = [H.slots(hdrs[i], *slot_ir(ctx, i), 127) for i in range(n)]
        out = ctx.slots_hist(list(range(n)), 127)
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        got = counts(out)                                # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(got[i], old[i]), i
        ctx.sync()
        got = counts(ctx.slots_hist(list(range(n)), 127))
        changed = 0
        for i in range(n):
            want = H.slots(new_hdrs[i], *slot_ir(ctx, i), 127)
            assert np.array_equal(got[i], want), i
            changed += not np.array_equal(want, old[i])
        assert changed > 0
    finally:
        prod.close()


def test_ordering_against_a_decode_into_the_same_frame_buffer(pkg):
    """frames_hist, then at once a decode of another frame into the same frame buffer: the histogram is that of the picture that was
    there at the call; and an earlier decode is seen without a sync"""
    P = pkg
    ctx, parser = two_key_frames_queued(P)
    try:
        w, h = ctx.width, ctx.height
        out = ctx.frames_hist([0, (0, 1)])               # behind the decode of frame 0 ...
        ctx.decode([(1, 0, None)], P.STAGE_ALL)          # ... and in front of the decode of frame 1 into the same frame buffer
        got = counts(out)
        after = counts(ctx.frames_hist([0, (0, 1)]))
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        planes0, planes1 = ctx.download_planes(0), ctx.download_planes(1)
        first, second = H.frames(planes0), H.frames(planes1)         # (frame buffer 1 holds frame 1 throughout)
        assert not np.array_equal(first, second)
        assert np.array_equal(got[0], first) and np.array_equal(got[1], H.frames(planes0, planes1))
        assert np.array_equal(after[0], second) and after[1, 0, 0] == w * h and not after[1, :, 1:].any()
    finally:
        parser.close()
        ctx.close()


def test_no_new_device_memory_and_sources_untouched(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host")
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        prod.put(0)
        prod.put(1)
        rng = np.random.default_rng(98)
        buf = rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(0, buf)
        given = [random_wear(rng, w, h), rng.integers(0, 400, (h, w)).astype(np.uint32)]
        pool = ctx.wear_pool(1)
        pool[0] = to_pool(given[0], np.uint8)
        cnt = to_pool(given[1], np.int32)[None]
        ir = slot_ir(ctx, 0)
        ctx.sync()
        torch.cuda.synchronize()
        before = ctx.memory_usage()
        reserved = torch.cuda.memory_allocated()
        outs = [torch.empty((2, k, 256), dtype=torch.int32, device="cuda:0") for k in (3, 7, 4, 2)]
        reserved = torch.cuda.memory_allocated()
        ctx.frames_hist([0, (0, 0)], out=outs[0])
        ctx.slots_hist([0, 0], 127, out=outs[1])
        ctx.trace_wear_hist(pool, [0, 0], out=outs[2])
        ctx.trace_cover_hist(cnt, [0, 0], out=outs[3])
        ctx.sync()
        assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        assert np.array_equal(ctx.download_full(0), buf)
        assert np.array_equal(dwords(pool)[0], given[0]) and np.array_equal(dwords(cnt)[0], given[1])
        again = slot_ir(ctx, 0)
        assert np.array_equal(again[0], ir[0]) and np.array_equal(again[1], ir[1])
    finally:
        prod.close()


def test_pair_refusal_texts(pkg):
    """What vp8hip_last_error says after each refusal of the three calls over picture pairs (vp8hip_frames_hist_async, _ssim_async,
    _motion_async), and, by two faults at once, which check comes first: the texts the library gave before the three calls shared
    their host path.  48x32 with two frame buffers -- 3 x 2 macroblocks, the smallest size at which every check is reachable;
    every call here is refused and nothing is enqueued.  (The alignment refusal prints a pointer and is left out.)"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        L, vp = ctx.L, ctypes.c_void_p
        mem = torch.empty((4096,), dtype=torch.uint8, device="cuda:0")
        d = mem.data_ptr()
        assert d % 16 == 0 and P.hist_size(3) == 3072 and P.ssim_sizes(48, 32, 7, 2) == (48, 304) and P.motion_sizes(3, 2, 31) == (24, 120)

        def hist(job=(0, 1), n=1, planes=7, stride=3072):
            return L.vp8hip_frames_hist_async(ctx.h, (P.HistJob * 1)(job), n, planes, vp(d), stride)

        def ssim(job=(0, 1), n=1, planes=7, sc=d, ss=48, mp=d + 1024, ms=304):
            return L.vp8hip_frames_ssim_async(ctx.h, (P.HistJob * 1)(job), n, ctypes.byref(P.SsimParams(planes, 2)), vp(sc), ss, vp(mp), ms)

        def motion(job=(0, 1), n=1, planes=31, mv=d, ms=24, st=d + 1024, ss=120, cen=None, cs=24):
            return L.vp8hip_frames_motion_async(ctx.h, (P.HistJob * 1)(job), n, ctypes.byref(P.MotionParams(4, 0, planes, None)),
                                                vp(cen) if cen else None, cs, vp(mv) if mv else None, ms, vp(st) if st else None, ss)
        params = "distance 4 (1..64), sad_per_bit 0 (0..255), planes 0x20 (of 0x1f)"
        cases = [(hist, "vp8hip_frames_hist_async", [
                      (dict(job=(0, -1), planes=0), ": planes 0x0 (at least one of 0x7)"),          # ref_fb -1: none, accepted
                      (dict(planes=0), ": planes 0x0 (at least one of 0x7)"),
                      (dict(planes=8), ": planes 0x8 (at least one of 0x7)"),
                      (dict(stride=3068), " (dst): stride 3068 below the frame's 3072 bytes"),
                      (dict(job=(5, 7), planes=8), ": frame buffer 5 out of range"),
                      (dict(planes=0xf, stride=3068), ": planes 0xf (at least one of 0x7)")]),
                 (ssim, "vp8hip_frames_ssim_async", [
                      (dict(job=(0, -1)), ": frame buffer -1 out of range"),
                      (dict(planes=0), ": planes 0x0 (at least one of 0x7)"),
                      (dict(planes=8), ": planes 0x8 (at least one of 0x7)"),
                      (dict(ss=40), " (scores): stride 40 below the frame's 48 bytes"),
                      (dict(ms=300), " (map): stride 300 below the frame's 304 bytes"),
                      (dict(mp=d + 16), ": scores and map overlap"),
                      (dict(job=(5, 7), planes=8), ": frame buffer 5 out of range"),
                      (dict(planes=0xf, ss=40), ": planes 0xf (at least one of 0x7)")]),
                 (motion, "vp8hip_frames_motion_async", [
                      (dict(job=(0, -1)), ": frame buffer -1 out of range"),
                      (dict(planes=0), ": stats without planes"),
                      (dict(planes=32), ": " + params),
                      (dict(ms=22), " (mv): stride 22 below the frame's 24 bytes"),
                      (dict(ss=116), " (stats): stride 116 below the frame's 120 bytes"),
                      (dict(cen=d + 2048, cs=22), " (centre): stride 22 below the frame's 24 bytes"),
                      (dict(st=d + 8), ": mv and stats overlap"),
                      (dict(cen=d + 2), ": mv and centre overlap"),
                      (dict(cen=d + 1028), ": stats and centre overlap"),
                      (dict(job=(5, 7), planes=32), ": frame buffer 5 out of range"),
                      (dict(planes=32, ms=22), ": " + params)])]
        for call, who, own in cases:
            shared = [(dict(n=0), ": bad arguments"), (dict(job=(2, 0)), ": frame buffer 2 out of range"), (dict(job=(0, 3)), ": frame buffer 3 out of range"),
                      (dict(job=(0, -2)), ": frame buffer -2 out of range"), (dict(job=(-1, 0)), ": frame buffer -1 out of range")]
            for kw, text in shared + own:
                assert call(**kw) == -2, (who, kw)
                assert L.vp8hip_last_error(ctx.h).decode() == who + text, (who, kw)
    finally:
        ctx.close()
