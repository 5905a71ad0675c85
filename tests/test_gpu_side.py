"""GPU (-m gpu): motion vectors and macroblock modes of IR slots as tensors in device memory (vp8hip_frames_side_async,
Vp8Hip.frames_side; csrc/hip/vp8_side.hip), bit for bit against the numpy restatement (tests/side_reference.py) applied to the
slot as vp8hip_ir_fetch / vp8hip_ir_fetch_mvs read it back, for slots written by the host parser and by the device's entropy
decoder.  torch is imported here, before the package loads libvp8hip.so: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path
from handover_testlib import (BITS, TORCH_DTYPE, Producer, assert_destinations_refused, assert_guards_intact, bits, equal_on_device, guarded,
                              later_writers_producer, write_later_frames)
import side_reference as R

pytestmark = pytest.mark.gpu

STREAMS = ["p_split_352x288", "p_arf_176x144", "p_seg_176x144", "p_roi_640x360", "p_odd_130x98", "kf_640x360", "kf_odd_67x45", "p_1920x1080"]
MASKS = [63, 7, 0b101010, 16, 1, 0b110100, 32]
SCALES = [(1.0, 1.0), (0.125, 0.125), (-1.0 / 3, 1e-3), (3.0e4, 2.0 ** -20)]


def call(ctx, slots, dw, dh, dtype="i16", planes=63, scale=None, **kw):
    size = {} if dw == 0 else dict(width=dw, height=dh)
    return ctx.frames_side(slots, mv_dtype=TORCH_DTYPE[dtype], planes=planes, scale=scale, **size, **kw)


def slot_ir(ctx, slot):
    mbs, _ = ctx.ir_fetch(slot)
    return mbs, ctx.mvs_fetch(slot)


def check(ctx, slot, hdr, ir, dw, dh, dtype="i16", planes=63, scale=None, what=None, **kw):
    """one slot through the call against the reference on what the slot holds (ir = slot_ir)"""
    mv, info = call(ctx, [slot], dw, dh, dtype, planes, scale, **kw)
    want_mv, want_info = R.side(hdr, ir[0], ir[1], dw, dh, dtype, planes, scale if scale is not None else (1.0, 1.0))
    if kw.get("out_mv", None) is False:
        assert mv is None
    else:
        got = mv.cpu().numpy()[0]
        assert got.shape == want_mv.shape and np.array_equal(bits(got, dtype), bits(want_mv, dtype)), (what, "mv", dw, dh, dtype, planes, scale)
    if kw.get("out_info", None) is False or planes == 0:
        assert info is None
    else:
        got = info.cpu().numpy()[0]
        assert got.shape == want_info.shape and np.array_equal(got, want_info), (what, "info", dw, dh, planes)


def _targets(w, h, rng):
    c = [(224, 224), (1, 1), (w + 1, max(1, h - 1)), (max(1, w // 2 + 1), max(1, h // 3)), (2 * w + 3, 2 * h), (max(1, w // 9), 3 * h + 2), (w, max(1, h // 2)),
         (4 * ((w + 15) // 16), 4 * ((h + 15) // 16))]
    c += [(int(rng.integers(1, 2 * w + 2)), int(rng.integers(1, 2 * h + 2))) for _ in range(3)]
    return c


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", STREAMS)
def test_slot_producers(pkg, name, how):
    """every frame of the fixture: the native grid and the display size with every plane; a sweep of sizes (224x224, widths that are
    no multiple of 4, 1x1, seeded random ones), the three types, plane masks, mv-only and info-only calls in rotation"""
    P = pkg
    prod = Producer(P, name, how)
    ctx, w, h = prod.ctx, prod.w, prod.h
    rng = np.random.default_rng(2026)
    sweep = itertools.cycle(itertools.product(_targets(w, h, rng), ("f32", "i16", "f16")))
    masks, scales = itertools.cycle(MASKS), itertools.cycle(SCALES)
    n_inter = 0
    try:
        nmb = ((w + 15) // 16) * ((h + 15) // 16)
        assert ctx.L.vp8hip_side_mv_size(ctx.h, ctypes.byref(P.SideParams(0, 0, 2, 3))) == 2 * 16 * nmb * 4
        assert ctx.L.vp8hip_side_info_size(ctx.h, ctypes.byref(P.SideParams(0, 0, 2, 3))) == 2 * 16 * nmb
        for i in range(len(prod.frames)):
            hdr = prod.put(i)
            n_inter += hdr.frame_type != 0
            ir = slot_ir(ctx, 0)
            what = (name, how, i)
            check(ctx, 0, hdr, ir, 0, 0, "i16", 63, what=what)
            sc = R.pixel_scale(hdr, w, h)
            assert sc == (np.float32(0.125), np.float32(0.125))
            check(ctx, 0, hdr, ir, w, h, ("f32", "f16", "i16")[i % 3], 63, scale=sc, what=what)
            for _ in range(3 if i < 6 else 1):
                (dw, dh), dtype = next(sweep)
                check(ctx, 0, hdr, ir, dw, dh, dtype, next(masks), scale=next(scales), what=what)
            if i < 4:
                check(ctx, 0, hdr, ir, *next(sweep)[0], "f16", 0, scale=(0.5, 2.0), what=what)                 # mv only: no planes
                check(ctx, 0, hdr, ir, *next(sweep)[0], "i16", 0b1001, what=what, out_info=False)             # mv only: planes not asked for
                check(ctx, 0, hdr, ir, *next(sweep)[0], "i16", 0b111000, what=what, out_mv=False)             # info only
        if name.startswith("p_"):
            assert n_inter > 0
    finally:
        prod.close()


def test_scale_pixels_convenience(pkg):
    """scale="pixels": 0.125 * dst / display, in double, rounded to float once -- the flow in pixels of the tensor"""
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host")
    try:
        hdr = prod.put(0)
        hdr = prod.put(1)
        ir = slot_ir(prod.ctx, 0)
        assert hdr.frame_type == 1 and ir[1].any()
        for dw, dh in ((224, 224), (130, 98), (65, 200), (0, 0)):
            sc = R.pixel_scale(hdr, dw, dh)
            for dtype in ("f32", "f16"):
                mv, _ = call(prod.ctx, [0], dw, dh, dtype, 0, "pixels")
                want, _ = R.side(hdr, ir[0], ir[1], dw, dh, dtype, 0, sc)
                assert np.array_equal(bits(mv.cpu().numpy()[0], dtype), bits(want, dtype)), (dw, dh, dtype)
    finally:
        prod.close()


def _random_ir(rng, nmb):
    mbs = np.zeros((nmb, 64), np.uint8)
    mbs[:, R.O_Y_MODE] = rng.integers(0, 10, nmb)
    mbs[:, R.O_REF] = np.where(mbs[:, R.O_Y_MODE] < 5, 0, rng.integers(1, 4, nmb))
    mbs[:, R.O_FLAGS] = rng.integers(0, 4, nmb)
    mbs[:, R.O_SEGMENT] = rng.integers(0, 4, nmb)
    mbs[:, 5] = rng.integers(0, 4, nmb)
    mbs[:, R.O_EOBS:R.O_EOBS + 25] = rng.integers(0, 17, (nmb, 25)) * (rng.integers(0, 3, (nmb, 25)) > 0)
    mbs[:, R.O_B_MODES:R.O_B_MODES + 16] = rng.integers(0, 10, (nmb, 16))
    mvs = rng.integers(-32768, 32768, (nmb, 16, 2)).astype(np.int16)
    return mbs, mvs


@pytest.mark.parametrize("size", [(16, 16), (67, 45), (640, 360), (6200, 40), (9000, 33), (16383, 16)])
def test_hand_built_slots(pkg, size):
    """random macroblocks (every mode, reference, partitioning, kind, segment; vectors over the whole int16 range) uploaded from
    the dense view, with absolute and delta segment quantisers that clamp at both ends -- also for frames so wide that a workgroup
    stages one macroblock row (over 8192: more than 64 KB of LDS)"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 31 + h)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 2)
        nmb = ctx.nmb
        coef = np.zeros((nmb, 400), np.int16)
        for slot, (ft, seg_on, abs_delta, base, sq) in enumerate(((1, 1, 0, 100, (-128, 40, 0, -7)), (0, 1, 1, 9, (127, -3, 64, 0)))):
            hdr = P.FrameHdr()
            hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows, hdr.frame_type = w, h, (w + 15) // 16, (h + 15) // 16, ft
            hdr.segmentation_enabled, hdr.mb_segment_abs_delta, hdr.base_qindex = seg_on, abs_delta, base
            for s in range(4):
                hdr.segment_quant[s] = sq[s]
            mbs, mvs = _random_ir(rng, nmb)
            ctx.fill_slot(slot, hdr, mbs, coef, mvs)
            ir = slot_ir(ctx, slot)
            assert np.array_equal(ir[0][:, :56], mbs[:, :56])
            for (dw, dh), dtype, planes in (((0, 0), "i16", 63), ((w, h), "f32", 63), ((224, 224), "f16", 0b110011), ((min(w + 1, 16383), 2 * h + 1), "i16", 63),
                                            ((max(1, w // 5), 7), "f32", 0b11100)):
                check(ctx, slot, hdr, ir, dw, dh, dtype, planes, scale=(0.125, -0.125), what=(size, slot))
    finally:
        ctx.close()


def test_float_types_on_every_int16(pkg):
    """every int16 as a vector component, both channels, against scales that make the float land on ties of the halves (the half
    is the FLOAT rounded: two roundings), powers of two, negative ones and ones so small that the floats are denormal"""
    P = pkg
    w, h = 1024, 1024                                   # 4096 macroblocks: 65536 vectors
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        nmb = ctx.nmb
        hdr = P.FrameHdr()
        hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows, hdr.frame_type = w, h, w // 16, h // 16, 1
        mbs = np.zeros((nmb, 64), np.uint8)
        mbs[:, R.O_Y_MODE], mbs[:, R.O_REF] = 9, 1
        v = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
        mvs = np.stack([v, v[::-1]], 1).reshape(nmb, 16, 2).copy()
        ctx.fill_slot(0, hdr, mbs, np.zeros((nmb, 400), np.int16), mvs)
        ir = slot_ir(ctx, 0)
        assert np.array_equal(ir[1].reshape(mvs.shape), mvs)
        differ = 0
        for sx, sy in ((1.0285249948501587, 1.9014227390289307), (0.2968776226043701, 0.6305446028709412), (1.0, 0.125), (-1.0 / 3, 1e-3),
                       (1e-42, -3e-41), (2.0 ** -24, 65504.0 / 32767), (3.0e4, 1e30), (0.125 * 224 / 1920, 0.125 * 224 / 1080)):
            scale = (np.float32(sx), np.float32(sy))
            for dtype in ("f32", "f16"):
                check(ctx, 0, hdr, ir, 0, 0, dtype, 0, scale=scale, what=(sx, sy))
            with np.errstate(over="ignore"):
                once = (mvs[:, :, 1].astype(np.float64) * np.float64(scale[0])).astype(np.float16)
            differ += int((once != R.convert(np.stack([mvs[:, :, 1], mvs[:, :, 0]]), "f16", scale)[0]).sum())
        assert differ > 0                               # (the sweep holds values one rounding would get wrong)
    finally:
        ctx.close()


def test_stale_vector_area_of_a_key_frame(pkg):
    """a key frame uploaded into a slot that held an inter frame: the slot's vector area still holds that frame's vectors"""
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host")
    ctx = prod.ctx
    try:
        prod.put(0)
        hdr = prod.put(1)
        assert hdr.frame_type == 1
        again = P.Parser()
        try:
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(again, prod.frames[0], 0)
        finally:
            again.close()
        assert hdr.frame_type == 0
        ir = slot_ir(ctx, 0)
        assert ir[1].any()                              # stale
        for dw, dh, dtype in ((0, 0, "i16"), (130, 98, "f32"), (224, 224, "f16"), (131, 50, "i16")):
            mv, info = call(ctx, [0], dw, dh, dtype, 1, (2.0, 2.0))
            assert not mv.cpu().numpy().view(BITS[dtype]).any()
            assert not info.cpu().numpy().any()         # REF: all intra
            check(ctx, 0, hdr, ir, dw, dh, dtype, 63, scale=(2.0, 2.0))
    finally:
        prod.close()


def test_batch_of_4096_slots(pkg):
    """4096 slots in one call (sixteen launches), a shuffled list with repeats, a list a little longer than one launch carries"""
    P = pkg
    n = 4096
    prod = Producer(P, "p_arf_176x144", "host", nslots=n)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        nsrc = 24
        hdrs = [prod.put(i, i) for i in range(nsrc)]
        irs = [slot_ir(ctx, i) for i in range(nsrc)]
        for i in range(nsrc, n):
            ctx.ir_copy(i, i % nsrc)
        rng = np.random.default_rng(5)
        for (dw, dh), dtype, planes in (((w, h), "f32", 0b100011), ((0, 0), "i16", 63), ((97, 55), "f16", 0b10000)):
            refs = [R.side(hdrs[k], irs[k][0], irs[k][1], dw, dh, dtype, planes, (0.125, 0.125)) for k in range(nsrc)]
            for slots in (list(range(n)), [int(s) for s in rng.integers(0, n, 700)], list(range(300, 300 + 257))):
                mv, info = call(ctx, slots, dw, dh, dtype, planes, (0.125, 0.125))
                which = [s % nsrc for s in slots]
                assert mv.shape[0] == len(slots) and info.shape[0] == len(slots)
                assert equal_on_device(mv, [r[0] for r in refs], which, dtype) == [], (dw, dh, dtype, len(slots))
                assert equal_on_device(info, [r[1] for r in refs], which, "u8") == [], (dw, dh, planes, len(slots))
                del mv, info
    finally:
        prod.close()


def test_destination_hygiene(pkg):
    """tensors at odd addresses with padded frame strides (info: any byte; vectors: aligned to the element but not to the piece) and
    aligned ones (whole-piece stores where the width allows): the sentinel bytes before, between and behind the frames stay"""
    P = pkg
    n = 3
    prod = Producer(P, "p_odd_130x98", "host", nslots=n)
    ctx = prod.ctx
    try:
        prod.put(0)
        hdrs = [prod.put(i + 1, i) for i in range(n)]   # inter frames
        irs = [slot_ir(ctx, i) for i in range(n)]
        assert all(h.frame_type == 1 for h in hdrs) and all(ir[1].any() for ir in irs)
        slots = [2, 0, 1]
        for (dw, dh), dtype, planes, (off, pad) in itertools.product(((130, 98), (64, 36), (0, 0), (33, 17)), ("i16", "f16", "f32"), (63, 0b100),
                                                                     ((0, 0), (3, 37), (2, 6), (4, 4), (8, 24), (16, 16))):
            gw, gh = (dw, dh) if dw else (4 * hdrs[0].mb_cols, 4 * hdrs[0].mb_rows)
            es = 4 if dtype == "f32" else 2
            nc = bin(planes).count("1")
            msize, isize = 2 * gh * gw * es, nc * gh * gw
            moff, mpad = off // es * es, pad // es * es                     # (the call refuses vectors not aligned to their element)
            (mbig, mflat), (ibig, iflat) = guarded(n, msize, mpad, moff), guarded(n, isize, pad, off, 0x5A)
            out_mv, out_info = mflat.view(TORCH_DTYPE[dtype]).unflatten(1, (2, gh, gw)), iflat.unflatten(1, (nc, gh, gw))
            assert out_mv.data_ptr() % 16 == moff % 16 and out_info.data_ptr() % 16 == off % 16
            mv, info = call(ctx, slots, dw, dh, dtype, planes, (0.25, 0.5), out_mv=out_mv, out_info=out_info)
            assert mv.data_ptr() == out_mv.data_ptr() and info.data_ptr() == out_info.data_ptr()
            gm, gi = out_mv.cpu().numpy(), out_info.cpu().numpy()
            for k, s in enumerate(slots):
                wm, wi = R.side(hdrs[s], irs[s][0], irs[s][1], dw, dh, dtype, planes, (0.25, 0.5))
                assert np.array_equal(bits(gm[k], dtype), bits(wm, dtype)) and np.array_equal(gi[k], wi), (dw, dh, dtype, planes, off, pad, k)
            assert_guards_intact(mbig, n, msize, mpad, moff, what=(dw, dh, dtype, planes, off, pad))
            assert_guards_intact(ibig, n, isize, pad, off, 0x5A, what=(dw, dh, dtype, planes, off, pad))
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the tensors read on torch's stream: they hold what the slots held at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        irs = [slot_ir(ctx, i) for i in range(n)]
        old = [R.side(hdrs[i], irs[i][0], irs[i][1], w, h, "f32", 63, (0.125, 0.125)) for i in range(n)]
        mv, info = call(ctx, list(range(n)), w, h, "f32", 63, (0.125, 0.125))
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        gm, gi = mv.cpu().numpy(), info.cpu().numpy()   # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(bits(gm[i], "f32"), bits(old[i][0], "f32")) and np.array_equal(gi[i], old[i][1]), i
        ctx.sync()
        # ... and the slots now hold the later frames
        changed = 0
        for i in range(n):
            ir = slot_ir(ctx, i)
            check(ctx, i, new_hdrs[i], ir, w, h, "f32", 63, scale=(0.125, 0.125))
            changed += not np.array_equal(ir[1], irs[i][1])
        assert changed > 0
    finally:
        prod.close()


def test_refusals(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host", nslots=4)
    ctx = prod.ctx
    L = ctx.L
    try:
        hdrs = [prod.put(i, i) for i in range(3)]       # slot 3 is never filled
        irs = [slot_ir(ctx, i) for i in range(3)]
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        d2 = d + (1 << 21)
        assert d % 16 == 0
        slots = (ctypes.c_int * 3)(0, 1, 2)

        def prm(w=34, h=23, dtype=0, planes=3):
            return P.SideParams(w, h, dtype, planes)

        def run(arr, n, p, mv, ms, info, istride):
            return L.vp8hip_frames_side_async(ctx.h, arr, n, ctypes.byref(p), ctypes.c_void_p(mv) if mv else None, ms,
                                              ctypes.c_void_p(info) if info else None, istride)
        msize, isize = 2 * 34 * 23 * 2, 2 * 34 * 23
        assert L.vp8hip_side_mv_size(ctx.h, ctypes.byref(prm())) == msize and L.vp8hip_side_info_size(ctx.h, ctypes.byref(prm())) == isize
        assert run(slots, 0, prm(), d, msize, d2, isize) == -2
        assert run(slots, -1, prm(), d, msize, d2, isize) == -2
        for bad in (-1, 4, 1 << 20):
            assert run((ctypes.c_int * 1)(bad), 1, prm(), d, msize, d2, isize) == -2, bad
        assert run((ctypes.c_int * 1)(3), 1, prm(), d, msize, d2, isize) == -2        # never filled
        assert run((ctypes.c_int * 2)(0, 3), 2, prm(), d, msize, d2, isize) == -2
        for w, h in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert run(slots, 3, prm(w, h), d, 1 << 19, d2, 1 << 19) == -2, (w, h)
        for dt in (-1, 3):
            assert run(slots, 3, prm(dtype=dt), d, 1 << 19, d2, 1 << 19) == -2
        for planes in (64, 0x80000001, 0xffffffff):
            assert run(slots, 3, prm(planes=planes), d, 1 << 19, d2, 1 << 19) == -2
        assert run(slots, 3, prm(planes=0), d, msize, d2, isize) == -2                 # an info tensor of no planes
        assert run(slots, 3, prm(), None, 0, None, 0) == -2                            # neither destination
        for dtype, es in ((0, 2), (1, 2), (2, 4)):          # the vectors alone, each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: run(slots, n, prm(dtype=dtype), dst, stride, None, 0), d, msize * es // 2, es)
        assert_destinations_refused(ctx, lambda n, dst, stride: run(slots, n, prm(), None, 0, dst, stride), d2, isize, 1)      # the info tensor alone
        # ... and beside vectors that would do (no null: that is the vectors alone)
        assert_destinations_refused(ctx, lambda n, dst, stride: run(slots, n, prm(), d, msize, dst, stride), d2, isize, 1, null=False)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                                       # nothing was enqueued
        # the same call into memory the test owns is accepted: three frames of each tensor, nothing else written
        assert run(slots, 3, prm(), d, msize, d2, isize) == 0
        ctx.sync()
        a = big.cpu().numpy()
        for k in range(3):
            wm, wi = R.side(hdrs[k], irs[k][0], irs[k][1], 34, 23, "i16", 3)
            assert a[k * msize:(k + 1) * msize].tobytes() == wm.tobytes()
            assert a[(1 << 21) + k * isize:(1 << 21) + (k + 1) * isize].tobytes() == wi.tobytes()
        assert (a[3 * msize:1 << 21] == 0x5C).all() and (a[(1 << 21) + 3 * isize:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        with pytest.raises(ValueError):
            ctx.frames_side([0], mv_dtype=torch.int8)
        with pytest.raises(ValueError):
            ctx.frames_side([0], planes=("ref", "nope"))
        with pytest.raises(ValueError):
            ctx.frames_side([0], width=34)
        with pytest.raises(ValueError):
            ctx.frames_side([0], 34, 23, planes=(), out_mv=False)
        with pytest.raises(ValueError):
            ctx.frames_side([0, 1], 34, 23, out_mv=torch.empty((2, 2, 23, 36), dtype=torch.int16, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError):
            ctx.frames_side([3], 34, 23)
    finally:
        prod.close()


def test_no_new_device_memory(pkg, monkeypatch):
    """frames a large launch left as tiles: the call reads slots only -- no raster pool, no scratch, no field of memory_usage grows"""
    P = pkg
    monkeypatch.setenv("VP8HIP_RECON", "simt")
    n = 10
    w, h, frames = P.read_ivf(ivf_path("kf_640x360"))
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, n + 2, n)
        hdrs = []
        for i, data in enumerate(frames[:n]):
            ctx.sync()
            hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
            parser.swap(hdr)
            hdrs.append(hdr)
        ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)
        ctx.sync()
        before = ctx.memory_usage()
        assert before["raster_pool"] == 0 and before["tile_pool"] > 0
        for dw, dh, dtype in ((0, 0, "i16"), (w, h, "f32"), (224, 224, "f16"), (1001, 77, "f32")):
            mv, info = call(ctx, list(range(n)), dw, dh, dtype, 63)
            ir = slot_ir(ctx, n - 1)
            want = R.side(hdrs[n - 1], ir[0], ir[1], dw, dh, dtype, 63)
            assert np.array_equal(bits(mv[n - 1].cpu().numpy(), dtype), bits(want[0], dtype)) and np.array_equal(info[n - 1].cpu().numpy(), want[1])
            assert (info[:, 0] == 0).all() and (info[:, 4] == hdrs[0].base_qindex).any()
        assert ctx.memory_usage() == before
        assert ctx.rgb_scratch_bytes() == 0
    finally:
        parser.close()
        ctx.close()
