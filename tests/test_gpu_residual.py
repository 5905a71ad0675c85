"""GPU (-m gpu): the decoded residual of IR slots as tensors in device memory (vp8hip_frames_residual_async, Vp8Hip.frames_residual;
csrc/hip/vp8_residual.hip), bit for bit against the numpy restatement (tests/residual_reference.py, pinned to the oracle by
tests/test_residual_cpu.py) applied to the slot as vp8hip_ir_fetch reads it back -- for slots written by the host parser, by the
device's entropy decoder and on a pooled context -- and, independent of that file, against the decoder's own pixels.  torch is
imported here, before the package loads libvp8hip.so: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import ivf_path, synth_ir
from handover_testlib import (TORCH_DTYPE, Producer, assert_destinations_refused, assert_guards_intact, bits, guarded, later_writers_producer,
                              write_later_frames)
import residual_reference as R

pytestmark = pytest.mark.gpu

STREAMS = ["p_split_352x288", "p_arf_176x144", "p_seg_176x144", "p_odd_130x98", "kf_odd_67x45"]
LAYOUTS = ("planar", "i420")
B_PRED, SPLITMV = 4, 9


def call(ctx, slots, dw=0, dh=0, dtype="i16", layout="planar", scale=None, out=None):
    size = {} if dw == 0 else dict(width=dw, height=dh)
    return ctx.frames_residual(slots, dtype=TORCH_DTYPE[dtype], layout=layout, scale=scale, out=out, **size)


def check(ctx, slot, hdr, planes, dw=0, dh=0, dtype="i16", layout="planar", scale=None, what=None):
    """one slot through the call against the reference's planes of what the slot holds (planes = R.residual_planes of ir_fetch)"""
    got = call(ctx, [slot], dw, dh, dtype, layout, scale).cpu().numpy()[0]
    sc = (1.0, 1.0, 1.0) if scale is None else (scale,) * 3 if np.ndim(scale) == 0 else scale
    want = R.arrange(planes, hdr, dw, dh, dtype, layout, sc)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(bits(got, dtype), bits(want, dtype)), (what, dw, dh, dtype, layout, scale, int((bits(got, dtype) != bits(want, dtype)).sum()))


def slot_planes(ctx, slot, hdr):
    mbs, coef = ctx.ir_fetch(slot)
    return R.residual_planes(hdr, mbs, coef)


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", STREAMS)
def test_slot_producers(pkg, name, how):
    """the fixture's first frames: the native grid, both layouts, int16"""
    P = pkg
    prod = Producer(P, name, how)
    ctx = prod.ctx
    nonzero = 0
    try:
        nmb = ((prod.w + 15) // 16) * ((prod.h + 15) // 16)
        assert ctx.L.vp8hip_residual_size(ctx.h, ctypes.byref(P.ResidualParams(0, 0, 1, 0))) == 3 * 256 * nmb * 2
        assert ctx.L.vp8hip_residual_size(ctx.h, ctypes.byref(P.ResidualParams(0, 0, 0, 2))) == 384 * nmb * 4
        for i in range(min(len(prod.frames), 8)):
            hdr = prod.put(i)
            planes = slot_planes(ctx, 0, hdr)
            nonzero += int(planes[0].any()) + int(planes[1].any())
            for layout in LAYOUTS:
                check(ctx, 0, hdr, planes, layout=layout, what=(name, how, i, layout))
        assert nonzero > 0
    finally:
        prod.close()


def _branches(hdr, mbs, coef):
    """which branches of the definition a frame's IR takes"""
    y_mode, eobs = mbs[:, R.O_Y_MODE], mbs[:, R.O_EOBS:R.O_EOBS + 25]
    live = (mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0
    has_y2 = (y_mode != B_PRED) & (y_mode != SPLITMV)
    wrapped = any((a != b).any() for a, b in zip(R.residual_planes(hdr, mbs, coef), R.residual_planes(hdr, mbs, coef, wrap=False)))
    return {
        "y2 with more than a DC": bool((live & has_y2 & (eobs[:, 24] > 1)).any()),
        "y2 with a DC or nothing": bool((live & has_y2 & (eobs[:, 24] <= 1)).any()),
        "a lone DC": bool((live[:, None] & (eobs[:, 16:24] == 1)).any() and ((live & ~has_y2)[:, None] & (eobs[:, :16] == 1)).any()),
        "a Y2 macroblock's luma block with eob <= 1": bool(((live & has_y2)[:, None] & (eobs[:, :16] <= 1)).any()),
        "a block with eob > 1": bool((live[:, None] & (eobs[:, :24] > 1)).any()),
        "B_PRED": bool((live & (y_mode == B_PRED)).any()),
        "SPLITMV": bool((live & (y_mode == SPLITMV)).any()),
        "skipped": bool((~live).any()),
        "an int16 truncation that bites": bool(wrapped),
    }


def test_random_ir(pkg):
    """random macroblocks with coefficients up to +-2047 and segment quantisers, one macroblock to 99, key and inter frames"""
    P = pkg
    seen = {}
    for (w, h), inter in itertools.product(((16, 16), (67, 45), (176, 144)), (False, True)):
        ctx = P.Vp8Hip(0)
        try:
            ctx.configure(w, h, 1, 1)
            for seed in ((1, 2, 3, 4, 5, 6) if w == 16 else (7, 8)):
                hdr, mbs, coef, mvs = synth_ir(w, h, seed + 100 * inter, inter=inter, big=True, segmented=True, dense=0.5)
                ctx.fill_slot(0, hdr, mbs, coef, mvs)
                got_mbs, got_coef = ctx.ir_fetch(0)
                assert np.array_equal(got_mbs[:, :56], mbs[:, :56])
                if w > 16:
                    for k, v in _branches(hdr, got_mbs, got_coef).items():
                        seen[k] = seen.get(k, False) or v
                planes = R.residual_planes(hdr, got_mbs, got_coef)
                for layout in LAYOUTS:
                    check(ctx, 0, hdr, planes, layout=layout, what=(w, h, inter, seed, layout))
                check(ctx, 0, hdr, planes, w, h, "f32", "planar", 0.5, what=(w, h, inter, seed))
        finally:
            ctx.close()
    assert all(seen.values()), seen


@pytest.mark.parametrize("size", [(4112, 32), (16383, 16)])
def test_hand_built_wide_slots(pkg, size):
    """macroblock rows of 257 and 1024 macroblocks: many runs a row, the last one short or full"""
    P = pkg
    w, h = size
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        hdr, mbs, coef, mvs = synth_ir(w, h, w + h, inter=False, big=True, dense=0.4)       # (a key frame: vectors this far out leave int16)
        ctx.fill_slot(0, hdr, mbs, coef, mvs)
        planes = slot_planes(ctx, 0, hdr)
        assert planes[0].any() and planes[2].any()
        for (dw, dh), dtype, layout in (((0, 0), "i16", "planar"), ((0, 0), "i16", "i420"), ((w, h), "f16", "i420"), ((w, h), "i16", "planar"),
                                        ((w // 3 + 1, 2 * h + 1), "i16", "planar"), ((min(w + 5, 16383), 7), "f32", "i420")):
            check(ctx, 0, hdr, planes, dw, dh, dtype, layout, 0.25, what=(size, dw, dh, dtype, layout))
    finally:
        ctx.close()


@pytest.mark.parametrize("name,sizes", [("p_odd_130x98", ((130, 98), (1, 1), (7, 3), (224, 224), (260, 196))), ("p_split_352x288", ((350, 286),))])
def test_sized_grids(pkg, name, sizes):
    """both layouts at each size, into an aligned tensor and into one that begins one element further on, where every store is
    element by element"""
    P = pkg
    prod = Producer(P, name, "host")
    ctx = prod.ctx
    try:
        prod.put(0)
        hdr = prod.put(1)
        mbs, coef = ctx.ir_fetch(0)
        planes = R.residual_planes(hdr, mbs, coef)
        assert hdr.frame_type == 1 and planes[0].any()
        for (dw, dh), layout, dtype in itertools.product(sizes, LAYOUTS, ("i16", "f32")):
            what = (name, dw, dh, layout, dtype)
            check(ctx, 0, hdr, planes, dw, dh, dtype, layout, 0.5, what=what)
            want = R.arrange(planes, hdr, dw, dh, dtype, layout, (0.5,) * 3)
            big = torch.zeros(want.size + 16, dtype=TORCH_DTYPE[dtype], device="cuda:0")
            out = big[1:1 + want.size].view((1,) + want.shape)                 # one element further on
            assert out.data_ptr() % (8 if dtype == "i16" else 16) != 0
            got = call(ctx, [0], dw, dh, dtype, layout, 0.5, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert np.array_equal(bits(got.cpu().numpy()[0], dtype), bits(want, dtype)), what
            a = big.cpu().numpy()
            assert not a[:1].any() and not a[1 + want.size:].any(), what
    finally:
        prod.close()


def test_float_types(pkg):
    """a frame whose residual spans the int16 range against scales that make the float land on ties of the halves (the half is the
    FLOAT rounded: two roundings), powers of two, negative ones, ones so small that the floats are denormal, and a scale per plane"""
    P = pkg
    w, h = 176, 144
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        hdr, mbs, coef, mvs = synth_ir(w, h, 77, inter=True, big=True, dense=0.6)
        ctx.fill_slot(0, hdr, mbs, coef, mvs)
        planes = slot_planes(ctx, 0, hdr)
        assert len(np.unique(planes[0])) > 2000 and np.abs(planes[0].astype(np.int64)).max() > 4000
        differ = 0
        for sc in ((1.0, 1.0, 1.0), (0.125, 0.125, 0.125), (0.125 * 224 / 1920, 0.125 * 224 / 1080, 1.0), (-1.0 / 3, 1e-3, 7.0), (2.0 ** -20, 3.0e4, 1e30),
                   (1.0 / 7, 65504.0 / 32767, -0.5), (1.0285249948501587, 1.9014227390289307, 0.2968776226043701), (1e-42, -3e-41, 2.0 ** -24),
                   (1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 / 255)):
            scale = tuple(np.float32(s) for s in sc)
            for dtype, layout in (("f32", "planar"), ("f16", "planar"), ("f16", "i420"), ("f32", "i420")):
                check(ctx, 0, hdr, planes, 0, 0, dtype, layout, scale, what=sc)
            with np.errstate(over="ignore"):
                once = (planes[0].astype(np.float64) * np.float64(scale[0])).astype(np.float16)
            differ += int((once != R.convert(planes[0], "f16", scale[0])).sum())
        assert differ > 0                               # (the sweep holds values one rounding would get wrong)
        check(ctx, 0, hdr, planes, w, h, "f16", "planar", 0.03125)            # one number for all three planes
    finally:
        ctx.close()


def test_destination_hygiene(pkg):
    """frames at padded strides, aligned to the piece and to the element only: the guard bytes before, between and behind them stay"""
    P = pkg
    n = 3
    prod = Producer(P, "p_odd_130x98", "host", nslots=n)
    ctx = prod.ctx
    try:
        prod.put(0)
        hdrs = [prod.put(i + 1, i) for i in range(n)]   # inter frames
        planes = [slot_planes(ctx, i, hdrs[i]) for i in range(n)]
        slots = [2, 0, 1]
        for (dw, dh), dtype, layout, (off, pad) in itertools.product(((130, 98), (64, 36), (0, 0), (33, 17)), ("i16", "f16", "f32"), LAYOUTS,
                                                                     ((0, 0), (2, 6), (4, 4), (8, 24), (16, 16))):
            es = 4 if dtype == "f32" else 2
            off, pad = off // es * es, pad // es * es                       # (the call refuses what is not aligned to the element)
            size = R.size(hdrs[0], dw, dh, dtype, layout)
            big, flat = guarded(n, size, pad, off)
            flat = flat.view(TORCH_DTYPE[dtype])
            gw, gh = (dw, dh) if dw else (16 * hdrs[0].mb_cols, 16 * hdrs[0].mb_rows)
            out = flat.unflatten(1, (3, gh, gw)) if layout == "planar" else flat
            got = call(ctx, slots, dw, dh, dtype, layout, (0.25, 0.5, 2.0), out=out)
            assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == off % 16
            g = got.cpu().numpy()
            for k, s in enumerate(slots):
                want = R.arrange(planes[s], hdrs[s], dw, dh, dtype, layout, (0.25, 0.5, 2.0))
                assert np.array_equal(bits(g[k], dtype), bits(want, dtype)), (dw, dh, dtype, layout, off, pad, k)
            assert_guards_intact(big, n, size, pad, off, what=(dw, dh, dtype, layout, off, pad))
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the tensor read on torch's stream: it holds what the slots held at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx, w, h = prod.ctx, prod.w, prod.h
    try:
        old = [R.arrange(slot_planes(ctx, i, hdrs[i]), hdrs[i], w, h, "f32", "planar", (0.5, 0.5, 0.5)) for i in range(n)]
        out = call(ctx, list(range(n)), w, h, "f32", "planar", 0.5)
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        g = out.cpu().numpy()                           # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(bits(g[i], "f32"), bits(old[i], "f32")), i
        ctx.sync()
        # ... and the slots now hold the later frames
        changed = 0
        for i in range(n):
            hdr = new_hdrs[i]
            planes = slot_planes(ctx, i, hdr)
            check(ctx, i, hdr, planes, w, h, "f32", "planar", 0.5)
            changed += not np.array_equal(R.arrange(planes, hdr, w, h, "f32", "planar", (0.5, 0.5, 0.5)), old[i])
        assert changed > 0
    finally:
        prod.close()


def test_batch_boundary(pkg):
    """a list longer than one launch's slot table (128), with repeats, of one-macroblock frames that all differ"""
    P = pkg
    nsrc = 40
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(16, 16, 1, nsrc)
        refs = {}
        for s in range(nsrc):
            hdr, mbs, coef, mvs = synth_ir(16, 16, 300 + s, inter=bool(s & 1), big=True, dense=0.7)
            ctx.fill_slot(s, hdr, mbs, coef, mvs)
            refs[s] = (hdr, slot_planes(ctx, s, hdr))
        assert sum(bool(p[0].any()) for _, p in refs.values()) > nsrc // 2
        rng = np.random.default_rng(3)
        for slots in ([int(s) for s in rng.integers(0, nsrc, 300)], [s % nsrc for s in range(129)], [7] * 128 + [9]):
            for layout, dtype in (("planar", "i16"), ("i420", "f32")):
                got = call(ctx, slots, 0, 0, dtype, layout, (1.0, -2.0, 0.5)).cpu().numpy()
                assert got.shape[0] == len(slots)
                for k, s in enumerate(slots):
                    want = R.arrange(refs[s][1], refs[s][0], 0, 0, dtype, layout, (1.0, -2.0, 0.5))
                    assert np.array_equal(bits(got[k], dtype), bits(want, dtype)), (k, s, layout)
    finally:
        ctx.close()


def test_identity_with_the_decoders_own_pixels(pkg):
    """independent of the numpy file: an inter frame reconstructed by vp8hip_decode, and reconstructed again from a copy of its slot
    with every record flagged skipped -- the prediction alone; on the inter macroblocks clamp255(pred + R) is the reconstruction"""
    P = pkg
    w, h, frames = P.read_ivf(ivf_path("p_seg_176x144"))
    ctx, parser = P.Vp8Hip(0), P.Parser()
    try:
        ctx.configure(w, h, 6, 2)
        g = ctx.g
        checked = 0
        for i, data in enumerate(frames[:4]):
            hdr, _, mbs, coef, mvs = P.parse_to_numpy(parser, data)
            r = parser.refs
            refs = (r.lst_idx, r.gld_idx, r.alt_idx)
            ctx.sync()
            ctx.fill_slot(0, hdr, mbs, coef, mvs)
            inter = (mbs[:, R.O_REF] != 0).reshape(hdr.mb_rows, hdr.mb_cols)
            if inter.any():
                skipped = mbs.copy()
                skipped[:, R.O_FLAGS] |= R.MB_SKIP
                ctx.fill_slot(1, hdr, skipped, np.zeros_like(coef), mvs)
                ctx.decode([(0, 4, refs)], P.STAGE_RECON)
                ctx.decode([(1, 5, refs)], P.STAGE_RECON)
                rec, pred = ctx.download_full(4), ctx.download_full(5)
                res = call(ctx, [0]).cpu().numpy()[0].astype(np.int64)
                assert res.shape == (3, g.aligned_h, g.aligned_w)

                def view(buf, off, stride, pw, ph):
                    return np.lib.stride_tricks.as_strided(buf[off:], shape=(ph, pw), strides=(stride, 1)).astype(np.int64)
                m = inter.repeat(16, 0).repeat(16, 1)
                a, b = view(rec, g.y_off, g.y_stride, g.aligned_w, g.aligned_h), view(pred, g.y_off, g.y_stride, g.aligned_w, g.aligned_h)
                assert np.array_equal(np.clip(b + res[0], 0, 255)[m], a[m]), i
                for k, off in ((1, g.u_off), (2, g.v_off)):
                    a, b = (view(buf, off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2).repeat(2, 0).repeat(2, 1) for buf in (rec, pred))
                    assert np.array_equal(np.clip(b + res[k], 0, 255)[m], a[m]), (i, k)
                checked += int(m.sum()) if res[0][m].any() else 0
            ctx.decode([(0, r.new_idx, refs)], P.STAGE_ALL)
            parser.swap(hdr)
        assert checked > 10000
    finally:
        parser.close()
        ctx.close()


def test_refusals(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host", nslots=4)
    ctx = prod.ctx
    L = ctx.L
    try:
        hdrs = [prod.put(i, i) for i in range(3)]       # slot 3 is never filled
        planes = [slot_planes(ctx, i, hdrs[i]) for i in range(3)]
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        assert d % 16 == 0
        slots = (ctypes.c_int * 3)(0, 1, 2)

        def prm(w=34, h=23, layout=1, dtype=0):
            return P.ResidualParams(w, h, layout, dtype)

        def run(arr, n, p, dst, stride):
            return L.vp8hip_frames_residual_async(ctx.h, arr, n, ctypes.byref(p), ctypes.c_void_p(dst) if dst else None, stride)
        size = 3 * 34 * 23 * 2
        assert L.vp8hip_residual_size(ctx.h, ctypes.byref(prm())) == size
        assert run(slots, 0, prm(), d, size) == -2
        assert run(slots, -1, prm(), d, size) == -2
        for bad in (-1, 4, 1 << 20):
            assert run((ctypes.c_int * 1)(bad), 1, prm(), d, size) == -2, bad
        assert run((ctypes.c_int * 1)(3), 1, prm(), d, size) == -2        # never filled
        assert run((ctypes.c_int * 2)(0, 3), 2, prm(), d, size) == -2
        for w, h in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5), (-1, -1)):
            assert run(slots, 3, prm(w, h), d, 1 << 20) == -2, (w, h)
        for dt in (-1, 3):
            assert run(slots, 3, prm(dtype=dt), d, 1 << 20) == -2
        for lay in (-1, 2, 77):
            assert run(slots, 3, prm(layout=lay), d, 1 << 20) == -2
        assert run(slots, 3, prm(layout=0), d, (34 * 23 + 2 * 17 * 12) * 2 - 2) == -2
        for dtype, es in ((0, 2), (1, 2), (2, 4)):          # each type: also the alignment to its element
            assert_destinations_refused(ctx, lambda n, dst, stride: run(slots, n, prm(dtype=dtype), dst, stride), d, size * es // 2, es)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                            # nothing was enqueued
        # the same call into memory the test owns is accepted: three frames, nothing else written
        assert run(slots, 3, prm(), d, size) == 0
        ctx.sync()
        a = big.cpu().numpy()
        for k in range(3):
            want = R.arrange(planes[k], hdrs[k], 34, 23, "i16", "planar")
            assert a[k * size:(k + 1) * size].tobytes() == want.tobytes()
        assert (a[3 * size:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        with pytest.raises(ValueError):
            ctx.frames_residual([0], dtype=torch.int8)
        with pytest.raises(ValueError):
            ctx.frames_residual([0], layout="nhwc")
        with pytest.raises(ValueError):
            ctx.frames_residual([0], width=34)
        with pytest.raises(ValueError):
            ctx.frames_residual([0], 34, 23, scale=(1.0, 2.0))
        with pytest.raises(ValueError):
            ctx.frames_residual([0, 1], 34, 23, out=torch.empty((2, 3, 23, 36), dtype=torch.int16, device="cuda:0")[:, :, :, :34])
        with pytest.raises(RuntimeError):
            ctx.frames_residual([3], 34, 23)
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
        planes = slot_planes(ctx, n - 1, hdrs[n - 1])
        for dw, dh, dtype, layout in ((0, 0, "i16", "i420"), (w, h, "f32", "planar"), (224, 224, "f16", "planar"), (1001, 77, "f32", "i420")):
            out = call(ctx, list(range(n)), dw, dh, dtype, layout, 0.5)
            want = R.arrange(planes, hdrs[n - 1], dw, dh, dtype, layout, (0.5, 0.5, 0.5))
            assert np.array_equal(bits(out[n - 1].cpu().numpy(), dtype), bits(want, dtype)), (dw, dh, dtype, layout)
        assert ctx.memory_usage() == before
        assert ctx.rgb_scratch_bytes() == 0
    finally:
        parser.close()
        ctx.close()
