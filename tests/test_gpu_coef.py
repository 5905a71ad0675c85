"""GPU (-m gpu): the transform coefficients of IR slots as tensors in device memory (vp8hip_frames_coef_async, Vp8Hip.frames_coef;
csrc/hip/vp8_coef.hip), bit for bit against the numpy restatement (tests/coef_reference.py, held to the oracle and to the residual's
restatement by tests/test_coef_cpu.py) applied to the slot as vp8hip_ir_fetch reads it back -- for slots written by the host parser,
by the device's entropy decoder and on a pooled context -- and, independent of that file, against vp8hip_frames_residual_async and
the dense coefficients.  torch is imported here, before the package loads libvp8hip.so: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import synth_ir
from handover_testlib import (TORCH_DTYPE, Producer, assert_destinations_refused, assert_guards_intact, bits, guarded, later_writers_producer,
                              write_later_frames)
import coef_reference as C
import residual_reference as R

pytestmark = pytest.mark.gpu

STAGES = ("dequant", "levels")
LAYOUTS = ("channels", "inplace")
ALL = C.PLANES


def names(mask):
    return tuple(p for k, p in enumerate(C.PLANES) if mask >> k & 1)


def slot_blocks(ctx, slot, hdr):
    """the restatement's blocks of what the slot holds, by stage"""
    mbs, coef = ctx.ir_fetch(slot)
    return {stage: C.coef_blocks(hdr, mbs, coef, stage) for stage in STAGES}


def call(ctx, slots, stage="dequant", layout="channels", planes=ALL, nfreq=16, order="raster", dtype="i16", scale=None, out=None):
    return ctx.frames_coef(slots, stage=stage, layout=layout, planes=planes, nfreq=nfreq, order=order, dtype=TORCH_DTYPE[dtype], scale=scale, out=out)


def check(ctx, slot, hdr, blocks, stage="dequant", layout="channels", planes=ALL, nfreq=16, order="raster", dtype="i16", scale=None, what=None):
    """one slot through the call against the restatement's blocks of what the slot holds (blocks = slot_blocks)"""
    got = call(ctx, [slot], stage, layout, planes, nfreq, order, dtype, scale)
    sc = (1.0,) * 4 if scale is None else (scale,) * 4 if np.ndim(scale) == 0 else scale
    want, _ = C.arrange(blocks[stage], hdr, layout, names(planes) if isinstance(planes, int) else planes, nfreq, order, dtype, sc)
    assert list(got) == list(want), (what, list(got))
    for name in want:
        g = got[name].cpu().numpy()[0]
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, (what, name, g.shape, want[name].shape)
        bad = int((bits(g, dtype) != bits(want[name], dtype)).sum())
        assert bad == 0, (what, stage, layout, planes, nfreq, order, dtype, scale, name, bad)


@pytest.mark.parametrize("how", ["host", "entropy", "pooled"])
@pytest.mark.parametrize("name", ["p_odd_130x98", "kf_odd_67x45"])
def test_slot_producers(pkg, name, how):
    """the fixture's first frames: both stages, both layouts, all four planes, int16"""
    P = pkg
    prod = Producer(P, name, how)
    ctx = prod.ctx
    nonzero = 0
    try:
        for i in range(min(len(prod.frames), 4)):
            hdr = prod.put(i)
            blocks = slot_blocks(ctx, 0, hdr)
            nonzero += int(blocks["levels"][:, :24].any()) + int(blocks["dequant"][:, 24].any())
            for stage, layout in itertools.product(STAGES, LAYOUTS):
                check(ctx, 0, hdr, blocks, stage, layout, what=(name, how, i))
        assert nonzero > 1
    finally:
        prod.close()


def _branches(hdr, mbs, coef):
    """which branches of the definition a frame's IR takes"""
    kind, has_y2 = C.block_kinds(mbs)
    y_mode, eobs = mbs[:, R.O_Y_MODE], mbs[:, R.O_EOBS:R.O_EOBS + 25]
    live = (mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0
    lv = C.coef_blocks(hdr, mbs, coef, "levels")
    f = R.factors(hdr)[mbs[:, R.O_SEGMENT] & 3]
    return {
        "y2 with more than a DC": bool((live & has_y2 & (eobs[:, 24] > 1)).any()),
        "y2 with a DC alone": bool((live & has_y2 & (eobs[:, 24] == 1)).any()),
        "y2 with nothing": bool((live & has_y2 & (eobs[:, 24] == 0)).any()),
        "a lone DC": bool((kind[:, 16:24] == 1).any() and (kind[:, :16] == 1).any()),
        "a block with eob > 1": bool((kind[:, :24] == 2).any()),
        "an empty block beside full ones": bool((live[:, None] & (kind[:, :24] == 0)).any()),
        "B_PRED": bool((live & (y_mode == R.B_PRED)).any()),
        "SPLITMV": bool((live & (y_mode == R.SPLITMV)).any()),
        "skipped": bool((~live).any()),
        "an int16 truncation that bites": bool((np.abs(lv[:, :16] * f[:, 1][:, None, None, None]) > 32767).any()),
    }


RANDOM_SIZES = ((16, 16), (67, 45), (176, 144), (272, 16))


def test_random_ir(pkg):
    """random macroblocks with coefficients up to +-2047 and segment quantisers: one macroblock (rows of 2 and 1 elements), 5 x 3 (odd
    columns: U, V and Y2 element by element), 11 x 9, and 17 x 1 (Y2 rows of 17); key and inter frames; every plane mask; the
    channel counts under both orders"""
    P = pkg
    seen = {}
    for w, h in RANDOM_SIZES:
        ctx = P.Vp8Hip(0)
        try:
            ctx.configure(w, h, 1, 1)
            for inter, seed in itertools.product((False, True), (1, 2, 3) if w == 16 else (7, 8)):
                hdr, mbs, coef, mvs = synth_ir(w, h, seed + 100 * inter, inter=inter, big=True, segmented=True, dense=0.5)
                ctx.fill_slot(0, hdr, mbs, coef, mvs)
                got_mbs, got_coef = ctx.ir_fetch(0)
                assert np.array_equal(got_mbs[:, :56], mbs[:, :56])
                for k, v in _branches(hdr, got_mbs, got_coef).items():
                    seen[k] = seen.get(k, False) or v
                blocks = {stage: C.coef_blocks(hdr, got_mbs, got_coef, stage) for stage in STAGES}
                what = (w, h, inter, seed)
                for stage, layout in itertools.product(STAGES, LAYOUTS):
                    check(ctx, 0, hdr, blocks, stage, layout, what=what)
                for (nfreq, order), stage in zip(itertools.product((1, 3, 10, 16), ("raster", "zigzag")), itertools.cycle(STAGES)):
                    check(ctx, 0, hdr, blocks, stage, "channels", ALL, nfreq, order, what=what)
                if (w, seed) == (67, 7):
                    for mask in range(1, 16):
                        check(ctx, 0, hdr, blocks, STAGES[mask & 1], "channels", names(mask), 3 + mask % 3, "zigzag", what=what)
                        check(ctx, 0, hdr, blocks, STAGES[~mask & 1], "inplace", mask, what=what)     # (the mask itself)
        finally:
            ctx.close()
    assert all(seen.values()), seen


def test_hand_built_wide_slot(pkg):
    """a macroblock row of 257 macroblocks: nine runs, the last of one macroblock"""
    P = pkg
    w, h = 4112, 32
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        hdr, mbs, coef, mvs = synth_ir(w, h, w + h, inter=False, big=True, dense=0.4)
        ctx.fill_slot(0, hdr, mbs, coef, mvs)
        blocks = slot_blocks(ctx, 0, hdr)
        assert blocks["levels"][-1].any() or blocks["levels"][256].any()
        for stage, layout, nfreq, order, dtype in (("dequant", "channels", 16, "raster", "i16"), ("levels", "inplace", 16, "raster", "i16"),
                                                   ("levels", "channels", 6, "zigzag", "f16"), ("dequant", "inplace", 16, "raster", "f32")):
            check(ctx, 0, hdr, blocks, stage, layout, ALL, nfreq, order, dtype, 0.25, what=(stage, layout, nfreq, order, dtype))
    finally:
        ctx.close()


def test_independent_of_the_restatement(pkg):
    """DEQUANT, in place, int16, through the reference's inverse DCT on the host is frames_residual's native I420 tensor of the same slot;
    LEVELS is ir_fetch's dense coefficients under the definition's zeros; the Y2 plane's inverse WHT gives the luma DCs"""
    P = pkg
    checked = 0
    for (w, h), inter in itertools.product(((67, 45), (176, 144)), (False, True)):
        ctx = P.Vp8Hip(0)
        try:
            ctx.configure(w, h, 1, 1)
            hdr, mbs, coef, mvs = synth_ir(w, h, 21 + inter, inter=inter, big=True, segmented=True, dense=0.5)
            ctx.fill_slot(0, hdr, mbs, coef, mvs)
            rows, cols = hdr.mb_rows, hdr.mb_cols
            got = {k: v.cpu().numpy()[0].astype(np.int64) for k, v in call(ctx, [0], "dequant", "inplace").items()}
            res = P.split_residual(ctx.frames_residual([0], layout="i420").cpu().numpy()[0], 16 * cols, 16 * rows)
            for name, r in zip(("y", "u", "v"), res):
                g = C.CELLS[name]
                blk = got[name].reshape(g * rows, 4, g * cols, 4).transpose(0, 2, 1, 3)                    # [block row, block col, v, u]
                back = R.idct(blk).transpose(0, 2, 1, 3).reshape(4 * g * rows, 4 * g * cols)
                assert np.array_equal(back, r.astype(np.int64)), (w, h, inter, name)
                checked += int((r != 0).sum())
            # LEVELS against the dense coefficients as the slot gives them back
            got_mbs, dense = ctx.ir_fetch(0)
            dense = np.asarray(dense, np.int64).reshape(-1, 25, 4, 4).transpose(0, 1, 3, 2).copy()         # [mb, block, v, u]
            y_mode = got_mbs[:, R.O_Y_MODE]
            has_y2 = (y_mode != R.B_PRED) & (y_mode != R.SPLITMV)
            dense[(got_mbs[:, R.O_FLAGS] & R.MB_SKIP) != 0] = 0
            dense[has_y2, :16, 0, 0] = 0
            dense[~has_y2, 24] = 0
            lv = {k: v.cpu().numpy()[0] for k, v in call(ctx, [0], "levels", "channels").items()}
            for name in C.PLANES:
                g, first = C.CELLS[name], C.FIRST[name]
                want = dense[:, first:first + g * g].reshape(rows, cols, g, g, 16).transpose(4, 0, 2, 1, 3).reshape(16, g * rows, g * cols)
                assert np.array_equal(lv[name], want), (w, h, inter, name)
            # the DEQUANT Y2 plane through the inverse WHT: the luma DCs of the macroblocks that have one and code more than its DC
            y2 = got["y2"].reshape(rows, 4, cols, 4).transpose(0, 2, 1, 3).reshape(-1, 4, 4)
            dcs = got["y"].reshape(4 * rows, 4, 4 * cols, 4)[:, 0, :, 0].reshape(rows, 4, cols, 4).transpose(0, 2, 1, 3).reshape(-1, 4, 4)
            full = has_y2 & ((got_mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0) & (got_mbs[:, R.O_EOBS + 24] > 1)
            assert full.sum() > 3 and np.array_equal(R.inv_walsh(y2[full]), dcs[full])
        finally:
            ctx.close()
    assert checked > 20000


def test_float_types(pkg):
    """test_gpu_residual.test_float_types's scales -- ties of the halves, powers of two, negative ones, denormal floats -- with a scale of
    its own for each of the four planes"""
    P = pkg
    w, h = 176, 144
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 1, 1)
        hdr, mbs, coef, mvs = synth_ir(w, h, 77, inter=True, big=True, dense=0.6)
        ctx.fill_slot(0, hdr, mbs, coef, mvs)
        blocks = slot_blocks(ctx, 0, hdr)
        y = blocks["dequant"][:, :16]
        assert len(np.unique(y)) > 2000 and np.abs(y).max() > 20000
        triples = ((1.0, 1.0, 1.0), (0.125, 0.125, 0.125), (0.125 * 224 / 1920, 0.125 * 224 / 1080, 1.0), (-1.0 / 3, 1e-3, 7.0), (2.0 ** -20, 3.0e4, 1e30),
                   (1.0 / 7, 65504.0 / 32767, -0.5), (1.0285249948501587, 1.9014227390289307, 0.2968776226043701), (1e-42, -3e-41, 2.0 ** -24),
                   (1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 / 255))
        differ = 0
        for i, sc in enumerate(triples):
            scale = tuple(np.float32(s) for s in sc + (triples[(i + 1) % len(triples)][0],))         # Y, U, V and a fourth for Y2
            for (dtype, layout), stage in zip((("f32", "channels"), ("f16", "channels"), ("f16", "inplace"), ("f32", "inplace")), itertools.cycle(STAGES)):
                check(ctx, 0, hdr, blocks, stage, layout, ALL, 16, "raster", dtype, scale, what=sc)
            with np.errstate(over="ignore"):
                once = (y.astype(np.float64) * np.float64(scale[0])).astype(np.float16)
            differ += int((once != R.convert(y, "f16", scale[0])).sum())
        assert differ > 0                               # (the sweep holds values one rounding would get wrong)
        check(ctx, 0, hdr, blocks, "dequant", "channels", ("y", "y2"), 5, "zigzag", "f16", 0.03125)        # one number for all planes
    finally:
        ctx.close()


def test_destination_hygiene(pkg):
    """frames at padded strides, aligned to the piece and to the element only -- one element off: every store element by element -- the
    guard bytes before, between and behind them stay"""
    P = pkg
    n = 3
    prod = Producer(P, "p_odd_130x98", "host", nslots=n)
    ctx = prod.ctx
    try:
        prod.put(0)
        hdrs = [prod.put(i + 1, i) for i in range(n)]   # inter frames
        blocks = [slot_blocks(ctx, i, hdrs[i]) for i in range(n)]
        slots = [2, 0, 1]
        scale = (0.25, 0.5, 2.0, -1.0)
        for (stage, layout, planes, nfreq), dtype, (off, pad) in itertools.product(
                (("dequant", "channels", ALL, 16), ("levels", "inplace", ALL, 16), ("dequant", "channels", ("u", "y2"), 3), ("levels", "channels", ("y2",), 1)),
                ("i16", "f16", "f32"), ((0, 0), (2, 6), (4, 4), (8, 24), (16, 16))):
            es = 4 if dtype == "f32" else 2
            off, pad = off // es * es, pad // es * es                       # (the call refuses what is not aligned to the element)
            size = C.size(hdrs[0], layout, planes, nfreq, dtype)
            assert size == P.coef_size(ctx, stage, layout, planes, nfreq, "raster", TORCH_DTYPE[dtype])
            big, flat = guarded(n, size, pad, off)
            out = flat.view(TORCH_DTYPE[dtype])
            got = call(ctx, slots, stage, layout, planes, nfreq, "raster", dtype, scale, out=out)
            first = next(iter(got.values()))
            assert first.data_ptr() == out.data_ptr() and first.data_ptr() % 16 == off % 16
            g = out.cpu().numpy()
            for k, s in enumerate(slots):
                _, want = C.arrange(blocks[s][stage], hdrs[s], layout, planes, nfreq, "raster", dtype, scale)
                assert np.array_equal(bits(g[k], dtype), bits(want, dtype)), (stage, layout, planes, dtype, off, pad, k)
            assert_guards_intact(big, n, size, pad, off, what=(stage, layout, planes, dtype, off, pad))
    finally:
        prod.close()


@pytest.mark.parametrize("how", ["host", "entropy", "copy"])
def test_ordering_against_later_slot_writers(pkg, how):
    """the call, then at once the next frames into the same slots (an upload; an entropy launch; vp8hip_ir_copy from slots that hold
    them), then the tensor read on torch's stream: it holds what the slots held at the call"""
    P = pkg
    n = 4
    prod, hdrs, staged = later_writers_producer(P, "p_split_352x288", how, n)
    ctx = prod.ctx
    try:
        old = [C.arrange(slot_blocks(ctx, i, hdrs[i])["dequant"], hdrs[i], "channels", ALL, 16, "raster", "f32", (0.5,) * 4)[1] for i in range(n)]
        out = torch.empty((n, old[0].size), dtype=torch.float32, device="cuda:0")
        call(ctx, list(range(n)), "dequant", "channels", ALL, 16, "raster", "f32", 0.5, out=out)
        new_hdrs = write_later_frames(P, prod, how, n, staged)
        g = out.cpu().numpy()                           # .cpu() on torch's current stream
        for i in range(n):
            assert np.array_equal(bits(g[i], "f32"), bits(old[i], "f32")), i
        ctx.sync()
        # ... and the slots now hold the later frames
        changed = 0
        for i in range(n):
            blocks = slot_blocks(ctx, i, new_hdrs[i])
            check(ctx, i, new_hdrs[i], blocks, "dequant", "channels", ALL, 16, "raster", "f32", 0.5)
            changed += not np.array_equal(C.arrange(blocks["dequant"], new_hdrs[i], "channels", ALL, 16, "raster", "f32", (0.5,) * 4)[1], old[i])
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
            refs[s] = (hdr, slot_blocks(ctx, s, hdr))
        assert sum(bool(b["levels"].any()) for _, b in refs.values()) > nsrc // 2
        rng = np.random.default_rng(3)
        scale = (1.0, -2.0, 0.5, 3.0)
        for slots in ([int(s) for s in rng.integers(0, nsrc, 300)], [s % nsrc for s in range(129)], [7] * 128 + [9]):
            for stage, layout, dtype in (("dequant", "channels", "i16"), ("levels", "inplace", "f32")):
                got = call(ctx, slots, stage, layout, ALL, 16, "raster", dtype, scale)
                flat = np.concatenate([got[p].cpu().numpy().reshape(len(slots), -1) for p in got], 1)
                assert flat.shape[0] == len(slots)
                for k, s in enumerate(slots):
                    _, want = C.arrange(refs[s][1][stage], refs[s][0], layout, ALL, 16, "raster", dtype, scale)
                    assert np.array_equal(bits(flat[k], dtype), bits(want, dtype)), (k, s, layout)
    finally:
        ctx.close()


def test_sizes_on_a_context(pkg):
    """vp8hip_coef_size on a context against the restatement for every layout, channel count and plane mask; 0 for every refusal"""
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host")
    ctx = prod.ctx
    L = ctx.L
    try:
        hdr = prod.put(0)
        for layout, nfreq, mask, (dt, dname) in itertools.product(LAYOUTS, range(1, 17), range(1, 16), enumerate(("i16", "f16", "f32"))):
            for order in (0, 1):
                p = P.CoefParams(0, C.LAYOUTS[layout], order, nfreq, mask, dt)
                ok = layout == "channels" or (nfreq == 16 and order == 0)
                want = C.size(hdr, layout, names(mask), nfreq, dname) if ok else 0
                assert L.vp8hip_coef_size(ctx.h, ctypes.byref(p)) == want, (layout, nfreq, mask, dname, order)
        assert P.coef_size(ctx) == 16 * 24 * 63 * 2 and P.coef_size(ctx, "levels", "inplace", ("y2",), dtype=torch.float32) == 16 * 63 * 4
        assert P.coef_size(ctx, nfreq=0) == 0 and P.coef_size(ctx, nfreq=17) == 0 and P.coef_size(ctx, layout="inplace", order="zigzag") == 0
        assert P.coef_size(ctx, planes=()) == 0 and P.coef_size(ctx, planes=16) == 0 and P.coef_size(ctx, stage="idct") == 0
        assert L.vp8hip_coef_size(ctx.h, None) == 0
    finally:
        prod.close()


def test_refusals(pkg):
    P = pkg
    prod = Producer(P, "p_odd_130x98", "host", nslots=4)
    ctx = prod.ctx
    L = ctx.L
    try:
        hdrs = [prod.put(i, i) for i in range(3)]       # slot 3 is never filled
        blocks = [slot_blocks(ctx, i, hdrs[i]) for i in range(3)]
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        assert d % 16 == 0
        slots = (ctypes.c_int * 3)(0, 1, 2)

        def prm(stage=0, layout=0, order=0, nfreq=4, planes=9, dtype=0):
            return P.CoefParams(stage, layout, order, nfreq, planes, dtype)

        def run(arr, n, p, dst, stride):
            return L.vp8hip_frames_coef_async(ctx.h, arr, n, ctypes.byref(p) if p is not None else None, ctypes.c_void_p(dst) if dst else None, stride)
        size = 4 * 17 * 63 * 2
        assert L.vp8hip_coef_size(ctx.h, ctypes.byref(prm())) == size
        assert run(slots, 0, prm(), d, size) == -2
        assert run(slots, -1, prm(), d, size) == -2
        assert run(None, 3, prm(), d, size) == -2
        assert run(slots, 3, None, d, size) == -2
        for bad in (-1, 4, 1 << 20):
            assert run((ctypes.c_int * 1)(bad), 1, prm(), d, size) == -2, bad
        assert run((ctypes.c_int * 1)(3), 1, prm(), d, size) == -2        # never filled
        assert run((ctypes.c_int * 2)(0, 3), 2, prm(), d, size) == -2
        for bad in (dict(stage=-1), dict(stage=2), dict(layout=-1), dict(layout=2), dict(order=-1), dict(order=2), dict(dtype=-1), dict(dtype=3),
                    dict(nfreq=0), dict(nfreq=17), dict(nfreq=-4), dict(planes=0), dict(planes=16), dict(planes=31), dict(planes=1 << 31),
                    dict(layout=1, nfreq=4), dict(layout=1, nfreq=15), dict(layout=1, nfreq=16, order=1)):
            assert L.vp8hip_coef_size(ctx.h, ctypes.byref(prm(**bad))) == 0, bad
            assert run(slots, 3, prm(**bad), d, 1 << 20) == -2, bad
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
            _, want = C.arrange(blocks[k]["dequant"], hdrs[k], "channels", ("y", "y2"), 4)
            assert a[k * size:(k + 1) * size].tobytes() == want.tobytes()
        assert (a[3 * size:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        for bad in (dict(dtype=torch.int8), dict(stage="idct"), dict(layout="nhwc"), dict(order="morton"), dict(planes=("y", "a")), dict(planes=()),
                    dict(nfreq=0), dict(nfreq=17), dict(layout="inplace", nfreq=8), dict(layout="inplace", order="zigzag"), dict(scale=(1.0, 2.0, 3.0)),
                    dict(out=torch.empty((2, 7), dtype=torch.int16, device="cuda:0")), dict(out=torch.empty((1, 16 * 24 * 63), dtype=torch.float32, device="cuda:0")),
                    dict(out=torch.empty((1, 2 * 16 * 24 * 63), dtype=torch.int16, device="cuda:0")[:, ::2])):
            with pytest.raises(ValueError):
                ctx.frames_coef([0], **bad)
        with pytest.raises(RuntimeError):
            ctx.frames_coef([3])
        ctx.sync()
        assert (big.cpu().numpy()[3 * size:] == 0x5C).all()
    finally:
        prod.close()


def test_no_new_device_memory(pkg):
    """the call reads slots only: no field of memory_usage changes"""
    P = pkg
    n = 4
    prod = Producer(P, "p_odd_130x98", "host", nslots=n)
    ctx = prod.ctx
    try:
        hdrs = [prod.put(i, i) for i in range(n)]
        ctx.sync()
        before = ctx.memory_usage()
        blocks = slot_blocks(ctx, n - 1, hdrs[n - 1])
        for stage, layout, nfreq, order, dtype in (("dequant", "channels", 16, "raster", "i16"), ("levels", "channels", 6, "zigzag", "f32"),
                                                   ("dequant", "inplace", 16, "raster", "f16")):
            got = call(ctx, list(range(n)), stage, layout, ALL, nfreq, order, dtype, 0.5)
            want, _ = C.arrange(blocks[stage], hdrs[n - 1], layout, ALL, nfreq, order, dtype, (0.5,) * 4)
            for name in want:
                assert np.array_equal(bits(got[name][n - 1].cpu().numpy(), dtype), bits(want[name], dtype)), (stage, layout, name)
        ctx.sync()
        assert ctx.memory_usage() == before
    finally:
        prod.close()
