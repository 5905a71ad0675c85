"""GPU (-m gpu): decoded frames as RGB tensors in device memory (vp8hip_frames_rgb_async, Vp8Hip.frames_rgb; csrc/hip/vp8_rgb.hip),
bit for bit against the numpy restatement (tests/rgb_reference.py = the colour arithmetic of include/vp8hip.h applied to
tests/scale_reference.py's I420Scale), from frames left as tiles and from raster frames.  torch is imported here, before the
package loads libvp8hip.so: one HIP runtime per process."""
import ctypes
import itertools

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import load_package, oracle_decode_ivf
from handover_testlib import (TORCH_DTYPE, assert_destinations_refused, assert_guards_intact, bits, decode_stream, equal_on_device, guarded,
                              large_launch)
import rgb_reference as R
import scale_reference as S

pytestmark = pytest.mark.gpu

PY_LAYOUT = {"planar": "nchw", "packed3": "nhwc", "packed4": "nhwc4"}
# every matrix x layout x order for bytes; every float type for the planar and the three-channel packed layout
U8_COMBOS = [(m, l, o, "u8") for m in R.MATRICES for l in R.LAYOUTS for o in R.ORDERS]
FLOAT_COMBOS = [("bt601", l, o, d) for l, o in (("planar", "rgb"), ("packed3", "bgr")) for d in ("f16", "f32")]
COMBOS = U8_COMBOS + FLOAT_COMBOS


def call(ctx, fbs, dw, dh, filt, combo, **kw):
    matrix, layout, order, dtype = combo
    norm = dict(mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD) if dtype != "u8" else {}
    return ctx.frames_rgb(fbs, dw, dh, filt, dtype=TORCH_DTYPE[dtype], layout=PY_LAYOUT[layout], order=order, matrix=matrix, **norm, **kw)


def want(packed, dw, dh, combo):
    matrix, layout, order, dtype = combo
    scale, bias = R.scale_bias(R.IMAGENET_MEAN, R.IMAGENET_STD) if dtype != "u8" else R.scale_bias()
    return R.convert(packed, dw, dh, matrix, layout, order, dtype, scale, bias)


def shown_buffers(name):
    """(geometry, w, h, frame buffer) of every shown frame, from the oracle"""
    P = load_package()
    _, kept = oracle_decode_ivf(name, keep_frames=True)
    return [(P.geom(hdr.width, hdr.height), hdr.width, hdr.height, buf) for hdr, _, _, _, buf in kept if hdr.show_frame]


@pytest.mark.parametrize("form", ["tiles", "raster"])
@pytest.mark.parametrize("name", ["kf_odd_67x45", "p_odd_130x98", "kf_640x360"])
def test_fixtures_from_both_forms(pkg, monkeypatch, name, form):
    P = pkg
    frames = shown_buffers(name)
    ctx, shown = decode_stream(P, name, form, monkeypatch)
    try:
        assert len(shown) == len(frames)
        w, h = ctx.width, ctx.height
        before = ctx.memory_usage()
        for dw, dh, filt in ((w, h, 1), (max(1, w // 2), max(1, h // 2), 1), (w * 3 // 2 + 1, h + 3, 1)):
            packed = [S.scale_frame(buf, g, w, h, dw, dh, filt) for g, _, _, buf in frames]
            for combo in COMBOS:
                got = call(ctx, shown, dw, dh, filt, combo).cpu().numpy()
                for k in range(len(shown)):
                    assert np.array_equal(bits(got[k], combo[3]), bits(want(packed[k], dw, dh, combo), combo[3])), (name, form, dw, dh, combo, k)
        after = ctx.memory_usage()
        assert after["raster_pool"] == before["raster_pool"] and after["packed_staging"] == before["packed_staging"]
        if form == "tiles" and name.startswith("kf_"):
            assert after["raster_pool"] == 0           # read as tiles: no raster form was made
        # the scratch is the only device memory the call adds, and release_staging gives it back
        assert ctx.rgb_scratch_bytes() > 0
        ctx.release_staging()
        assert ctx.rgb_scratch_bytes() == 0
        got = call(ctx, shown, w, h, 1, COMBOS[0]).cpu().numpy()          # the display size needs none
        assert ctx.rgb_scratch_bytes() == 0
        assert np.array_equal(got[0], want(S.scale_frame(frames[0][3], frames[0][0], w, h, w, h, 1), w, h, COMBOS[0]))
    finally:
        ctx.close()


SIZES = [(16, 16), (17, 9), (67, 45), (64, 48), (130, 98), (96, 40), (33, 130), (176, 144)]


def _targets(w, h, rng):
    c = [(w, h), (1, 1), (2 * w, 2 * h), (max(1, w // 2), max(1, h // 2)), (max(1, w // 4), max(1, h // 4)), (max(1, 3 * w // 4), max(1, 3 * h // 4)),
         (max(1, 3 * w // 8), max(1, (3 * h + 7) // 8)), (max(1, w // 8), max(1, h // 8)), (w + 1, max(1, h - 1)), (max(1, w - 3), 2 * h)]
    c += [(int(rng.integers(1, 2 * w + 2)), int(rng.integers(1, 2 * h + 2))) for _ in range(3)]
    return c


def test_random_sweep(pkg):
    """uploaded random frame buffers, the scaler's targets, filters 0 and 1, a list with repeats; the parameter combinations in
    rotation (every one of them many times over the sweep)"""
    P = pkg
    rng = np.random.default_rng(2025)
    combos = itertools.cycle([(m, l, o, d) for m in R.MATRICES for l in R.LAYOUTS for o in R.ORDERS for d in R.DTYPES
                              if not (l == "packed4" and d != "u8")])
    seen = set()
    for w, h in SIZES:
        ctx = P.Vp8Hip(0)
        try:
            ctx.configure(w, h, 5, 1)
            g = ctx.g
            bufs = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
            for i, b in enumerate(bufs):
                ctx.upload_frame(i, b)
            fbs = [2, 0, 3, 2, 1]
            for dw, dh in _targets(w, h, rng):
                for f in (0, 1):
                    packed = [S.scale_frame(b, g, w, h, dw, dh, f) for b in bufs]
                    for _ in range(2):
                        combo = next(combos)
                        seen.add(combo)
                        got = call(ctx, fbs, dw, dh, f, combo).cpu().numpy()
                        for k, fb in enumerate(fbs):
                            assert np.array_equal(bits(got[k], combo[3]), bits(want(packed[fb], dw, dh, combo), combo[3])), \
                                (w, h, dw, dh, f, combo, k, S.plan(w, h, dw, dh, f))
        finally:
            ctx.close()
    assert len(seen) == 3 * 2 * 7


def test_large_launch_batch(pkg, monkeypatch):
    """1024 kf_1920x1080 frames left as tiles by one launch: bytes at the display size, normalised halves at 224x224"""
    P = pkg
    n = 1024
    _, kept = oracle_decode_ivf("kf_1920x1080", keep_frames=True)
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, "kf_1920x1080", n, monkeypatch)
        for dw, dh, combo in ((1920, 1080, ("bt601", "planar", "rgb", "u8")), (224, 224, ("bt601", "planar", "rgb", "f16"))):
            refs = [want(S.scale_frame(buf, P.geom(hdr.width, hdr.height), hdr.width, hdr.height, dw, dh, 1), dw, dh, combo)
                    for hdr, _, _, _, buf in kept[:nsrc]]
            out = call(ctx, list(range(n)), dw, dh, 1, combo)
            assert equal_on_device(out, refs, [i % nsrc for i in range(n)], combo[3]) == [], (dw, dh)
            del out
        assert ctx.memory_usage()["raster_pool"] == 0
    finally:
        ctx.close()


def test_tiled_and_raster_frames_in_one_call(pkg, monkeypatch):
    """frames a large launch left as tiles beside uploaded (raster-only) frames, in one call"""
    P = pkg
    n = 10
    _, kept = oracle_decode_ivf("kf_640x360", keep_frames=True)
    ctx = P.Vp8Hip(0)
    try:
        large_launch(P, ctx, "kf_640x360", n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0
        g = ctx.g
        rnd = np.random.default_rng(3).integers(0, 256, g.frame_size, dtype=np.uint8)
        ctx.upload_frame(n, rnd)                          # raster only (this makes the raster pool; frames 0..n-1 stay tiles)
        fbs = [n, 4, 0, n, 9]
        srcs = {n: rnd, 4: kept[4][4], 0: kept[0][4], 9: kept[9][4]}
        for (dw, dh, f), combo in zip(((640, 360, 1), (320, 180, 1), (224, 224, 1), (480, 270, 0), (1000, 500, 1)),
                                      (COMBOS[0], COMBOS[7], FLOAT_COMBOS[1], COMBOS[14], FLOAT_COMBOS[2])):
            got = call(ctx, fbs, dw, dh, f, combo).cpu().numpy()
            for k, fb in enumerate(fbs):
                ref = want(S.scale_frame(srcs[fb], g, 640, 360, dw, dh, f), dw, dh, combo)
                assert np.array_equal(bits(got[k], combo[3]), bits(ref, combo[3])), (dw, dh, f, combo, k)
    finally:
        ctx.close()


def test_more_frames_than_a_chunk_of_the_scratch(pkg):
    """a target so large that 256 MB of scratch hold fewer frames than the call has: the scratch is reused chunk after chunk"""
    P = pkg
    w, h, dw, dh, n = 64, 48, 4096, 2304, 20
    per = 256 * 2 ** 20 // S.i420_size(dw, dh)
    assert 1 <= per < n
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 3, 1)
        rng = np.random.default_rng(12)
        bufs = [rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8) for _ in range(3)]
        for i, b in enumerate(bufs):
            ctx.upload_frame(i, b)
        combo = ("bt709", "planar", "bgr", "u8")
        refs = [want(S.scale_frame(b, ctx.g, w, h, dw, dh, 0), dw, dh, combo) for b in bufs]
        out = call(ctx, [i % 3 for i in range(n)], dw, dh, 0, combo)
        assert equal_on_device(out, refs, [i % 3 for i in range(n)], "u8") == []
        assert 0 < ctx.rgb_scratch_bytes() <= 256 * 2 ** 20 and ctx.rgb_scratch_bytes() < n * S.i420_size(dw, dh)
        ctx.release_staging()
        assert ctx.rgb_scratch_bytes() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("form", ["tiles", "raster"])
def test_destination_hygiene(pkg, monkeypatch, form):
    """bytes at an odd address with a padded frame stride; halves at a 2-aligned address that is not 4-aligned; aligned starts as
    well (whole-piece stores where the width allows): the sentinel bytes before, between and behind the frames stay"""
    P = pkg
    frames = shown_buffers("kf_odd_67x45")
    ctx, shown = decode_stream(P, "kf_odd_67x45", form, monkeypatch)
    try:
        n = len(shown)
        for (dw, dh), combo, off, pad in itertools.product(((67, 45), (34, 23), (200, 150), (64, 36)),
                                                           (("bt601", "planar", "rgb", "u8"), ("bt601", "packed3", "bgr", "u8"),
                                                            ("bt601", "packed4", "rgb", "u8"), ("bt601", "planar", "rgb", "f16"),
                                                            ("bt601", "packed3", "rgb", "f16")), (3, 2, 0), (37, 0)):
            dtype, layout = combo[3], combo[1]
            es = 1 if dtype == "u8" else 2
            if (off + pad) % es or off % es:
                continue
            size = R.frame_size(dw, dh, layout, dtype)
            big, flat = guarded(n, size, pad, off)
            shape = (3, dh, dw) if layout == "planar" else (dh, dw, 3 if layout == "packed3" else 4)
            out = flat.view(TORCH_DTYPE[dtype]).unflatten(1, shape)
            assert out.data_ptr() % 4 == off and out.stride(0) * es == size + pad
            r = call(ctx, shown, dw, dh, 1, combo, out=out)
            assert r.data_ptr() == out.data_ptr()
            got = out.cpu().numpy()
            for k, (g, w, h, buf) in enumerate(frames):
                assert np.array_equal(bits(got[k], dtype), bits(want(S.scale_frame(buf, g, w, h, dw, dh, 1), dw, dh, combo), dtype)), (dw, dh, combo, k)
            assert_guards_intact(big, n, size, pad, off, what=(dw, dh, combo, off, pad))
    finally:
        ctx.close()


def test_ordering_against_later_launches(pkg, monkeypatch):
    """convert, then at once decode other frames into the same frame buffers, then read the tensor on torch's stream: no sync"""
    P = pkg
    n = 10
    _, kept = oracle_decode_ivf("kf_640x360", keep_frames=True)
    combo = ("bt601", "packed3", "rgb", "u8")
    refs = [want(S.scale_frame(buf, P.geom(640, 360), 640, 360, 240, 135, 1), 240, 135, combo) for _, _, _, _, buf in kept[:n]]
    ctx = P.Vp8Hip(0)
    try:
        large_launch(P, ctx, "kf_640x360", n, monkeypatch)
        out = call(ctx, list(range(n)), 240, 135, 1, combo)
        ctx.decode([(i, (i + 1) % n, None) for i in range(n)], P.STAGE_ALL)     # frame i into frame buffer i + 1
        got = out.cpu().numpy()                           # .cpu() on torch's current stream
        assert all(np.array_equal(got[i], refs[i]) for i in range(n))
        ctx.sync()
        got = call(ctx, list(range(n)), 240, 135, 1, combo).cpu().numpy()
        assert all(np.array_equal(got[i], refs[(i - 1) % n]) for i in range(n))
    finally:
        ctx.close()


def test_refusals(pkg, monkeypatch):
    P = pkg
    frames = shown_buffers("kf_odd_67x45")
    ctx, shown = decode_stream(P, "kf_odd_67x45", "raster", monkeypatch)
    L = ctx.L
    try:
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        assert d % 16 == 0
        fbs = (ctypes.c_int * 3)(*shown)

        def prm(w=34, h=23, filt=1, matrix=0, layout=0, order=0, dtype=0):
            return P.RgbParams(w, h, filt, matrix, layout, order, dtype)

        def run(fb_arr, n, p, dst, stride):
            return L.vp8hip_frames_rgb_async(ctx.h, fb_arr, n, ctypes.byref(p), ctypes.c_void_p(dst), stride)
        size = 34 * 23 * 3
        assert L.vp8hip_rgb_size(ctypes.byref(prm())) == size
        assert run(fbs, 0, prm(), d, size) == -2
        assert run((ctypes.c_int * 1)(-1), 1, prm(), d, size) == -2
        assert run((ctypes.c_int * 1)(ctx.num_fb), 1, prm(), d, size) == -2
        for w, h in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5)):
            assert run(fbs, 3, prm(w, h), d, 1 << 20) == -2, (w, h)
        for bad in (dict(filt=-1), dict(filt=3), dict(matrix=-1), dict(matrix=3), dict(layout=-1), dict(layout=3), dict(order=-1), dict(order=2),
                    dict(dtype=-1), dict(dtype=3), dict(layout=2, dtype=1), dict(layout=2, dtype=2)):
            assert run(fbs, 3, prm(**bad), d, 1 << 20) == -2, bad
        for dtype, es in ((0, 1), (1, 2), (2, 4)):          # bytes; halves and floats: also the alignment to the element
            assert_destinations_refused(ctx, lambda n, dst, stride: run(fbs, n, prm(dtype=dtype), dst, stride), d, size * es, es)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                          # nothing was enqueued
        assert ctx.rgb_scratch_bytes() == 0                               # ... and nothing allocated
        # the same call into memory the test owns is accepted: three frames at the start of `big`, nothing else written
        assert run(fbs, 3, prm(), d, size) == 0
        ctx.sync()
        a = big.cpu().numpy()
        for k, (g, w, h, buf) in enumerate(frames):
            ref = R.convert(S.scale_frame(buf, g, w, h, 34, 23, 1), 34, 23)
            assert a[k * size:(k + 1) * size].tobytes() == ref.tobytes()
        assert (a[3 * size:] == 0x5C).all()
        # the Python wrapper refuses what it can see before the call
        with pytest.raises(ValueError):
            ctx.frames_rgb(shown, 34, 23, layout="nhwc4", dtype=torch.float16)
        with pytest.raises(ValueError):
            ctx.frames_rgb(shown, 34, 23, out=torch.empty((3, 3, 23, 36), dtype=torch.uint8, device="cuda:0")[:, :, :, :34])
    finally:
        ctx.close()


@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
def test_close_to_float_arithmetic_on_the_device(pkg, monkeypatch, matrix):
    """not bit-exact: against torch's float64 arithmetic with the exact matrix, the bound tests/test_rgb_cpu.py establishes (1)"""
    P = pkg
    ctx, shown = decode_stream(P, "kf_640x360", "tiles", monkeypatch)
    try:
        w, h = ctx.width, ctx.height
        got = ctx.frames_rgb(shown, matrix=matrix).to(torch.int32)                       # [n, 3, h, w]
        y, u, v = P.split_i420(ctx.frames_scaled(shown, w, h, 0), w, h)
        yoff, ky, rows = R.exact_matrix(matrix)
        up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w].to(torch.float64) - 128.0
        yf, uf, vf = ky * (y.to(torch.float64) - yoff), up(u), up(v)
        for c in range(3):
            exact = torch.clamp(torch.round(yf + rows[c][0] * uf + rows[c][1] * vf), 0, 255).to(torch.int32)
            assert int((got[:, c] - exact).abs().max()) <= 1, (matrix, c)
    finally:
        ctx.close()
