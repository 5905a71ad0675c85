"""GPU (-m gpu): decoded frames scaled into device memory as libyuv's I420Scale scales them (vp8hip_frames_scale_async,
Vp8Hip.frames_scaled; csrc/hip/vp8_scale.hip).  The listings the reference tree's own scaler wrote (tests/golden/*.scale_*.md5)
are reproduced from frames left as tiles and from raster frames; other sizes are checked against the numpy restatement
(tests/scale_reference.py).  torch is imported here, before the package loads libvp8hip.so: one HIP runtime per process."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import GOLDEN, ROOT, golden_md5, md5_list, oracle_decode_ivf, synth_ir
from vp8_writer import write_key_frame
from handover_testlib import assert_destinations_refused, assert_guards_intact, decode_stream, guarded, large_launch
import scale_reference as S

pytestmark = pytest.mark.gpu

CASE = re.compile(r"(.+)\.scale_(\d+)x(\d+)_f(\d)\.md5$")


def listings():
    out = {}
    for f in sorted(os.listdir(GOLDEN)):
        m = CASE.match(f)
        if m:
            out.setdefault(m.group(1), []).append((int(m.group(2)), int(m.group(3)), int(m.group(4)),
                                                   [l.split()[0] for l in open(os.path.join(GOLDEN, f))]))
    return out


def md5s(t):
    a = t.cpu().numpy()
    return [hashlib.md5(a[i].tobytes()).hexdigest() for i in range(a.shape[0])]


@pytest.mark.parametrize("form", ["tiles", "raster"])
@pytest.mark.parametrize("name", sorted(listings()))
def test_listings_from_both_forms(pkg, monkeypatch, name, form):
    P = pkg
    ctx, shown = decode_stream(P, name, form, monkeypatch)
    try:
        before = ctx.memory_usage()
        for dw, dh, flt, gold in listings()[name]:
            for f in ((flt,) if flt == 0 else (1, 2)):
                got = md5s(ctx.frames_scaled(shown, dw, dh, f))
                assert got == gold, f"{name} {dw}x{dh} f{f} from {form}: frames {[i for i, (a, b) in enumerate(zip(got, gold)) if a != b][:8]}"
        # in reverse order, repeated: any list of frame buffers
        got = md5s(ctx.frames_scaled(shown[::-1] + shown[:1], None, None, 0))
        assert got == (golden_md5(name)[::-1] + golden_md5(name)[:1])
        after = ctx.memory_usage()
        assert after["raster_pool"] == before["raster_pool"] and after["packed_staging"] == before["packed_staging"]
        if form == "tiles" and name.startswith("kf_"):
            assert after["raster_pool"] == 0           # read as tiles: no raster form was made
        assert md5_list(ctx, shown) == golden_md5(name)
    finally:
        ctx.close()


def test_large_launch_batch(pkg, monkeypatch):
    P = pkg
    n = 1024
    _, kept = oracle_decode_ivf("kf_1920x1080", keep_frames=True)
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, "kf_1920x1080", n, monkeypatch)
        for dw, dh in ((960, 540), (224, 224)):
            want = [hashlib.md5(S.scale_frame(buf, P.geom(hdr.width, hdr.height), hdr.width, hdr.height, dw, dh, 1).tobytes()).hexdigest()
                    for hdr, _, _, _, buf in kept]
            got = md5s(ctx.frames_scaled(list(range(n)), dw, dh, 1))
            assert got == [want[i % nsrc] for i in range(n)], (dw, dh)
        assert ctx.memory_usage()["raster_pool"] == 0
    finally:
        ctx.close()


SIZES = [(16, 16), (17, 9), (1, 1), (2, 2), (67, 45), (64, 48), (130, 98), (96, 40), (33, 130), (176, 144)]


def _targets(w, h, rng):
    c = [(w, h), (1, 1), (2 * w, 2 * h), (max(1, w // 2), max(1, h // 2)), (max(1, w // 4), max(1, h // 4)), (max(1, 3 * w // 4), max(1, 3 * h // 4)),
         (max(1, 3 * w // 8), max(1, (3 * h + 7) // 8)), (max(1, w // 8), max(1, h // 8)), (w + 1, max(1, h - 1)), (max(1, w - 3), 2 * h)]
    c += [(int(rng.integers(1, 2 * w + 2)), int(rng.integers(1, 2 * h + 2))) for _ in range(3)]
    return c


def test_random_sweep(pkg):
    P = pkg
    rng = np.random.default_rng(2024)
    ran = []
    for w, h in SIZES:
        ctx = P.Vp8Hip(0)
        try:
            try:
                ctx.configure(w, h, 5, 1)
            except RuntimeError:
                if (w, h) in ((1, 1), (2, 2)):
                    continue                               # (the only sizes configure may refuse)
                raise
            ran.append((w, h))
            g = ctx.g
            bufs = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
            for i, b in enumerate(bufs):
                ctx.upload_frame(i, b)
            fbs = [2, 0, 3, 2, 1]
            for dw, dh in _targets(w, h, rng):
                for f in (0, 1, 2):
                    got = ctx.frames_scaled(fbs, dw, dh, f).cpu().numpy()
                    for k, fb in enumerate(fbs):
                        want = S.scale_frame(bufs[fb], g, w, h, dw, dh, f)
                        assert np.array_equal(got[k], want), (w, h, dw, dh, f, k, S.plan(w, h, dw, dh, f))
        finally:
            ctx.close()
    assert len(ran) >= len(SIZES) - 2, ran


def test_widest_planes_read_the_frame(pkg):
    """a plane whose source rows for one output row do not fit in LDS (Down4 filtered at 16376 wide: 4 rows of 16400 bytes) is read
    from the frame buffer directly; its chroma (8188 wide) goes through LDS"""
    P = pkg
    w, h = 16376, 16
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, 2, 1)
        buf = np.random.default_rng(9).integers(0, 256, ctx.g.frame_size, dtype=np.uint8)
        ctx.upload_frame(0, buf)
        for dw, dh, f in ((4094, 4, 1), (4094, 4, 0), (1000, 3, 1)):
            got = ctx.frames_scaled([0, 0], dw, dh, f).cpu().numpy()
            want = S.scale_frame(buf, ctx.g, w, h, dw, dh, f)
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), (dw, dh, f, S.plan(w, h, dw, dh, f))
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
        for dw, dh, f in ((320, 180, 1), (224, 224, 1), (480, 270, 0), (240, 135, 1), (1000, 500, 1)):
            got = ctx.frames_scaled(fbs, dw, dh, f).cpu().numpy()
            for k, fb in enumerate(fbs):
                assert np.array_equal(got[k], S.scale_frame(srcs[fb], g, 640, 360, dw, dh, f)), (dw, dh, f, k)
    finally:
        ctx.close()


def test_synthetic_5200_wide_down8_point_fallback(pkg):
    """Down8 with more than 640 output pixels point-samples even when asked to filter (kMaxOutputWidth)"""
    P = pkg
    w, h = 5200, 64
    hdr, mbs, coef, _ = synth_ir(w, h, 11, inter=False)
    data = write_key_frame(hdr, mbs, coef)
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 2, 1)
        hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
        ctx.decode([(0, 0, None)], P.STAGE_ALL)
        ctx.sync()
        buf = ctx.download_full(0)
        assert S.plan(w, h, 650, 8, 1) == ("down8", "down8")
        got = ctx.frames_scaled([0], 650, 8, 1).cpu().numpy()[0]
        assert np.array_equal(got, S.scale_frame(buf, ctx.g, w, h, 650, 8, 1))
        # luma (650 > 640 wide) is the point-sampled bytes; chroma (325 wide) filters
        assert np.array_equal(got[:650 * 8], S.scale_frame(buf, ctx.g, w, h, 650, 8, 0)[:650 * 8])
        assert not np.array_equal(got[650 * 8:], S.scale_frame(buf, ctx.g, w, h, 650, 8, 0)[650 * 8:])
    finally:
        parser.close()
        ctx.close()


@pytest.mark.parametrize("form", ["tiles", "raster"])
def test_destination_hygiene(pkg, monkeypatch, form):
    P = pkg
    ctx, shown = decode_stream(P, "kf_odd_67x45", form, monkeypatch)
    try:
        for dw, dh, gold_name in ((67, 45, None), (34, 23, "kf_odd_67x45.scale_34x23_f1.md5"), (200, 150, "kf_odd_67x45.scale_200x150_f1.md5")):
            size = S.i420_size(dw, dh)
            n, pad, off = len(shown), 37, 3
            big, out = guarded(n, size, pad, off)
            assert out.stride(0) == size + pad and out.data_ptr() % 2 == 1
            r = ctx.frames_scaled(shown, dw, dh, 1, out=out)
            assert r.data_ptr() == out.data_ptr()
            want = golden_md5("kf_odd_67x45") if gold_name is None else [l.split()[0] for l in open(os.path.join(GOLDEN, gold_name))]
            assert md5s(out) == want
            assert_guards_intact(big, n, size, pad, off, what=(dw, dh))
    finally:
        ctx.close()


def test_ordering_against_later_launches(pkg, monkeypatch):
    """scale, then at once decode other frames into the same frame buffers, then read the tensor on torch's stream: no sync"""
    P = pkg
    n = 10
    gold = [l.split()[0] for l in open(os.path.join(GOLDEN, "kf_640x360.scale_240x135_f1.md5"))]
    ctx = P.Vp8Hip(0)
    try:
        large_launch(P, ctx, "kf_640x360", n, monkeypatch)
        out = ctx.frames_scaled(list(range(n)), 240, 135, 1)
        ctx.decode([(i, (i + 1) % n, None) for i in range(n)], P.STAGE_ALL)     # frame i into frame buffer i + 1
        assert md5s(out) == gold                          # .cpu() on torch's current stream
        ctx.sync()
        assert md5s(ctx.frames_scaled(list(range(n)), 240, 135, 1)) == [gold[(i - 1) % n] for i in range(n)]
    finally:
        ctx.close()


def test_refusals(pkg, monkeypatch):
    P = pkg
    ctx, shown = decode_stream(P, "kf_odd_67x45", "raster", monkeypatch)
    L = ctx.L
    try:
        size = S.i420_size(34, 23)
        big = torch.full((1 << 22,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d = big.data_ptr()
        fbs = (ctypes.c_int * 3)(*shown)

        def call(fb_arr, n, w, h, f, dst, stride):
            return L.vp8hip_frames_scale_async(ctx.h, fb_arr, n, w, h, f, ctypes.c_void_p(dst), stride)
        assert call(fbs, 0, 34, 23, 1, d, size) == -2
        assert call((ctypes.c_int * 1)(-1), 1, 34, 23, 1, d, size) == -2
        assert call((ctypes.c_int * 1)(ctx.num_fb), 1, 34, 23, 1, d, size) == -2
        for w, h in ((0, 23), (34, 0), (16384, 2), (2, 16384), (-3, 5)):
            assert call(fbs, 3, w, h, 1, d, size) == -2, (w, h)
        for f in (-1, 3, 7):
            assert call(fbs, 3, 34, 23, f, d, size) == -2
        assert_destinations_refused(ctx, lambda n, dst, stride: call(fbs, n, 34, 23, 1, dst, stride), d, size, 1)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                              # nothing was enqueued
        # ... and the same call into memory the test owns is accepted: three frames at the start of `big`, nothing else written
        assert call(fbs, 3, 34, 23, 1, d, size) == 0
        ctx.sync()
        a = big.cpu().numpy()
        gold = [l.split()[0] for l in open(os.path.join(GOLDEN, "kf_odd_67x45.scale_34x23_f1.md5"))]
        assert [hashlib.md5(a[i * size:(i + 1) * size].tobytes()).hexdigest() for i in range(3)] == gold
        assert (a[3 * size:] == 0x5C).all()
    finally:
        ctx.close()


def test_torch_after_library_is_refused():
    """frames_scaled refuses when libvp8hip.so was loaded before torch (two HIP runtimes): a fresh interpreter"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from vp8_testlib import load_package\n"
            "P = load_package(); ctx = P.Vp8Hip(0); ctx.configure(64, 48, 2, 1)\n"
            "import torch\n"
            "try:\n    ctx.frames_scaled([0], 32, 24)\nexcept RuntimeError as e:\n    print('refused', 'import torch before' in str(e))\n"
            "ctx.close()\n") % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "refused True" in r.stdout, r.stdout + r.stderr
