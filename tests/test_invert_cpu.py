"""CPU: the definition of a trace's inverse and of the cover tensor (vp8hip_trace_invert_async, vp8hip_trace_cover_async,
include/vp8hip.h) as tests/invert_reference.py restates it -- against a brute-force double loop, its properties on the fixtures'
chained traces, the tensor and the library's size function."""
import ctypes
import os
import re

import numpy as np
import pytest

import invert_reference as I
import trace_reference as R
from tensor_reference import grid_map
from trace_testlib import chain, frames_of, random_trace


def brute(t, w, h):
    """the definition, pixel by pixel in raster order"""
    first = np.full((h, w), 0xffffffff, np.uint32)
    count = np.zeros((h, w), np.uint32)
    for y in range(h):
        for x in range(w):
            d = int(t[y, x])
            tx, ty = d & 0xffff, d >> 16
            tx, ty = tx - 65536 * (tx >> 15), ty - 65536 * (ty >> 15)
            ax, ay = min(max(tx, 0), w - 1), min(max(ty, 0), h - 1)
            first[ay, ax] = min(int(first[ay, ax]), y << 16 | x)
            count[ay, ax] += 1
    return first, count


@pytest.mark.parametrize("size", [(16, 16), (20, 4)])
def test_reference_against_the_double_loop(size):
    w, h = size
    rng = np.random.default_rng(w * 31 + h)
    traces = [R.identity(w, h), np.full((h, w), R.pack(w - 1, 2), np.uint32), random_trace(rng, w, h),
              rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32),                          # every position clamped, most far outside
              R.pack(rng.integers(-3, w + 3, (h, w)), rng.integers(-3, h + 3, (h, w)))]    # a few pixels past every edge
    for k, t in enumerate(traces):
        first, count = I.invert(t, w, h)
        bf, bc = brute(t, w, h)
        assert first.dtype == np.uint32 and count.dtype == np.uint32 and first.shape == (h, w) == count.shape
        assert np.array_equal(first, bf) and np.array_equal(count, bc), (size, k)
    first, count = I.invert(traces[1], w, h)
    assert count[2, w - 1] == w * h and count.sum() == w * h and first[2, w - 1] == 0 and (first.ravel() != 0xffffffff).sum() == 1


@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98"])
def test_properties_on_chained_traces(pkg, name):
    P = pkg
    frames = frames_of(P, name)
    w, h = int(frames[0][0].width), int(frames[0][0].height)
    ident = R.identity(w, h)
    empties = several = 0
    for i, t in enumerate(chain(frames)):
        first, count = I.invert(t, w, h)
        assert int(count.sum(dtype=np.int64)) == w * h, i
        seen = count > 0
        assert np.array_equal(first == 0xffffffff, ~seen), i               # FIRST is "none" exactly where COUNT is 0
        # a(FIRST(a)) == a wherever COUNT > 0: the first descendant's trace names the anchor pixel
        fx, fy = R.unpack(first[seen])
        assert (fx >= 0).all() and (fx < w).all() and (fy >= 0).all() and (fy < h).all()
        ax, ay = R.clamped(t[fy, fx], w, h)
        ys, xs = np.nonzero(seen)
        assert np.array_equal(ax, xs) and np.array_equal(ay, ys), i
        if frames[i][0].frame_type == 0:
            assert np.array_equal(t, ident)
        empties += int((~seen).sum())
        several += int((count > 1).sum())
    assert empties > 0 and several > 0
    first, count = I.invert(ident, w, h)                                 # an identity trace inverts to itself with COUNT 1
    assert np.array_equal(first, ident) and (count == 1).all()


def test_tensor_restatement():
    rng = np.random.default_rng(12)
    w, h = 130, 98
    count = rng.choice(np.array([0, 0, 1, 2, 7, 254, 255, 256, 400, 12740], np.uint32), (h, w))
    full = I.tensor(count)
    assert full.shape == (2, h, w) and full.dtype == np.uint8
    assert np.array_equal(full[0], np.minimum(count, 255)) and np.array_equal(full[1], count != 0)
    assert full[0].max() == 255 and (count > 255).any()
    for planes, which in ((("seen",), [1]), (("seen", "count"), [0, 1]), (1, [0]), (3, [0, 1])):
        assert np.array_equal(I.tensor(count, planes=planes), full[which])
    for gw, gh in ((224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h)):
        got = I.tensor(count, gw, gh)
        sx, sy = grid_map(gw, w), grid_map(gh, h)
        for y, x in ((0, 0), (gh - 1, gw - 1), (gh // 2, gw // 3)):
            assert got[0, y, x] == min(int(count[sy[y], sx[x]]), 255) and got[1, y, x] == (count[sy[y], sx[x]] != 0)
        assert got.nbytes == I.tensor_size(w, h, gw, gh)
    sc = (np.float32(1.0 / 255), np.float32(-0.5))
    f32 = I.tensor(count, 33, 7, dtype="f32", scale=sc)
    u8 = I.tensor(count, 33, 7)
    assert f32.dtype == np.float32 and np.array_equal(f32[0], (u8[0].astype(np.float64) * np.float64(sc[0])).astype(np.float32))
    assert np.array_equal(f32[1], np.where(u8[1] != 0, np.float32(-0.5), np.float32(0.0)))
    f16 = I.tensor(count, 33, 7, dtype="f16", scale=sc)
    assert f16.dtype == np.float16 and np.array_equal(f16, f32.astype(np.float16))


def test_size_function_of_the_library(pkg):
    P = pkg
    L = P.load_hip()

    def lib(w, h, dtype=0, planes=3):
        return int(L.vp8hip_trace_cover_size(None, ctypes.byref(P.TraceCoverParams(w, h, dtype, planes))))
    count = np.zeros((3, 7), np.uint32)
    for w, h in ((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3)):
        for dt, name in enumerate(("u8", "f16", "f32")):
            for planes in (3, 1, 2):
                assert lib(w, h, dt, planes) == I.tensor_size(7, 3, w, h, planes, name), (w, h, name, planes)
                assert P.trace_cover_size(w, h, planes, dt) == lib(w, h, dt, planes)
    for dt, name in enumerate(("u8", "f16", "f32")):
        for planes in (3, ("seen",), ("count",)):
            for gw, gh in ((7, 3), (10, 4), (1, 1)):
                assert P.trace_cover_size(gw, gh, planes, dt) == I.tensor(count, gw, gh, planes, name).nbytes
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (0, 0)):       # (0 x 0: the display size needs a context)
        assert lib(w, h) == 0, (w, h)
    for dt in (-1, 3):
        assert lib(8, 8, dt) == 0
    for planes in (0, 4, 7, 1 << 31):
        assert lib(8, 8, 0, planes) == 0, planes
    assert L.vp8hip_trace_cover_size(None, None) == 0
    assert P.trace_cover_size(8, 8, ("seen", "count"), "float16") == 2 * 64 * 2 and P.trace_cover_size(8, 8, ("nope",)) == 0
    assert P.trace_cover_size(8, 8, (), 0) == 0 and P.trace_cover_size(8, 8, 3, "int16") == 0 and P.trace_cover_size(0, 0) == 0
    assert P.trace_cover_size(8, 8, 4) == 0
    # the structs as the header lays them out
    assert ctypes.sizeof(P.TraceCoverParams) == 24
    assert [f[0] for f in P.TraceCoverParams._fields_] == ["dst_w", "dst_h", "dtype", "planes", "scale"]
    assert ctypes.sizeof(P.InvertJob) == 8 and [f[0] for f in P.InvertJob._fields_] == ["trace", "dst"]
    assert P.COVER_PLANES == I.PLANES


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vp8hip.h")
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_trace_invert_async", "vp8hip_trace_cover_size", "vp8hip_trace_cover_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert re.search(r"#define\s+VP8HIP_COVER_COUNT\s+1\b", src) and re.search(r"#define\s+VP8HIP_COVER_SEEN\s+2\b", src)
    assert re.search(r"typedef struct vp8hip_invert_job\s*{\s*int32_t trace;\s*int32_t dst;\s*}", src)
