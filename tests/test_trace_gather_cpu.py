"""CPU: the definition of the gather along the trace (vp8hip_trace_gather_async, include/vp8hip.h) as tests/trace_gather_reference.py
restates it -- against numpy's fancy indexing at the display size, the header's stated properties of the cell maps, the bilinear
weights on ramps, what is already pinned to the oracle decoder (the accumulated residual of whole streams), and the library's size
function and structs."""
import ctypes
import os
import re

import numpy as np
import pytest

from vp8_testlib import oracle_decode_ivf
import rgb_reference as RGB
import scale_reference as S
import trace_reference as T
import trace_residual_reference as R
import trace_gather_reference as G
from trace_testlib import chain, frames_of

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vp8hip.h")


def wild_trace(rng, w, h):
    """positions over all of int16: most of them clamped"""
    return T.pack(rng.integers(-32768, 32768, (h, w)), rng.integers(-32768, 32768, (h, w)))


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45)])
def test_display_size_is_fancy_indexing(size):
    w, h = size
    rng = np.random.default_rng(w * 11 + h)
    for dtype, C in ((np.uint8, 1), (np.int16, 5), (np.float32, 3)):
        src = rng.integers(0, 200, (C, h, w)).astype(dtype)
        for t in (T.pack(rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w))), wild_trace(rng, w, h), T.identity(w, h)):
            ax, ay = T.clamped(t, w, h)
            got = G.nearest(src, t, w, h)
            assert got.dtype == src.dtype and got.shape == (C, h, w) and np.array_equal(got, src[:, ay, ax])
            # another output size: the display-size result under each output's centre
            for gw, gh in ((1, 1), (224, 224), (45, 67)):
                sx, sy = G.grid_map(gw, w), G.grid_map(gh, h)
                assert np.array_equal(G.nearest(src, t, w, h, gw, gh), src[:, ay, ax][:, sy[:, None], sx[None, :]])
    assert np.array_equal(G.nearest(src, T.identity(w, h), w, h), src)


def test_cells_of_strided_and_other_grids():
    # a stride that divides the display width: the cell is ax // s
    for d in (352, 288):
        a = np.arange(d)
        for s in (2, 4, 8, 16, 32):
            assert np.array_equal(G.nearest_cell(a, d // s, d), a // s), (d, s)
    # smaller, equal and larger source grids: monotone and inside the grid; every cell is taken where there are pixels enough for
    # that (d pixels cannot name more than d cells: on the larger grid they name d different ones)
    for d, grids in ((130, (7, 130, 261)), (98, (5, 98, 197))):
        a = np.arange(d)
        for s in grids:
            cx = G.nearest_cell(a, s, d)
            assert (np.diff(cx) >= 0).all() and cx.min() >= 0 and cx.max() <= s - 1, (d, s)
            assert set(cx.tolist()) == set(range(s)) if s <= d else len(set(cx.tolist())) == d, (d, s)
            x0, x1, wx, px = G.bilinear_cell(a, s, d)
            assert (np.diff(px) >= 0).all() and px.min() >= 0 and px.max() <= (s - 1) * 256 and x1.max() == s - 1
            assert ((x1 == x0) <= (wx == 0)).all()           # a clamped neighbour carries no weight
    assert np.array_equal(G.nearest_cell(np.arange(130), 130, 130), np.arange(130))


def test_bilinear_weights():
    w, h = 130, 98
    rng = np.random.default_rng(130)
    t = wild_trace(rng, w, h)
    t[:4] = T.pack(rng.integers(0, w, (4, w)), rng.integers(0, h, (4, w)))
    # the source grid is the display's: no weight off the first corner, R is the nearest cell's value exactly
    for dtype in (np.float16, np.float32):
        src = rng.uniform(-1000, 1000, (3, h, w)).astype(dtype)
        _, _, wx, _ = G.bilinear_cell(np.arange(w), w, w)
        _, _, wy, _ = G.bilinear_cell(np.arange(h), h, h)
        assert not wx.any() and not wy.any()
        Rv, M = G.bilinear(src, t, w, h)
        near = G.nearest(src, t, w, h)
        assert np.array_equal(Rv.astype(dtype).view(np.uint16 if dtype == np.float16 else np.uint32),
                              near.view(np.uint16 if dtype == np.float16 else np.uint32))
        assert (M >= np.abs(Rv)).all()
    # a ramp alpha * cx + beta * cy comes out as alpha * px / 256 + beta * py / 256: clamped edges included
    alpha, beta = 3.0, -0.5
    for sw, sh in ((7, 5), (33, 25), (261, 197), (130, 98)):
        ys, xs = np.mgrid[0:sh, 0:sw]
        src = (alpha * xs + beta * ys).astype(np.float32)[None]
        for gw, gh in ((0, 0), (45, 67)):
            Rv, M = G.bilinear(src, t, w, h, gw, gh)
            ax, ay = G.anchor_positions(t, w, h, gw, gh)
            px, py = G.bilinear_cell(ax, sw, w)[3], G.bilinear_cell(ay, sh, h)[3]
            want = alpha * px / 256.0 + beta * py / 256.0
            assert (np.abs(Rv[0] - want) <= G.bound(want, M[0], np.float32)).all(), (sw, sh, gw, gh)
            if sw < w:                                       # (the clamp of px bites on grids smaller than the display only)
                assert px.min() == 0 and px.max() == (sw - 1) * 256 and py.min() == 0 and py.max() == (sh - 1) * 256
    # the bound: what it is at M = 1000
    assert G.bound(np.float64(0.0), np.float64(1000.0), np.float32) == 8 * 2.0 ** -24 * 1000
    assert G.bound(np.float64(2.0), np.float64(4.0), np.float16) == 8 * 2.0 ** -24 * 4 + 2.0 ** -11 * 2 + 2.0 ** -25


@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98", "p_split_352x288"])
def test_pinned_to_the_accumulated_residual(pkg, name):
    """every frame of a stream as the oracle decodes it, its trace by trace_reference over the parsed IR: the anchor's RGB bytes
    gathered at the trace are the frame's RGB bytes minus the accumulated residual, element for element"""
    P = pkg
    frames = frames_of(P, name)
    traces = chain(frames)
    _, kept = oracle_decode_ivf(name, keep_frames=True)
    assert len(kept) == len(frames)
    w, h = frames[0][0].width, frames[0][0].height
    g = P.geom(w, h)
    anchor = None
    moved = 0
    for (hdr, *_), t, k in zip(frames, traces, kept):
        packed = S.scale_frame(k[4], g, w, h, w, h, 0)
        if hdr.frame_type == 0:
            anchor = packed
        rgb_a = RGB.convert(anchor, w, h)
        assert rgb_a.dtype == np.uint8 and rgb_a.shape == (3, h, w)
        got = G.nearest(rgb_a, t, w, h)
        want = RGB.convert(packed, w, h).astype(np.int64) - R.residual(packed, anchor, t, w, h, dtype="i16")
        assert np.array_equal(got, want), name
        moved += bool((t != T.identity(w, h)).any())
    assert moved > len(frames) // 2


def header_struct(name):
    """the int / int32_t fields of `typedef struct name { ... } name;` in include/vp8hip.h, in order"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype in ("int", "int32_t"), decl
            fields += [n.strip() for n in names.split(",")]
    return fields


def test_size_function_and_structs_of_the_library(pkg):
    P = pkg
    L = P.load_hip()
    assert [f[0] for f in P.TraceGatherParams._fields_] == header_struct("vp8hip_trace_gather")
    assert [f[0] for f in P.GatherJob._fields_] == header_struct("vp8hip_gather_job")
    assert ctypes.sizeof(P.TraceGatherParams) == 32 and ctypes.sizeof(P.GatherJob) == 8
    assert all(getattr(P.TraceGatherParams, f).size == 4 for f, _ in P.TraceGatherParams._fields_)
    assert P.GATHER_FILTERS == {"nearest": 0, "bilinear": 1} and P.GATHER_LAYOUTS == {"planar": 0, "channels_last": 1}

    def lib(gw, gh, C=3, elem=2, sw=8, sh=8, layout=0, filt=0):
        return int(L.vp8hip_trace_gather_size(None, ctypes.byref(P.TraceGatherParams(gw, gh, sw, sh, C, elem, layout, filt))))
    for gw, gh in ((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3)):
        for C, elem in ((1, 1), (21, 1), (5, 2), (64, 2), (4096, 4)):
            for layout in (0, 1):
                assert lib(gw, gh, C, elem, layout=layout) == G.size(0, 0, C, elem, gw, gh) == C * gh * gw * elem
                assert P.trace_gather_size(gw, gh, C, elem, layout=("planar", "channels_last")[layout]) == C * gh * gw * elem
                assert lib(gw, gh, C, elem, layout=layout, filt=1) == (0 if elem == 1 else C * gh * gw * elem)
    assert lib(16383, 16383, 4096, 4) == 4096 * 16383 * 16383 * 4 > 1 << 32
    for gw, gh in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (0, 0)):     # (0 x 0: the display size needs a context)
        assert lib(gw, gh) == 0 and P.trace_gather_size(gw, gh, 3, 2) == 0, (gw, gh)
    for sw, sh in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, 4)):
        assert lib(8, 8, sw=sw, sh=sh) == 0 and P.trace_gather_size(8, 8, 3, 2, sw, sh) == 0, (sw, sh)
    assert lib(8, 8, sw=16383, sh=1) == lib(8, 8, sw=1, sh=16383) == 3 * 64 * 2
    for C in (0, -1, 4097):
        assert lib(8, 8, C=C) == 0
    for elem in (0, 3, 8, -2):
        assert lib(8, 8, elem=elem) == 0
    for bad in (-1, 2):
        assert lib(8, 8, layout=bad) == 0 and lib(8, 8, filt=bad) == 0
    assert P.trace_gather_size(8, 8, 3, 2, layout="nhwc") == 0 and P.trace_gather_size(8, 8, 3, 2, filter="cubic") == 0
    assert P.trace_gather_size(8, 8, 3, 1, filter="bilinear") == 0 and P.trace_gather_size(8, 8, 3, 4, filter="bilinear") == 3 * 64 * 4
    assert L.vp8hip_trace_gather_size(None, None) == 0
