"""CPU: the definition of the accumulated residual (vp8hip_trace_residual_async, include/vp8hip.h) as tests/trace_residual_reference.py
restates it -- against INTEGRATION's formula written out (the RGB bytes of both frames, a flat gather, a subtraction), axis order and
sign pinned by the oracle decoder on a hand-built frame, the clamp against a loop written out pixel by pixel, and the library's size
function."""
import ctypes

import numpy as np
import pytest

from vp8_testlib import oracle_decode
import rgb_reference as RGB
import scale_reference as S
import trace_reference as T
import trace_residual_reference as R
from trace_testlib import luma, whole_pixel_frame

SIZES = [(16, 16), (17, 33), (67, 45)]


def random_i420(rng, w, h):
    return rng.integers(0, 256, S.i420_size(w, h), dtype=np.uint8)


def rgb_planes(packed, w, h, matrix):
    """[3, h, w] int64, R, G, B: rgb_reference's bytes with the chroma replicated, without its convert()"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    y = packed[:w * h].reshape(h, w)
    u = packed[w * h:w * h + cw * ch].reshape(ch, cw)
    v = packed[w * h + cw * ch:].reshape(ch, cw)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack(RGB.rgb_bytes(y, u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], matrix))


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("matrix", ["bt601", "bt601-full", "bt709"])
@pytest.mark.parametrize("size", SIZES)
def test_matches_the_snippet(size, matrix, order):
    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    cur, anc = random_i420(rng, w, h), random_i420(rng, w, h)
    t = T.pack(rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w)))
    # the snippet: rgb_u8(fb) - rgb_u8(anchor)[:, ay, ax] as a flat gather
    tx, ty = T.unpack(t)
    flat = (ty.astype(np.int64) * w + tx.astype(np.int64)).ravel()
    snippet = rgb_planes(cur, w, h, matrix) - rgb_planes(anc, w, h, matrix).reshape(3, -1)[:, flat].reshape(3, h, w)
    if order == "bgr":
        snippet = snippet[::-1]
    at = R.residual(cur, anc, t, w, h, matrix=matrix, order=order)
    assert at.dtype == np.int16 and at.shape == (3, h, w) and np.array_equal(at, snippet)
    assert snippet.min() < -100 and snippet.max() > 100
    # another size: the display-size result sampled under each output's centre
    for gw, gh in ((224, 224), (w + 1, h - 1), (1, 1), (2 * w + 3, 2 * h)):
        sx, sy = R.grid_map(gw, w), R.grid_map(gh, h)
        got = R.residual(cur, anc, t, w, h, gw, gh, matrix=matrix, order=order)
        assert got.shape == (3, gh, gw) and np.array_equal(got, snippet[:, sy[:, None], sx[None, :]]), (gw, gh)
    # the float types: by colour, not by position
    sc = (0.5, -0.25, 3.0)
    f = R.residual(cur, anc, t, w, h, dtype="f32", matrix=matrix, order=order, scale=sc)
    by_pos = sc[::-1] if order == "bgr" else sc
    assert f.dtype == np.float32 and np.array_equal(f, (snippet * np.asarray(by_pos)[:, None, None]).astype(np.float32))
    assert R.size(w, h, dtype="f32") == f.nbytes and R.size(w, h, 5, 3, "f16") == 3 * 5 * 3 * 2


@pytest.mark.parametrize("size", [(16, 16), (67, 45), (176, 144)])
def test_oracle_pins_axis_order_and_sign(pkg, size):
    """a frame of skipped inter macroblocks with whole-pixel vectors of an even number of pixels, decoded by the oracle from a random
    picture with grey chroma: with the full-range matrix every channel is the luma byte, and the residual against the picture at the
    frame's one-hop trace is 0 at every pixel -- with x and y swapped in the gather it is not"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 131 + h + 1)
    g = P.geom(w, h)
    hdr, mbs, mvs = whole_pixel_frame(P, w, h, rng)
    mvs = ((mvs >> 4) << 4).astype(np.int16)             # an even number of pixels: the chroma vectors are whole too
    mbs[:, T.O_REF] = 1                                 # one reference: the anchor
    pic = rng.integers(0, 256, (h, w)).astype(np.uint8)
    ref = np.full(g.frame_size, 128, np.uint8)
    luma(ref, g, g.aligned_h, g.aligned_w, 32)[:] = np.pad(pic, ((32, g.aligned_h - h + 32), (32, g.aligned_w - w + 32)), "edge")
    dst = np.zeros(g.frame_size, np.uint8)
    oracle_decode(hdr, mbs, np.zeros((len(mbs), 400), np.int16), mvs, dst, [ref, ref, ref], stages=1)
    cur, anc = S.scale_frame(dst, g, w, h, w, h, 0), S.scale_frame(ref, g, w, h, w, h, 0)
    assert (cur[w * h:] == 128).all() and (anc[w * h:] == 128).all() and np.array_equal(anc[:w * h].reshape(h, w), pic)
    t = T.trace(hdr, mbs, mvs, [T.identity(w, h)] * 3)
    assert (t != T.identity(w, h)).any()
    res = R.residual(cur, anc, t, w, h, matrix="bt601-full")
    assert not res.any(), (size, int((res != 0).sum()))
    # every channel is the luma byte, so this was the pixels' own comparison
    assert np.array_equal(RGB.convert(cur, w, h, matrix="bt601-full")[1], cur[:w * h].reshape(h, w))
    tx, ty = T.unpack(t)
    assert R.residual(cur, anc, T.pack(ty, tx), w, h, matrix="bt601-full").any()
    # the sign: frame minus anchor
    brighter = cur.copy()
    brighter[:w * h] = np.minimum(cur[:w * h].astype(int) + 1, 255)
    up = R.residual(brighter, anc, t, w, h, matrix="bt601-full")
    assert up.min() >= 0 and up.max() == 1


def test_clamp_against_a_loop():
    """traces over all of int16, with -1, d_w (d_h), -32768 and 32767 on both halves: the restatement against a loop written out
    pixel by pixel"""
    w, h = 17, 33
    rng = np.random.default_rng(17)
    cur, anc = random_i420(rng, w, h), random_i420(rng, w, h)
    tx = rng.integers(-32768, 32768, (h, w))
    ty = rng.integers(-32768, 32768, (h, w))
    edge_x, edge_y = [-1, w, -32768, 32767], [-1, h, -32768, 32767]
    k = 0
    for ex in edge_x:                                    # each value on x beside each on y, and beside an inside one
        for ey in edge_y + [5]:
            tx[k // w, k % w], ty[k // w, k % w] = ex, ey
            k += 1
    for ey in edge_y:
        tx[k // w, k % w], ty[k // w, k % w] = 3, ey
        k += 1
    t = T.pack(tx, ty)
    c, a = rgb_planes(cur, w, h, "bt709"), rgb_planes(anc, w, h, "bt709")
    want = np.zeros((3, h, w), np.int64)
    moved = 0
    for y in range(h):
        for x in range(w):
            px, py = int(tx[y, x]), int(ty[y, x])
            ax = 0 if px < 0 else w - 1 if px > w - 1 else px
            ay = 0 if py < 0 else h - 1 if py > h - 1 else py
            moved += (ax, ay) != (px, py)
            for ch in range(3):
                want[ch, y, x] = c[ch, y, x] - a[ch, ay, ax]
    assert moved > h * w // 2
    assert np.array_equal(R.residual(cur, anc, t, w, h, matrix="bt709"), want)
    ax, ay = T.clamped(t, w, h)
    assert ax.min() == 0 and ax.max() == w - 1 and ay.min() == 0 and ay.max() == h - 1


def test_size_function_of_the_library(pkg):
    P = pkg
    L = P.load_hip()

    def lib(w, h, dtype=0, matrix=0, order=0):
        return int(L.vp8hip_trace_residual_size(None, ctypes.byref(P.TraceResidualParams(w, h, matrix, order, dtype))))
    for (w, h), (dt, name) in ((s, d) for s in ((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3)) for d in enumerate(("i16", "f16", "f32"))):
        assert lib(w, h, dt) == R.size(0, 0, w, h, name) == P.trace_residual_size(w, h, np.dtype(R.DTYPES[name]).name) == P.trace_residual_size(w, h, dt), (w, h, name)
        assert lib(w, h, dt, 2, 1) == R.size(0, 0, w, h, name)
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (0, 0)):       # (0 x 0: the display size needs a context)
        assert lib(w, h) == 0, (w, h)
        assert P.trace_residual_size(w, h) == 0
    for bad in (-1, 3):
        assert lib(8, 8, dtype=bad) == 0 and lib(8, 8, matrix=bad) == 0
    for bad in (-1, 2):
        assert lib(8, 8, order=bad) == 0
    assert P.trace_residual_size(8, 8, "int8") == 0
    assert L.vp8hip_trace_residual_size(None, None) == 0
