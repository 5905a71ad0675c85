"""CPU: the definition of the accumulated-motion trace and of its flow tensor (vp8hip_frames_trace_async, vp8hip_trace_flow_async,
include/vp8hip.h) as tests/trace_reference.py restates it -- the conventions pinned by the oracle decoder on a hand-built frame, one
hop against the side tensors, the chain over the fixtures against a last-frame-only chain, the special cases, the flow tensor and
the library's size functions."""
import ctypes

import numpy as np
import pytest

from vp8_testlib import oracle_decode
import side_reference as S
import trace_reference as R
from trace_testlib import NEWMV, chain, frames_of, luma, make_hdr, whole_pixel_frame



@pytest.mark.parametrize("size", [(16, 16), (67, 45), (176, 144)])
def test_oracle_pins_axis_order_sign_and_clamp(pkg, size):
    """the oracle decoder predicts such a frame from three random pictures (what lies past the display size replicating its edge,
    as the border extension does past the coded area): every display pixel is ref[r][sy, sx] as the restatement computes (r, sy, sx)"""
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    g = P.geom(w, h)
    hdr, mbs, mvs = whole_pixel_frame(P, w, h, rng)
    pics, bufs = [], []
    for _ in range(3):
        pic = rng.integers(0, 256, (h, w)).astype(np.uint8)
        buf = np.zeros(g.frame_size, np.uint8)
        luma(buf, g, g.aligned_h, g.aligned_w, 32)[:] = np.pad(pic, ((32, g.aligned_h - h + 32), (32, g.aligned_w - w + 32)), "edge")
        pics.append(pic)
        bufs.append(buf)
    dst = np.zeros(g.frame_size, np.uint8)
    oracle_decode(hdr, mbs, np.zeros((len(mbs), 400), np.int16), mvs, dst, bufs, stages=1)
    r, sy, sx = R.hop(hdr, mbs, mvs)
    assert set(np.unique(r).tolist()) <= {1, 2, 3}
    want = np.zeros((h, w), np.uint8)
    for q in (1, 2, 3):
        want[r == q] = pics[q - 1][sy[r == q], sx[r == q]]
    got = luma(dst, g, h, w)
    assert np.array_equal(got, want), (size, int((got != want).sum()))
    # the frame does what the test is about: vectors both ways on both axes, and sources that the clamp moved
    ys, xs = np.mgrid[0:h, 0:w]
    v = mvs[(ys >> 4) * hdr.mb_cols + (xs >> 4), ((ys >> 2) & 3) * 4 + ((xs >> 2) & 3)].astype(int) >> 3
    assert (v[..., 0] < 0).any() and (v[..., 0] > 0).any() and (v[..., 1] < 0).any() and (v[..., 1] > 0).any()
    assert ((xs + v[..., 1] != sx) | (ys + v[..., 0] != sy)).any()
    # ... and a trace through three identity references says the same
    ident = R.identity(w, h)
    tx, ty = R.unpack(R.trace(hdr, mbs, mvs, [ident] * 3))
    assert np.array_equal(tx, sx) and np.array_equal(ty, sy)


def test_one_hop_agrees_with_the_side_tensors(pkg):
    P = pkg
    frames = frames_of(P, "p_odd_130x98")
    hdr0, hdr, mbs, mvs = frames[0][0], *frames[1][:3]
    assert hdr0.frame_type == 0 and hdr.frame_type == 1
    w, h = hdr.width, hdr.height
    ident = R.identity(w, h)
    t = R.trace(hdr, mbs, mvs, [ident, ident, ident])
    mv, _ = S.side(hdr, mbs, mvs, w, h)          # [2, h, w]: x, y in 1/8 pel
    step = (mv.astype(int) + 4) >> 3
    ys, xs = np.mgrid[0:h, 0:w]
    inside = (xs + step[0] >= 0) & (xs + step[0] < w) & (ys + step[1] >= 0) & (ys + step[1] < h)
    tx, ty = R.unpack(t)
    assert inside.sum() > h * w // 2 and step.any()
    assert np.array_equal((tx - xs)[inside], step[0][inside]) and np.array_equal((ty - ys)[inside], step[1][inside])
    # the flow tensor at the display size is that difference
    fl = R.flow(t)
    assert fl.dtype == np.int16 and np.array_equal(fl[0], tx - xs) and np.array_equal(fl[1], ty - ys)


@pytest.mark.parametrize("name", ["p_arf_176x144", "p_prof1_640x360"])
def test_the_chain_discriminates(pkg, name):
    """following the reference each macroblock names differs from following the frame before on more than half of all pixel-frames;
    every value stays inside the picture"""
    P = pkg
    frames = frames_of(P, name)
    full, last = chain(frames), chain(frames, last_only=True)
    differ = sum(int((a != b).sum()) for a, b in zip(full, last))
    total = sum(a.size for a in full)
    assert 2 * differ > total, (name, differ, total)
    assert (differ, total) == {"p_arf_176x144": (2032400, 2407680), "p_prof1_640x360": (1459630, 2304000)}[name]
    w, h = frames[0][0].width, frames[0][0].height
    for t in full:
        tx, ty = R.unpack(t)
        assert tx.min() >= 0 and tx.max() < w and ty.min() >= 0 and ty.max() < h
    if name == "p_arf_176x144":
        assert sum(1 for f in frames if not f[0].show_frame) == 5 and len(frames) == 95


def test_key_frames_intra_macroblocks_and_missing_references(pkg):
    P = pkg
    w, h = 67, 45
    rng = np.random.default_rng(3)
    hdr, mbs, mvs = whole_pixel_frame(P, w, h, rng)
    mvs += rng.integers(-7, 8, mvs.shape).astype(np.int16)          # sub-pixel parts
    ident = R.identity(w, h)
    junk = [rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32) for _ in range(3)]
    # a key frame is the identity whatever the references and the vector area hold
    key = make_hdr(P, w, h, frame_type=0)
    assert np.array_equal(R.trace(key, mbs, mvs, junk), ident)
    assert np.array_equal(R.trace(key, mbs, mvs, [None] * 3), ident)
    # a reference of -1: the identity where a macroblock names it, the gathered dword elsewhere
    r, sy, sx = R.hop(hdr, mbs, mvs)
    for q in (1, 2, 3):
        refs = list(junk)
        refs[q - 1] = None
        t = R.trace(hdr, mbs, mvs, refs)
        assert np.array_equal(t[r == q], ident[r == q]) and (r == q).any()
        for o in {1, 2, 3} - {q}:
            assert np.array_equal(t[r == o], junk[o - 1][sy[r == o], sx[r == o]])
    assert np.array_equal(R.trace(hdr, mbs, mvs, [None] * 3), ident)
    # intra macroblocks hold: through the last frame, in place, whatever their vectors
    intra = mbs.copy()
    intra[::2, R.O_REF] = 0
    t = R.trace(hdr, intra, mvs, junk)
    held = (np.arange(len(mbs)) % 2 == 0).reshape(hdr.mb_rows, hdr.mb_cols).repeat(16, 0).repeat(16, 1)[:h, :w]
    assert np.array_equal(t[held], junk[0][held])
    assert np.array_equal(t[~held], R.trace(hdr, mbs, mvs, junk)[~held])
    # ties go up: 4/8 -> 1, -4/8 -> 0, 12/8 -> 2, -12/8 -> -1
    one = make_hdr(P, 16, 16)
    m1 = np.zeros((1, 64), np.uint8)
    m1[0, 0], m1[0, R.O_REF] = NEWMV, 1
    for v8, want in ((4, 1), (-4, 0), (12, 2), (-12, -1), (3, 0), (-5, -1)):
        v1 = np.full((1, 16, 2), v8, np.int16)
        tx, ty = R.unpack(R.trace(one, m1, v1, [R.identity(16, 16)] * 3))
        assert tx[8, 8] == 8 + want and ty[8, 8] == 8 + want, v8


def test_flow_restatement():
    rng = np.random.default_rng(9)
    w, h = 130, 98
    t = R.pack(rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w)))
    tx, ty = R.unpack(t)
    ys, xs = np.mgrid[0:h, 0:w]
    at = R.flow(t)
    assert at.shape == (2, h, w) and np.array_equal(at[0], tx - xs) and np.array_equal(at[1], ty - ys)
    f = R.flow(t, 224, 224, "f32", R.pixel_scale(w, h, 224, 224))
    assert f.shape == (2, 224, 224) and f.dtype == np.float32
    sx, sy = R.grid_map(224, w), R.grid_map(224, h)
    assert np.array_equal(f[0], ((tx[sy][:, sx].astype(np.float64) - sx) * np.float64(np.float32(224 / w))).astype(np.float32))
    assert np.array_equal(f[1], ((ty[sy][:, sx].astype(np.float64) - sy[:, None]) * np.float64(np.float32(224 / h))).astype(np.float32))
    one = R.flow(t, 1, 1, "f16", (0.5, 2.0))     # 1x1: the centre pixel
    assert one.shape == (2, 1, 1) and one.dtype == np.float16
    assert one[0, 0, 0] == np.float16((int(tx[h // 2, w // 2]) - w // 2) * 0.5) and one[1, 0, 0] == np.float16((int(ty[h // 2, w // 2]) - h // 2) * 2.0)
    assert (R.flow(R.identity(w, h), 33, 77) == 0).all()
    # what a pool entry may hold is data: a difference beyond int16 keeps its low 16 bits
    wild = R.pack(np.full((h, w), -32768), np.full((h, w), 32767))
    assert R.flow(wild)[0, 0, w - 1] == np.int16((-32768 - (w - 1)) & 0xffff) and R.flow(wild, dtype="f32")[0, 0, w - 1] == -32768.0 - (w - 1)


def test_size_functions_of_the_library(pkg):
    P = pkg
    L = P.load_hip()
    assert L.vp8hip_trace_size(None) == 0        # needs a configured context
    assert P.trace_size(1920, 1080) == 4 * 1920 * 1080

    def lib(w, h, dtype=0):
        return int(L.vp8hip_trace_flow_size(None, ctypes.byref(P.TraceFlowParams(w, h, dtype))))
    for (w, h), (dt, name) in ((s, d) for s in ((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3)) for d in enumerate(("i16", "f16", "f32"))):
        assert lib(w, h, dt) == R.flow_size(0, 0, w, h, name), (w, h, name)
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (0, 0)):       # (0 x 0: the display size needs a context)
        assert lib(w, h) == 0, (w, h)
    for dt in (-1, 3):
        assert lib(8, 8, dt) == 0
    assert L.vp8hip_trace_flow_size(None, None) == 0
