"""CPU: the definitions of the four histogram calls (vp8hip_frames_hist_async, vp8hip_slots_hist_async,
vp8hip_trace_wear_hist_async, vp8hip_trace_cover_hist_async, include/vp8hip.h) as tests/hist_reference.py restates them -- pinned to
the reference modules whose tensors they count, on the small fixtures; the MVMAG rounding on its ties; the pair histogram's SSE; the
library's size function and what the Python wrappers refuse with no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import hist_reference as H
import invert_reference as I
import scale_reference as SC
import side_reference as S
import trace_reference as R
import wear_reference as W
from trace_testlib import chain, frames_of
from vp8_testlib import random_frame


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (67, 45), (130, 98)])
def test_pictures_against_the_scalers_display_size_image(pkg, size):
    """the planes the picture call counts are those of scale_reference's packed I420 at the display size: luma w x h, chroma
    ((w + 1) / 2) x ((h + 1) / 2)"""
    P = pkg
    w, h = size
    g = P.geom(w, h)
    a, b = random_frame(g, w + h), random_frame(g, w * h)
    pa, pb = (P.split_i420(SC.scale_frame(buf, g, w, h, w, h, 0), w, h) for buf in (a, b))
    assert pa[0].shape == (h, w) and pa[1].shape == ((h + 1) // 2, (w + 1) // 2) == pa[2].shape
    got = H.frames(pa)
    assert got.shape == (3, 256) and got.dtype == np.uint32
    assert got.sum(1).tolist() == [w * h, pa[1].size, pa[2].size]
    for p in range(3):
        assert np.array_equal(got[p], np.bincount(pa[p].ravel(), minlength=256))
    assert np.array_equal(H.frames(pa, planes=("v", "y")), got[[0, 2]]) and np.array_equal(H.frames(pa, planes=2), got[[1]])
    pair = H.frames(pa, pb)
    assert pair.sum(1).tolist() == got.sum(1).tolist()
    for p in range(3):
        d = pa[p].astype(np.int64) - pb[p].astype(np.int64)
        assert H.sse(pair[p]) == int((d * d).sum())                               # the pair histogram's SSE is the direct SSE ...
        assert int((pair[p] * np.arange(256)).sum()) == int(np.abs(d).sum())      # ... and its first moment the SAD
        assert int(pair[p][11:].sum()) == int((np.abs(d) > 10).sum())
    same = H.frames(pa, pa)
    assert (same[:, 0] == got.sum(1)).all() and not same[:, 1:].any()


@pytest.mark.parametrize("name", ["p_odd_130x98", "p_seg_176x144"])
def test_slots_against_the_side_tensor(pkg, name):
    P = pkg
    frames = frames_of(P, name)[:4]
    moved = 0
    for hdr, mbs, mvs, _ in frames:
        cells = 16 * hdr.mb_cols * hdr.mb_rows
        mv, info = S.side(hdr, mbs, mvs, planes=63)
        assert info.shape == (6, 4 * hdr.mb_rows, 4 * hdr.mb_cols) and mv.dtype == np.int16
        got = H.slots(hdr, mbs, mvs, 127)
        assert got.shape == (7, 256) and (got.sum(1) == cells).all()
        for b in range(6):
            assert np.array_equal(got[b], np.bincount(info[b].ravel(), minlength=256)), b
        mag = H.mvmag(mv[0], mv[1])
        assert np.array_equal(got[6], np.bincount(mag.ravel(), minlength=256))
        if hdr.frame_type == 0:
            assert got[6][0] == cells
        moved += int(got[6][1:].sum())
        for planes, which in ((("mvmag", "ref"), [0, 6]), (64, [6]), (("qindex", "coded", "mode"), [1, 4, 5]), (9, [0, 3])):
            assert np.array_equal(H.slots(hdr, mbs, mvs, planes), got[which]), planes
        if name == "p_seg_176x144":
            q = S.qindex_of_segments(hdr)
            assert set(np.nonzero(got[4])[0].tolist()) <= set(q.tolist())
    assert moved > 0


def test_mvmag_rounding_on_the_ties():
    """(v + 4) >> 3 with an arithmetic shift, the trace's rounding: half-way cases go up, also the negative ones"""
    cases = {4: 1, -4: 0, 12: 2, -12: 1, 3: 0, -5: 1, 0: 0, 8: 1, -8: 1, 2036: 255, 2035: 254, -2044: 255, -2036: 254, -32768: 255, 32767: 255}
    for v, want in cases.items():
        assert (abs((v + 4) >> 3) if abs((v + 4) >> 3) < 255 else 255) == want         # (Python's >> is arithmetic)
        for vx, vy in ((v, 0), (0, v), (v, v), (v, 3)):
            assert int(H.mvmag(np.int16(vx), np.int16(vy))) == want, (vx, vy)
    assert int(H.mvmag(np.int16(-12), np.int16(12))) == 2 and int(H.mvmag(np.int16(-32768), np.int16(32767))) == 255
    v = np.arange(-32768, 32768).astype(np.int16)
    assert np.array_equal(H.mvmag(v, np.zeros_like(v)), np.minimum(np.abs(np.floor((v.astype(np.float64) + 4) / 8)), 255).astype(np.uint8))


@pytest.mark.parametrize("name", ["p_arf_176x144", "p_odd_130x98"])
def test_pool_entries_against_the_wear_and_cover_tensors(pkg, name):
    P = pkg
    frames = frames_of(P, name)[:5]
    w, h = int(frames[0][0].width), int(frames[0][0].height)
    pool = {}
    for hdr, mbs, mvs, (new, lst, gld, alt) in frames:
        pool[new] = W.wear(hdr, mbs, mvs, [pool.get(lst), pool.get(gld), pool.get(alt)])
        entry = pool[new]
        got = H.wear(entry)
        assert got.shape == (4, 256) and (got.sum(1) == w * h).all()
        for c, plane in enumerate(W.unpack(entry)):
            assert np.array_equal(got[c], np.bincount(plane.ravel(), minlength=256))
        assert np.array_equal(H.wear(entry, ("coded", "intra")), got[[1, 3]]) and np.array_equal(H.wear(entry, 4), got[[2]])
    assert got[0][0] != w * h                                            # (the last one is an inter frame: hops counted)
    for t in chain(frames):
        _, count = I.invert(t, w, h)
        got = H.cover(count)
        assert got.shape == (2, 256) and (got.sum(1) == w * h).all()
        assert np.array_equal(got[0], np.bincount(np.minimum(count, 255).ravel(), minlength=256))
        assert not got[1][2:].any() and got[1][1] == int((count > 0).sum())          # SEEN fills bins 0 and 1 only
        assert np.array_equal(H.cover(count, ("seen",)), got[[1]])
    # one anchor pixel named by every frame pixel: COUNT saturates at 255
    _, count = I.invert(np.full((h, w), R.pack(3, 2), np.uint32), w, h)
    got = H.cover(count)
    assert got[0][255] == 1 and got[0][0] == w * h - 1 and got[1][1] == 1


def test_size_function_and_wrapper_refusals_with_no_device(pkg):
    P = pkg
    L = P.load_hip()
    for n in range(1, 8):
        assert L.vp8hip_hist_size(n) == n * 1024 == H.hist_size(n) == P.hist_size(n)
    for n in (0, -1, 33, 1 << 20):
        assert L.vp8hip_hist_size(n) == 0 and P.hist_size(n) == 0
    assert P.hist_size(("y", "u", "v")) == 3072 and P.hist_size(("mvmag",)) == 1024 and P.hist_size(()) == 0 and P.hist_size(None) == 0
    assert ctypes.sizeof(P.HistJob) == 8 and [f[0] for f in P.HistJob._fields_] == ["fb", "ref_fb"]
    assert P.HIST_PLANES == H.FRAME_PLANES and P.SLOT_HIST_PLANES == H.SLOT_PLANES and P.SIDE_PLANES == S.PLANES
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrappers see before the call
    for jobs, planes in (([], ("y",)), ([0], ()), ([0], ("y", "nope")), ([0], 8), ([0], 0), ([(0, 1, 2)], 7), ([(0,)], 7), ([-1], 7),
                         ([(0, -2)], 7)):
        with pytest.raises(ValueError):
            ctx.frames_hist(jobs, planes)
    for slots, planes in (([], ("ref",)), ([0], ()), ([0], 128), ([0], ("mvmag", "y")), ([-1], 64)):
        with pytest.raises(ValueError):
            ctx.slots_hist(slots, planes)
    for call, bad in ((ctx.trace_wear_hist, 16), (ctx.trace_cover_hist, 4)):
        for idx, planes in (([], 1), ([0], ()), ([0], bad), ([0], ("nope",)), ([-1], 1)):
            with pytest.raises(ValueError):
                call(None, idx, planes)


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vp8hip.h")
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_hist_size", "vp8hip_frames_hist_async", "vp8hip_slots_hist_async", "vp8hip_trace_wear_hist_async",
                 "vp8hip_trace_cover_hist_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for name, v in (("Y", 1), ("U", 2), ("V", 4), ("MVMAG", 64)):
        assert re.search(r"#define\s+VP8HIP_HIST_%s\s+%d\b" % (name, v), src)
    assert re.search(r"typedef struct vp8hip_hist_job\s*{\s*int32_t fb;\s*int32_t ref_fb;\s*}", src)
