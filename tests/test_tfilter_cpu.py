"""CPU: the definition of the temporal filter (vp8hip_frames_tfilter_async, include/vp8hip.h) as tests/tfilter_reference.py restates it
-- pinned bit for bit to what the reference's vp8_temporal_filter_apply_c accumulated over the reference's own predictions for the
cases of tests/golden/tfilter_ref.json --, its known answers, the library's host helpers and what the Python wrapper refuses with no
device."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import tfilter_reference as TR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_tfilter_fixtures import case_inputs, unpacked  # noqa: E402

with open(os.path.join(HERE, "golden", "tfilter_ref.json")) as _f:
    CASES = json.load(_f)["cases"]


def case_id(c):
    return f"{c['w']}x{c['h']}_n{c['count']}_{c['filter']}_s{c['strength']}_{c['vectors']}_{c['weights']}"


def test_the_fixture_covers_what_it_should():
    assert {(c["w"], c["h"]) for c in CASES} == {(32, 32), (48, 32), (176, 144)}
    assert {c["count"] for c in CASES} == {1, 2, 3, 15}
    assert {c["filter"] for c in CASES} == set(TR.FILTERS) and {c["strength"] for c in CASES} == {1, 3, 6}
    assert {c["vectors"] for c in CASES} == set(TR.VECTORS) and {c["weights"] for c in CASES} == set(TR.WEIGHTS) | {"val"}
    for size in ((32, 32), (48, 32), (176, 144)):                       # every size with both filters and with every kind of vector
        mine = [c for c in CASES if (c["w"], c["h"]) == size]
        assert {c["filter"] for c in mine} == set(TR.FILTERS) and {c["vectors"] for c in mine} == set(TR.VECTORS)
        assert all(("picture" in c) == (size != (176, 144)) for c in mine)
    lx, ly, cx, cy, neg_odd, weights, outside = set(), set(), set(), set(), False, set(), False
    for c in CASES:
        _, _, mvs, errs = case_inputs(c)
        rows, cols = c["h"] // 16, c["w"] // 16
        for k in range(c["count"]):
            e = None if errs is None else np.asarray(errs[k]).astype(np.int64)
            assert e is None or int(e.max()) < 1 << 31
            weights |= {2} if e is None else {TR.weight(v) for v in e.ravel()}
            if e is not None and c["weights"] == "mixed":
                assert {TR.THRESH[0] - 1, TR.THRESH[0], TR.THRESH[1] - 1, TR.THRESH[1]} <= set(e.ravel().tolist()) or rows * cols < 8
            if mvs is None:
                continue
            x, y = mvs[k][0].ravel(), mvs[k][1].ravel()
            # phases by direction: (phase, sign of the vector)
            lx |= set(zip((x & 7).tolist(), np.sign(x).tolist()))
            ly |= set(zip((y & 7).tolist(), np.sign(y).tolist()))
            cx |= set(zip(((x >> 1) & 7).tolist(), np.sign(x).tolist()))
            cy |= set(zip(((y >> 1) & 7).tolist(), np.sign(y).tolist()))
            neg_odd |= bool(((x < 0) & ((x & 1) == 1)).any() and ((y < 0) & ((y & 1) == 1)).any())
            if c["vectors"] == "outside":
                my, mx = np.mgrid[0:rows, 0:cols]
                bx, by = 16 * mx + (mvs[k][0] >> 3), 16 * my + (mvs[k][1] >> 3)
                assert (((bx + 18 < 0) | (bx - 2 >= c["w"])) | ((by + 18 < 0) | (by - 2 >= c["h"]))).all()
                outside = True
    for seen in (lx, ly, cx, cy):                                       # all eight phases, towards either side
        assert {(p, s) for p in range(1, 8) for s in (-1, 1)} <= seen and any(p == 0 for p, _ in seen)
    assert neg_odd and outside and weights == {0, 1, 2}
    assert any(c["weights"] == "none" for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_against_the_reference(case):
    """the picture and the count of every pixel"""
    centre, sources, mvs, errs = case_inputs(case)
    pic, cnt = TR.tfilter(centre, sources, mvs, errs, case["strength"], case["filter"])
    cnt = cnt.astype("<u2")
    if "picture" in case:
        assert np.array_equal(pic, unpacked(case["picture"], np.uint8)) and np.array_equal(cnt, unpacked(case["counts"], "<u2"))
    else:
        assert hashlib.sha256(pic.tobytes()).hexdigest() == case["picture_sha256"]
        assert hashlib.sha256(cnt.tobytes()).hexdigest() == case["counts_sha256"]
    if case["weights"] == "none":
        assert not pic.any() and not cnt.any()


def test_known_answers():
    w, h = 48, 32
    noise, smooth = TR.picture("noise", w, h, 4), TR.picture("smooth", w, h, 5)
    # a picture filtered over itself any number of times is itself, with count = 32 * count -- 480 with fifteen
    for pic in (noise, smooth):
        for n, strength, filt in ((1, 0, "sixtap"), (2, 3, "bilinear"), (7, 6, "sixtap"), (15, 3, "sixtap")):
            out, cnt = TR.tfilter(pic, [pic] * n, strength=strength, filt=filt)
            assert np.array_equal(out, TR.pack(pic, w, h)) and (cnt == 32 * n).all(), (n, strength)
    assert int(TR.tfilter(noise, [noise] * 15)[1].max()) == 480
    # all weights 0: picture 0, count 0
    zero = [np.full((2, 3), 20000, np.uint32)] * 2
    out, cnt = TR.tfilter(noise, [noise, smooth], errs=zero)
    assert not out.any() and not cnt.any()
    # a source further away than the strength allows (m reaches 16) leaves the centre unchanged where the centre is listed
    f90, f97, f200 = (TR.picture(k, w, h, 0) for k in ("flat90", "flat97", "flat200"))
    for strength in (0, 3, 6):
        out, cnt = TR.tfilter(f90, [f90, f200], strength=strength)
        assert (out == 90).all() and (cnt == 32).all()
    # flat 90 against flat 97: d = 7, 3 d^2 = 147; strength 4: (147 + 8) >> 4 = 9, m = 7, W = 2: 14; 5: (147 + 16) >> 5 = 5, m = 11: 22;
    # 6: (147 + 32) >> 6 = 2, m = 14: 28.  With the centre: (32 * 90 + 14 * 97) / 46 = 92.13 -> 92; 5014 / 54 = 92.85 -> 93; 5596 / 60 = 93.27 -> 93
    for strength, m, byte in ((4, 14, 92), (5, 22, 93), (6, 28, 93)):
        out, cnt = TR.tfilter(f90, [f97], strength=strength)
        assert (out == 97).all() and (cnt == m).all(), strength
        out, cnt = TR.tfilter(f90, [f90, f97], strength=strength)
        assert (out == byte).all() and (cnt == 32 + m).all(), strength
        out, cnt = TR.tfilter(f90, [f97], errs=[np.full((2, 3), 10000, np.uint32)], strength=strength)    # W = 1: half the count
        assert (out == 97).all() and (cnt == m // 2).all(), strength
    out, cnt = TR.tfilter(f90, [f97], strength=3)                           # (147 + 4) >> 3 = 18: m reaches 16
    assert not out.any() and not cnt.any()
    # strength 0: m = 3 d^2 -- d = 2: 12, 16 - 12 = 4, W = 2: 8; d = 1: 3 -> 26
    f92, f91 = TR.picture("flat92", w, h, 0), TR.picture("flat91", w, h, 0)
    assert (TR.tfilter(f90, [f92], strength=0)[1] == 8).all() and (TR.tfilter(f90, [f91], strength=0)[1] == 26).all()
    assert (TR.tfilter(f90, [f92], strength=1)[1] == 2 * (16 - ((12 + 1) >> 1))).all()
    # the weight: unsigned, both thresholds exclusive below
    assert [TR.weight(e) for e in (0, 9999, 10000, 19999, 20000, (1 << 32) - 1, -1)] == [2, 2, 1, 1, 0, 0, 0]
    # the normalisation is the reference's table, not a division: 255 * 7 = 1785, + 3, * (0x80000 / 7 = 74898) >> 19 = 255
    assert int(TR.normalise(np.array([1785]), np.array([7]))[0]) == (1788 * 74898) >> 19 == 255
    assert int(TR.normalise(np.array([0]), np.array([0]))[0]) == 0
    # the chroma vector is the luma vector >> 1, arithmetic: -1 -> -1 (base -1, offset 7), not 0
    ramp = [np.tile(np.arange(w, dtype=np.uint8) * 4, (h, 1)), np.tile(np.arange(w // 2, dtype=np.uint8) * 8, (h // 2, 1)),
            np.tile(np.arange(w // 2, dtype=np.uint8) * 8, (h // 2, 1))]
    q = TR.predict(ramp[1], 8, 8, 0, -1 >> 1, 8, "bilinear")
    assert (q == ramp[1][8:16, 8:16].astype(np.int64) - 1).all()            # 1/8 of a chroma pixel left on a ramp of 8 a pixel
    # the crop from the coded to an odd display size keeps the right pixels: 37x21, chroma 19x11
    pic, cnt = TR.tfilter_planes(smooth, [smooth, noise], strength=6)
    out, oc = TR.tfilter(smooth, [smooth, noise], strength=6, display=(37, 21))
    assert out.size == 37 * 21 + 2 * 19 * 11 == oc.size
    assert np.array_equal(out[:37 * 21].reshape(21, 37), pic[0][:21, :37]) and np.array_equal(out[37 * 21:37 * 21 + 209].reshape(11, 19), pic[1][:11, :19])
    assert np.array_equal(out[37 * 21 + 209:].reshape(11, 19), pic[2][:11, :19]) and np.array_equal(oc[37 * 21 + 209:].reshape(11, 19), cnt[2][:11, :19])


def test_sizes_structs_and_what_the_wrapper_refuses(pkg):
    P = pkg
    assert P.tfilter_sizes(176, 144) == (38016, 76032) and P.tfilter_sizes(37, 21) == (37 * 21 + 2 * 19 * 11, 2 * (37 * 21 + 2 * 19 * 11))
    assert P.tfilter_sizes(0, 16) == (0, 0) and P.tfilter_sizes(16, 16384) == (0, 0)
    assert [f[0] for f in P.TfilterParams._fields_] == ["strength", "filter", "thresh_low", "thresh_high"] and ctypes.sizeof(P.TfilterParams) == 16
    assert [f[0] for f in P.TfilterJob._fields_] == ["fb", "first", "count"] and ctypes.sizeof(P.TfilterJob) == 12
    assert P.TFILTER_FILTERS == {"sixtap": 0, "bilinear": 1} and P.TFILTER_MAX_COUNT == 15
    L = P.load_hip()
    assert L.vp8hip_tfilter_count_size(None) == 0
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrapper sees before the call
    pairs = [(0, 1), (0, 2), (1, 0)]
    for kw in (dict(jobs=[]), dict(pairs=[]), dict(jobs=[0]), dict(jobs=[(0, 0)]), dict(jobs=[(0, 0, 1, 1)]), dict(pairs=[(0, 1, 2)]), dict(pairs=[(0, -1)]),
               dict(pairs=[(-1, 0)]), dict(jobs=[(-1, 0, 1)]), dict(jobs=[(0, 0, 0)]), dict(jobs=[(0, 0, 16)]), dict(jobs=[(0, -1, 1)]),
               dict(jobs=[(0, 0, 4)]), dict(jobs=[(0, 3, 1)]), dict(jobs=[(0, 1, 2)]), dict(jobs=[(1, 0, 1)]), dict(jobs=[(0, 0, 2), (0, 2, 1)]),
               dict(strength=-1), dict(strength=7), dict(filter="bicubic"), dict(filter=2), dict(thresh=(2, 1)), dict(thresh=(-1, 1)),
               dict(thresh=(0, 1 << 32))):
        with pytest.raises(ValueError):
            ctx.frames_tfilter(**dict(dict(jobs=[(0, 0, 2)], pairs=pairs), **kw))


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    with open(os.path.join(HERE, "..", "include", "vp8hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_tfilter_count_size", "vp8hip_frames_tfilter_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert re.search(r"#define\s+VP8HIP_TFILTER_SIXTAP\s+0\b", src) and re.search(r"#define\s+VP8HIP_TFILTER_BILINEAR\s+1\b", src)
    assert re.search(r"typedef struct vp8hip_tfilter\s*{\s*int strength;\s*int filter;\s*unsigned thresh_low;\s*unsigned thresh_high;\s*}", src)
    assert re.search(r"typedef struct vp8hip_tfilter_job\s*{\s*int32_t fb, first, count;\s*}", src)
