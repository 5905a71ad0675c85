"""CPU: the definition of the block motion search (vp8hip_frames_motion_async, include/vp8hip.h) as tests/motion_reference.py restates
it -- pinned bit for bit to what the reference's vp8_full_search_sad_c, vp8_sad16x16_c and vp8_variance16x16_c returned for the
picture pairs of tests/golden/motion_ref.json --, its known answers, the library's host helpers and what the Python wrapper refuses
with no device."""
import ctypes
import json
import os
import re
import time

import numpy as np
import pytest

import motion_reference as MR

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "motion_ref.json")) as _f:
    CASES = json.load(_f)["cases"]
REF_LIB = os.path.join(HERE, "..", "oracle", "_ref", "libvpxref.so")


def case_id(c):
    return f"{c['kind']}_{c['w']}x{c['h']}_d{c['d']}_{c['centre']}_{c['sad_per_bit']}"


def case_inputs(c):
    """-> (s, ref, centre or None, cost or None) of a fixture case"""
    s, r = MR.pair(c["kind"], c["w"], c["h"], c["seed"])
    centre = MR.fixture_centre(c["centre"], c["h"] // 16, c["w"] // 16, c["seed"] + 1)
    return s, r, centre, MR.fixture_cost(c["d"], c["seed"] + 2) if c["sad_per_bit"] else None


def test_the_fixture_covers_what_it_should():
    assert len(CASES) >= 80
    assert {c["kind"] for c in CASES} == set(MR.KINDS)
    assert {c["d"] for c in CASES} == {1, 4, 16, 64}
    assert {(32, 32), (48, 32), (176, 144)} <= {(c["w"], c["h"]) for c in CASES}
    assert {c["centre"] for c in CASES} == {"zero", "near", "far"}
    assert {0, 255} <= {c["sad_per_bit"] for c in CASES}
    # the reference's int product stays in range everywhere but on the pair made to leave it
    for c in CASES:
        s, r, _, _ = case_inputs(c)
        worst = 255 * 256 if c["kind"] == "extremes" else 46340
        assert all(abs(m[4] - m[5]) <= ((worst * worst) >> 8) for m in c["mbs"])
    # some case's best vector lies on every side of the centre, and some cost table changed the answer
    vec = np.array([m[:2] for c in CASES for m in c["mbs"]])
    assert (vec[:, 0] < 0).any() and (vec[:, 0] > 0).any() and (vec[:, 1] < 0).any() and (vec[:, 1] > 0).any()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_against_the_reference(case):
    """vector, SAD (the cost term taken off: the reference's plain vp8_sad16x16_c at its own vector), SAD0, SSE, VAR and SRCVAR of every
    macroblock; VAR not on the pair whose sum overflows the reference's int"""
    s, r, centre, cost = case_inputs(case)
    d, spb = case["d"], case["sad_per_bit"]
    mv, stats = MR.search(s, r, d, centre, cost, spb)
    rows, cols = case["h"] // 16, case["w"] // 16
    want = np.array(case["mbs"], np.int64).reshape(rows, cols, 7)
    assert np.array_equal(mv[0], want[:, :, 0] << 3) and np.array_equal(mv[1], want[:, :, 1] << 3)
    for my in range(rows):
        for mx in range(cols):
            cx, cy = MR.clamp_centre(s.shape, my, mx, *((0, 0) if centre is None else centre[:, my, mx]))
            term = int(MR.cost_term(cost, spb, want[my, mx, 1] - cy + d, want[my, mx, 0] - cx + d))
            assert int(stats[0, my, mx]) - term == want[my, mx, 2], (my, mx)
    assert np.array_equal(stats[1], want[:, :, 3]) and np.array_equal(stats[2], want[:, :, 4]) and np.array_equal(stats[4], want[:, :, 6])
    if case["kind"] != "extremes":
        assert np.array_equal(stats[3], want[:, :, 5])
    else:
        assert (stats[3] == 0).all() and (stats[2] == 255 * 255 * 256).all()


def test_both_forms_of_the_restatement_agree():
    """the array form against the loop written out candidate by candidate, with centres beyond the bounds and a cost table"""
    for k, (kind, d, centre, spb) in enumerate((("noise", 1, "far", 0), ("stripes", 4, "near", 0), ("smooth", 4, "far", 40), ("flat", 4, "zero", 7),
                                                ("smooth", 6, "near", 255), ("shifted", 5, "zero", 0))):
        s, r = MR.pair(kind, 48, 32, 900 + k)
        c = MR.fixture_centre(centre, 2, 3, 77 + k)
        cost = MR.fixture_cost(d, k) if spb else None
        a = MR.search(s, r, d, c, cost, spb)
        b = MR.search(s, r, d, c, cost, spb, mb=MR.search_mb_loop)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (kind, d)


def test_d64_on_six_macroblocks_is_quick():
    s, r = MR.pair("noise", 48, 32, 5)
    t = time.perf_counter()
    MR.search(s, r, 64)
    assert time.perf_counter() - t < 5.0            # (well under a second on an idle machine; the bound is loose on purpose)


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="the reference build is not present")
def test_sad_and_variance_against_the_reference_library():
    """vp8_sad16x16_c / vp8_variance16x16_c through ctypes on random blocks whose sum stays inside the reference's int product"""
    L = ctypes.CDLL(REF_LIB)
    vp = ctypes.c_void_p
    L.vp8_sad16x16_c.restype = ctypes.c_uint
    L.vp8_sad16x16_c.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int]
    L.vp8_variance16x16_c.restype = ctypes.c_uint
    L.vp8_variance16x16_c.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint)]
    done = 0
    for k in range(40):
        a = np.ascontiguousarray(MR.mixed_bytes(k, 256).reshape(16, 16))
        b = MR.mixed_bytes(100 + k, 256).reshape(16, 16)
        if k % 4 == 1:
            b = (b >> 2).astype(np.uint8)                # a dark block: a large sum
        if k % 4 == 2:
            a, b = np.ascontiguousarray(a >> 1), (128 + (b >> 1)).astype(np.uint8)
        b = np.ascontiguousarray(b)
        total = int(a.astype(np.int64).sum() - b.astype(np.int64).sum())
        if abs(total) > 46340:
            continue
        sse = ctypes.c_uint()
        var = L.vp8_variance16x16_c(a.ctypes.data, 16, b.ctypes.data, 16, ctypes.byref(sse))
        assert (sse.value, var) == MR.variance(a, b), k
        assert L.vp8_sad16x16_c(a.ctypes.data, 16, b.ctypes.data, 16, 0x7fffffff) == int(np.abs(a.astype(np.int64) - b).sum())
        done += 1
    assert done >= 25


def test_known_answers():
    w, h = 64, 48
    ref = MR.mixed_bytes(11, w * h).reshape(h, w)
    # noise shifted by (dy, dx) inside the range: exactly that vector and SAD 0 (every macroblock: the shift is made of E itself)
    for d, (dy, dx) in ((4, (3, -2)), (4, (-4, -4)), (4, (3, 3)), (16, (-16, 15)), (1, (-1, 0))):
        mv, st = MR.search(MR.shifted(ref, dy, dx), ref, d)
        assert (mv[0] == dx << 3).all() and (mv[1] == dy << 3).all() and (st[0] == 0).all() and (st[2] == 0).all() and (st[3] == 0).all(), (d, dy, dx)
        assert (st[1] > 0).all() and st[4][1, 1] > 0         # (a corner block far enough out is one replicated sample: activity 0)
    # a shift on the exclusive side of [-d, d) is not found; the same shift one pixel inside is
    for dy, dx in ((4, 0), (0, 4)):
        mv, st = MR.search(MR.shifted(ref, dy, dx), ref, 4)
        assert (st[0] > 0).all() and not ((mv[0] == dx << 3) & (mv[1] == dy << 3)).any()
        mv, st = MR.search(MR.shifted(ref, dy, dx), ref, 5)
        assert (st[0] == 0).all()
    # a flat pair: every candidate ties, the centre is first -- also a centre tensor's, clamped
    flat_s, flat_r = MR.pair("flat", w, h, 0)
    mv, st = MR.search(flat_s, flat_r, 8)
    assert not mv.any() and (st[0] == 7 * 256).all() and (st[1] == 7 * 256).all() and (st[2] == 49 * 256).all() and (st[3] == 0).all()
    assert (st[4] == 256 * 38 * 38 - ((256 * 38) ** 2 >> 8)).all()
    centre = np.zeros((2, 3, 4), np.int64)
    centre[0], centre[1] = 1000, -5
    mv, _ = MR.search(flat_s, flat_r, 8, centre)
    assert (mv[0] >> 3).tolist() == [[64, 48, 32, 16]] * 3 and (mv[1] >> 3).tolist() == [[-5] * 4, [-5] * 4, [-5] * 4]
    # vertical stripes of period 4 against themselves: (0, 0), the centre, ties with every column shift of 4 -- and wins, coming first;
    # moved off the ties' grid the first candidate in raster order among the ties wins: the top row, the leftmost tying column
    st_s, st_r = MR.pair("stripes", w, h, 0)
    mv, st = MR.search(st_s, st_r, 8)
    assert not mv.any() and not st[0].any()
    mv, st = MR.search(MR.shifted(st_r, 0, 1), st_r, 8)
    inner = (slice(None), slice(1, 2), slice(1, 3))
    assert (mv[0][inner[1:]] >> 3 == -7).all() and (mv[1][inner[1:]] >> 3 == -8).all() and not st[0][inner[1:]].any()
    # a cost table makes a farther exact match lose to a nearer inexact one
    near = ref.copy()
    s = MR.shifted(ref, 0, 6)
    near_s = s.copy()
    mv, st = MR.search(near_s, near, 8)
    assert (mv[0] == 6 << 3).all() and not st[0].any()
    cost = np.zeros((2, 17), np.int32)
    cost[1] = np.abs(np.arange(17) - 8) * 5000
    cost[0] = np.abs(np.arange(17) - 8) * 5000
    mv2, st2 = MR.search(near_s, near, 8, None, cost, 255)
    assert (np.abs(mv2[0] >> 3) < 6).all() and (st2[0] > 0).all() and (st2[0] < 6 * 5000 * 255 >> 8).all()
    # 0 against 255: |sum| = 65280, the variance in 64 bits is 0
    ex_s, ex_r = MR.pair("extremes", 32, 32, 0)
    mv, st = MR.search(ex_s, ex_r, 4)
    assert not mv.any() and (st[0] == 65280).all() and (st[2] == 255 * 255 * 256).all() and (st[3] == 0).all()


def test_planes_and_order():
    stats = np.arange(5 * 6, dtype=np.uint32).reshape(5, 2, 3)
    assert np.array_equal(MR.pick(stats, ("var", "sad")), stats[[0, 3]]) and np.array_equal(MR.pick(stats, 31), stats)
    assert np.array_equal(MR.pick(stats, ("srcvar",)), stats[[4]]) and MR.mask_of(("sad0", "sse")) == 6
    assert MR.bounds((48, 64), 0, 0) == (-16, 48, -16, 64) and MR.bounds((48, 64), 2, 3) == (-48, 16, -64, 16)


def test_module_functions(pkg):
    """motion_sizes, MotionParams and what frames_motion refuses before it needs a device"""
    P = pkg
    assert [f[0] for f in P.MotionParams._fields_] == ["distance", "sad_per_bit", "planes", "cost"] and ctypes.sizeof(P.MotionParams) == 24
    assert P.MOTION_PLANES == {"sad": 1, "sad0": 2, "sse": 4, "var": 8, "srcvar": 16}
    assert P.motion_sizes(11, 9) == (4 * 99, 4 * 99) and P.motion_sizes(11, 9, 31) == (396, 5 * 396) and P.motion_sizes(11, 9, ("var", "sad")) == (396, 792)
    assert P.motion_sizes(11, 9, ()) == (396, 0) and P.motion_sizes(11, 9, 32) == (396, 0) and P.motion_sizes(0, 9) == (0, 0)
    L = P.load_hip()
    assert L.vp8hip_motion_mv_size(None) == 0
    assert L.vp8hip_motion_stats_size(None, ctypes.byref(P.MotionParams(16, 0, 1, None))) == 0
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrapper sees before the call
    ok = np.zeros((2, 33), np.int32)
    for kw in (dict(jobs=[]), dict(jobs=[0]), dict(jobs=[(0, 1, 2)]), dict(jobs=[(0, -1)]), dict(jobs=[(-1, 0)]), dict(distance=0), dict(distance=65),
               dict(sad_per_bit=-1), dict(sad_per_bit=256), dict(planes=("sad", "nope")), dict(planes=32), dict(planes=(), out_stats=object()),
               dict(cost=np.zeros((2, 32), np.int32), sad_per_bit=1), dict(cost=ok - 1, sad_per_bit=1), dict(cost=ok + 65536, sad_per_bit=1)):
        with pytest.raises(ValueError):
            ctx.frames_motion(**dict(dict(jobs=[(0, 0)]), **kw))


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    with open(os.path.join(HERE, "..", "include", "vp8hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_motion_mv_size", "vp8hip_motion_stats_size", "vp8hip_frames_motion_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for k, name in enumerate(("SAD", "SAD0", "SSE", "VAR", "SRCVAR")):
        assert re.search(r"#define\s+VP8HIP_MOTION_" + name + r"\s+" + str(1 << k) + r"\b", src), name
    assert re.search(r"typedef struct vp8hip_motion\s*{\s*int distance;\s*int sad_per_bit;\s*unsigned planes;\s*const int32_t \*cost;\s*}", src)
