"""CPU: the definition of the sub-pixel refinement (vp8hip_frames_subpel_async, include/vp8hip.h) as tests/subpel_reference.py restates
it -- pinned bit for bit to what the reference's vp8_find_best_sub_pixel_step and vp8_find_best_half_pixel_step returned for the
picture pairs of tests/golden/subpel_ref.json --, its known answers, the library's host helpers and what the Python wrapper refuses
with no device."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import motion_reference as MR
import subpel_reference as SR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_subpel_fixtures import case_inputs  # noqa: E402

with open(os.path.join(HERE, "golden", "subpel_ref.json")) as _f:
    CASES = json.load(_f)["cases"]


def case_id(c):
    return f"{c['kind']}_{c['w']}x{c['h']}_{c['start']}_{c['ref']}_R{c['R']}_e{c['error_per_bit']}_p{c['precision']}"


def test_the_fixture_covers_what_it_should():
    assert len(CASES) >= 100
    assert {c["kind"] for c in CASES} == set(SR.KINDS) - {"extremes"}
    assert {(32, 32), (48, 32), (176, 144)} <= {(c["w"], c["h"]) for c in CASES}
    assert {c["start"] for c in CASES} == {"zero", "search", "near", "far", "bounds"}
    assert {c["ref"] for c in CASES} == {"zero", "given"} and {c["precision"] for c in CASES} == {2, 4}
    assert {0, 1, 16383} <= {c["error_per_bit"] for c in CASES} and {0, 40, 255, 1023} == {c["R"] for c in CASES}
    vec = np.array([m[:2] for c in CASES for m in c["mbs"]])
    assert set(np.unique(vec & 7)) == {0, 2, 4, 6}                      # every quarter-pel phase is some macroblock's answer
    assert (vec[:, 0] < 0).any() and (vec[:, 0] > 0).any() and (vec[:, 1] < 0).any() and (vec[:, 1] > 0).any()
    for c in CASES:                                                     # precision 2 never leaves the half-pel grid
        if c["precision"] == 2:
            assert not (np.array([m[:2] for m in c["mbs"]]) & 3).any()
    # some reference vector is odd, and some cost table changed an answer
    assert any((SR.fixture_ref("given", c["h"] // 16, c["w"] // 16, c["seed"] + 3) & 1).any() for c in CASES if c["ref"] == "given")
    assert any(m[2] != m[3] for c in CASES if c["R"] for m in c["mbs"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_against_the_reference(case):
    """vector, return value, *distortion and *sse1 of every macroblock, and the variance at the start"""
    s, r, start, rvec, cost = case_inputs(case)
    mv, stats = SR.refine(s, r, start, rvec, cost, case["error_per_bit"], case["precision"])
    want = np.array(case["mbs"], np.int64).reshape(case["h"] // 16, case["w"] // 16, 6)
    assert np.array_equal(mv[0], want[:, :, 0]) and np.array_equal(mv[1], want[:, :, 1])
    for k in range(4):
        assert np.array_equal(stats[k], want[:, :, 2 + k]), SR.NAMES[k]


def test_known_answers():
    w, h = 64, 48
    rows, cols = h // 16, w // 16
    noise = MR.mixed_bytes(21, w * h).reshape(h, w)
    # a picture against itself: v0 with value 0, from any start that is the true whole-pixel shift
    mv, st = SR.refine(noise, noise)
    assert not mv.any() and not st.any()
    true = np.zeros((2, rows, cols), np.int64)
    true[0], true[1] = -2 << 3, 3 << 3
    mv, st = SR.refine(MR.shifted(noise, 3, -2), noise, true)
    assert (mv[0] == -16).all() and (mv[1] == 24).all() and not st.any()
    # a smooth picture against its own bilinear shift: exactly that vector, VAR == 0 -- the half-pel one at either precision
    smooth = SR.lowpass(5, w, h)
    for vec in ((4, -4), (-4, 0), (0, 4), (-2, 6), (6, 2), (2, 0), (-6, -6)):
        for precision in ((2, 4) if not (vec[0] | vec[1]) & 3 else (4,)):
            mv, st = SR.refine(SR.subshifted(smooth, *vec), smooth, precision=precision)
            assert (mv[0] == vec[1]).all() and (mv[1] == vec[0]).all() and not st[:3].any() and st[3].all(), (vec, precision)
    # flat pictures keep v0: every comparison is strict -- also a start beyond the bounds, clamped
    flat_s, flat_r = MR.pair("flat", w, h, 0)
    mv, st = SR.refine(flat_s, flat_r)
    assert not mv.any() and (st[0] == 0).all() and (st[2] == 49 * 256).all() and (st[3] == 0).all()
    far = np.zeros((2, rows, cols), np.int64)
    far[0], far[1] = 8000 + 5, -8000
    mv, _ = SR.refine(flat_s, flat_r, far)
    assert mv[0].tolist() == [[8 * 64, 8 * 48, 8 * 32, 8 * 16]] * 3 and mv[1].tolist() == [[-8 * 16] * 4, [-8 * 32] * 4, [-8 * 48] * 4]
    # an arranged left / right tie: columns symmetric about every block's middle axis tie left with right, so the diagonal goes
    # right -- case 3 (down-right) where up and down tie too or down is smaller, case 1 (up-right) where up is smaller -- read
    # off the log of the evaluations
    xx, yy = np.arange(w) % 16, np.arange(h)[:, None] % 16
    sym = np.tile((np.minimum(xx, 15 - xx) * 9 + 40).astype(np.uint8), (h, 1))
    seen = set()
    below = np.where(np.arange(h)[:, None] >= 32, 30, 0)              # only the row under macroblock row 1 differs: down is worse
    for rowterm in (yy * 3, yy * yy // 3, below):
        other = (sym.astype(np.int64) + rowterm).astype(np.uint8)
        log = []
        SR.refine_mb(sym, other, 1, 1, log=log, precision=2)
        vals = [SR.dist(sym[16:32, 16:32], SR.predict(other, 16, 16, e[0], e[1]))[0] for e in log[1:5]]
        assert vals[0] == vals[1]
        assert log[5][:2] == ((-4 if vals[2] < vals[3] else 4), 4)
        seen.add(log[5][:2])
    assert seen == {(-4, 4), (4, 4)}
    # 0 against 255: |sum| = 65280, the variance in 64 bits is 0 everywhere and v0 stays
    ex_s, ex_r = MR.pair("extremes", 32, 32, 0)
    mv, st = SR.refine(ex_s, ex_r)
    assert not mv.any() and not st[[0, 1, 3]].any() and (st[2] == 255 * 255 * 256).all()
    # cost indices beyond the table are clamped to its ends
    cost = SR.fixture_cost(2, 1)
    assert SR.cost_term(cost, 256, 2, 100, -100, 0, 0) == int(cost[0][4]) + int(cost[1][0])
    assert SR.cost_term(cost, 256, 2, 3, -3, 1, 0) == int(cost[0][3]) + int(cost[1][0])       # (2 >> 1, -3 >> 1) = (1, -2)
    # a steep table keeps the refinement at the vector the cost is counted from
    steep = np.zeros((2, 81), np.int32)
    steep[:] = np.abs(np.arange(81) - 40) * 800
    mv, st = SR.refine(SR.subshifted(smooth, 4, -4), smooth, cost=steep, epb=16383)
    assert not mv.any() and (st[0] == st[3]).all()


def test_planes_and_sizes(pkg):
    P = pkg
    stats = np.arange(4 * 6, dtype=np.uint32).reshape(4, 2, 3)
    assert np.array_equal(SR.pick(stats, ("sse", "val")), stats[[0, 2]]) and np.array_equal(SR.pick(stats, 15), stats)
    assert SR.mask_of(("var0", "var")) == 10 and SR.PLANES == P.SUBPEL_PLANES
    assert [f[0] for f in P.SubpelParams._fields_] == ["precision", "error_per_bit", "cost_range", "planes", "cost"]
    assert ctypes.sizeof(P.SubpelParams) == 24
    assert P.subpel_sizes(11, 9) == (396, 396) and P.subpel_sizes(11, 9, 15) == (396, 4 * 396) and P.subpel_sizes(11, 9, ("var0", "val")) == (396, 792)
    assert P.subpel_sizes(11, 9, ()) == (396, 0) and P.subpel_sizes(11, 9, 16) == (396, 0) and P.subpel_sizes(0, 9) == (0, 0)
    L = P.load_hip()
    assert L.vp8hip_subpel_mv_size(None) == 0
    assert L.vp8hip_subpel_stats_size(None, ctypes.byref(P.SubpelParams(4, 0, 0, 1, None))) == 0
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrapper sees before the call
    ok = np.zeros((2, 33), np.int32)
    for kw in (dict(jobs=[]), dict(jobs=[0]), dict(jobs=[(0, 1, 2)]), dict(jobs=[(0, -1)]), dict(jobs=[(-1, 0)]), dict(precision=1), dict(precision=3),
               dict(precision=8), dict(error_per_bit=-1), dict(error_per_bit=16384), dict(planes=("val", "nope")), dict(planes=16),
               dict(planes=(), out_stats=object()), dict(cost=np.zeros((2, 32), np.int32), error_per_bit=1), dict(cost=np.zeros((3, 33), np.int32)),
               dict(cost=np.zeros((2, 1), np.int32)), dict(cost=np.zeros((2, 2049), np.int32)), dict(cost=ok - 1, error_per_bit=1),
               dict(cost=ok + 65536, error_per_bit=1)):
        with pytest.raises(ValueError):
            ctx.frames_subpel(**dict(dict(jobs=[(0, 0)]), **kw))


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    with open(os.path.join(HERE, "..", "include", "vp8hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_subpel_mv_size", "vp8hip_subpel_stats_size", "vp8hip_frames_subpel_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for k, name in enumerate(("VAL", "VAR", "SSE", "VAR0")):
        assert re.search(r"#define\s+VP8HIP_SUBPEL_" + name + r"\s+" + str(1 << k) + r"\b", src), name
    assert re.search(r"typedef struct vp8hip_subpel\s*{\s*int precision;\s*int error_per_bit;\s*int cost_range;\s*unsigned planes;\s*const int32_t \*cost;\s*}", src)
