"""CPU: the definition of the structural-similarity call (vp8hip_frames_ssim_async, include/vp8hip.h) as tests/ssim_reference.py
restates it -- pinned to what the reference's vp8_ssim2 returned for the plane pairs of tests/golden/ssim_ref.json (bit for bit
where the restatement sums as the reference sums; within the bound the header gives where it sums in Q32), its properties on the
adversarial pairs, the library's host helpers and what the Python wrappers refuse with no device."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import ssim_reference as SR

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ssim_ref.json")) as _f:
    CASES = json.load(_f)["cases"]


def case_id(c):
    return f"{c['kind']}_{c['w']}x{c['h']}"


def test_the_fixture_covers_what_it_should():
    assert len(CASES) >= 36
    assert {c["kind"] for c in CASES} == set(SR.KINDS)
    assert {(8, 8), (9, 9), (12, 12), (13, 13), (16, 16), (17, 33), (25, 9), (67, 45), (130, 98), (8208, 16)} <= {(c["w"], c["h"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_against_the_references_doubles(case):
    """summed in raster order the restatement's mean IS vp8_ssim2's double; the mean of the Q32 total is within 2^-33 + N * 2^-52 of
    it; 8x8 has no windows and the reference gives 0 / 0"""
    w, h = case["w"], case["h"]
    s, r = SR.pair(case["kind"], w, h, case["seed"])
    assert s.shape == (h, w) and s.dtype == np.uint8 and r.dtype == np.uint8
    got = SR.raster_mean(s, r)
    if case["ssim2"] == "nan":
        assert (w, h) == (8, 8) and math.isnan(got) and SR.plane_scores(s, r) == (0, 0) and math.isnan(SR.q32_mean(s, r))
        return
    want = float.fromhex(case["ssim2"])
    assert got.hex() == want.hex()
    total, count = SR.plane_scores(s, r)
    assert count == np.prod(SR.windows(w, h)) > 0
    assert abs(SR.q32_mean(s, r) - want) <= 2.0 ** -33 + count * 2.0 ** -52
    assert abs(total) <= count << 32
    if case["kind"] == "identical":
        assert want == 1.0 and total == count << 32


@pytest.mark.parametrize("size", [(9, 9), (16, 16), (17, 33), (67, 45), (130, 98)])
def test_bounds_symmetry_and_identity(size):
    """d > 0 and |v| <= 1 on the pairs that push either factor to its ends; (s, r) and (r, s) give the same bits; a plane against
    itself gives count << 32 exactly"""
    w, h = size
    for k, kind in enumerate(SR.KINDS):
        s, r = SR.pair(kind, w, h, 77 * w + h + k)
        n, d = SR.n_d(s, r)
        assert n.shape == SR.windows(w, h)[::-1]
        assert (d > 0).all(), kind
        v = SR.values(s, r)
        assert (np.abs(v) <= 1.0).all(), kind
        back = SR.values(r, s)
        assert np.array_equal(v.view(np.uint64), back.view(np.uint64)), kind
        assert SR.plane_scores(s, r) == SR.plane_scores(r, s)
        assert np.array_equal(SR.ssim_map([s] * 3, [r] * 3, 1, "f16").view(np.uint16), SR.ssim_map([r] * 3, [s] * 3, 1, "f16").view(np.uint16))
        for p in (s, r):
            total, count = SR.plane_scores(p, p)
            assert total == count << 32 and (SR.values(p, p) == 1.0).all()
    s, r = SR.pair("extremes", w, h, 0)
    assert (SR.values(s, r) > 0).all() and (SR.values(s, r) < 1e-3).all()       # c1 alone keeps the luminance term off zero
    s, r = SR.pair("antiphase", w, h, 0)
    assert (SR.values(s, r) < 0).all()                                          # negative covariance: the only way below zero


def test_scores_and_map_layout():
    """planes in bit order whatever order they are named in; a plane without windows has count 0, total 0 and no map elements"""
    w, h = 20, 18
    a = [SR.mixed_bytes(k, pw * ph).reshape(ph, pw) for k, (pw, ph) in enumerate(((w, h), (10, 9), (10, 9)))]
    b = [SR.mixed_bytes(9 + k, p.size).reshape(p.shape) for k, p in enumerate(a)]
    sc = SR.scores(a, b)
    assert sc.shape == (3, 2) and sc.dtype == np.int64 and sc[:, 1].tolist() == [3 * 3, 1 * 1, 1 * 1]
    assert np.array_equal(SR.scores(a, b, ("v", "y")), sc[[0, 2]]) and np.array_equal(SR.scores(a, b, 2), sc[[1]])
    m = SR.ssim_map(a, b)
    assert m.dtype == np.float32 and m.size == 11 == SR.map_elems(w, h)
    assert np.array_equal(m[:9].reshape(3, 3), SR.values(a[0], b[0]).astype(np.float32))
    assert np.array_equal(SR.ssim_map(a, b, 5), m[[0, 1, 2, 3, 4, 5, 6, 7, 8, 10]])
    assert SR.ssim_map(a, b, 7, "f16").dtype == np.float16
    small = [p[:8, :8] for p in a]
    assert SR.scores(small, small).tolist() == [[0, 0]] * 3 and SR.ssim_map(small, small).size == 0


def test_windows_through_the_library(pkg):
    """vp8hip_ssim_windows against the closed form and against counting the reference's loop, for every size 1..40 each way and
    16383; vp8hip_ssim_scores_size"""
    P = pkg
    L = P.load_hip()
    nwx, nwy = ctypes.c_int(), ctypes.c_int()
    sizes = list(range(1, 41)) + [16383]
    for w in sizes:
        for h in sizes:
            assert L.vp8hip_ssim_windows(w, h, ctypes.byref(nwx), ctypes.byref(nwy)) == 0
            assert (nwx.value, nwy.value) == SR.windows(w, h) == SR.loop_windows(w, h) == P.ssim_windows(w, h), (w, h)
    assert P.ssim_windows(16383, 16383) == (4094, 4094) and P.ssim_windows(8, 40) == (0, 8) and P.ssim_windows(9, 12) == (1, 1)
    for w, h in ((0, 16), (16, 0), (-1, 16), (16384, 16), (16, 16384)):
        nwx.value = nwy.value = 5
        assert L.vp8hip_ssim_windows(w, h, ctypes.byref(nwx), ctypes.byref(nwy)) == -2 and (nwx.value, nwy.value) == (0, 0)
        with pytest.raises(ValueError):
            P.ssim_windows(w, h)
    assert [L.vp8hip_ssim_scores_size(k) for k in (1, 2, 3)] == [16, 32, 48]
    for k in (0, -1, 4, 1 << 20):
        assert L.vp8hip_ssim_scores_size(k) == 0
    assert L.vp8hip_ssim_map_size(None, ctypes.byref(P.SsimParams(7, P.SSIM_F32))) == 0        # no context: no size
    assert L.vp8hip_ssim_share(None, 1, 7) == 0


def test_module_functions(pkg):
    """ssim_sizes, split_ssim_map, ssim_mean and ssim_combined need no device"""
    P = pkg
    assert ctypes.sizeof(P.SsimParams) == 8 and [f[0] for f in P.SsimParams._fields_] == ["planes", "map_dtype"]
    assert (P.SSIM_F16, P.SSIM_F32) == (1, 2)
    assert P.ssim_sizes(67, 45) == (48, 0)
    elems = SR.map_elems(67, 45)
    assert P.ssim_sizes(67, 45, ("y", "u", "v"), "float32") == (48, 4 * elems) and P.ssim_sizes(67, 45, 7, P.SSIM_F16) == (48, 2 * elems)
    assert P.ssim_sizes(67, 45, ("y",), np.dtype("float16")) == (16, 2 * SR.map_elems(67, 45, 1))
    assert P.ssim_sizes(16, 16, ("u", "v"), "float32") == (32, 0)
    assert P.ssim_sizes(67, 45, (), "float32") == (0, 0) and P.ssim_sizes(67, 45, 8) == (0, 0) and P.ssim_sizes(67, 45, 7, "uint8") == (0, 0)
    assert P.ssim_sizes(67, 45, 7, 0) == (0, 0) and P.ssim_sizes(67, 45, 7, 3) == (0, 0)
    flat = np.arange(2 * SR.map_elems(20, 18), dtype=np.float32).reshape(2, -1)
    y, u, v = P.split_ssim_map(flat, 20, 18)
    assert y.shape == (2, 3, 3) and u.shape == (2, 1, 1) == v.shape and v[1, 0, 0] == 21 and y[1, 2, 1] == 11 + 7
    y, v = P.split_ssim_map(flat[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]], 20, 18, ("v", "y"))
    assert y.shape == (2, 3, 3) and v[0, 0, 0] == 10
    empty = P.split_ssim_map(np.zeros((4, 4), np.float32), 16, 16)
    assert [e.shape for e in empty] == [(4, 2, 2), (4, 0, 0), (4, 0, 0)]
    with pytest.raises(ValueError):
        P.split_ssim_map(flat, 20, 22)
    with pytest.raises(ValueError):
        P.split_ssim_map(flat, 20, 18, ("y", "nope"))
    sc = np.array([[[3 << 31, 3], [0, 0], [-(5 << 30), 5]], [[7 << 32, 7], [1, 1], [0, 4]]], np.int64)
    mean = P.ssim_mean(sc)
    assert mean.dtype == np.float64 and mean.shape == (2, 3)
    assert mean[0, 0] == 0.5 and math.isnan(mean[0, 1]) and mean[0, 2] == -0.25 and mean[1].tolist() == [1.0, 2.0 ** -32, 0.0]
    assert np.isnan(mean).sum() == 1
    m = np.array([[0.9, 0.5, 0.25], [1.0, 1.0, 1.0]])
    assert np.array_equal(P.ssim_combined(m, "ssimg"), (m[:, 0] * 4 + m[:, 1] + m[:, 2]) / 6)
    assert np.array_equal(P.ssim_combined(m, "ssim"), m[:, 0] * .8 + .1 * (m[:, 1] + m[:, 2]))
    assert P.ssim_combined(m)[1] == 1.0 and P.ssim_combined([0.9, 0.5, 0.25], "ssim") == 0.9 * .8 + .1 * (0.5 + 0.25)
    for bad in (lambda: P.ssim_combined(m, "mean"), lambda: P.ssim_combined(m[:, :2]), lambda: P.ssim_mean(np.zeros((2, 3), np.int64))):
        with pytest.raises(ValueError):
            bad()
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrapper sees before the call
    for jobs, planes, dt in (([], ("y",), None), ([(0, 0)], (), None), ([(0, 0)], ("y", "nope"), None), ([(0, 0)], 8, None), ([0], 7, None),
                             ([(0, 1, 2)], 7, None), ([(0, -1)], 7, None), ([(-1, 0)], 7, None), ([(0, 0)], 7, "uint8"), ([(0, 0)], 7, 0),
                             ([(0, 0)], 7, 3)):
        with pytest.raises(ValueError):
            ctx.frames_ssim(jobs, planes, dt)


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    path = os.path.join(HERE, "..", "include", "vp8hip.h")
    with open(path) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_ssim_windows", "vp8hip_ssim_scores_size", "vp8hip_ssim_map_size", "vp8hip_frames_ssim_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert re.search(r"#define\s+VP8HIP_SSIM_F16\s+1\b", src) and re.search(r"#define\s+VP8HIP_SSIM_F32\s+2\b", src)
    assert re.search(r"typedef struct vp8hip_ssim\s*{\s*unsigned planes;\s*int map_dtype;\s*}", src)
