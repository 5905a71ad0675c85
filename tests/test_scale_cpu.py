"""The numpy restatement of libyuv's I420Scale (tests/scale_reference.py) against the listings the reference tree's own scaler
wrote (tests/golden/*.scale_*.md5, tests/golden/make_scale_fixtures.py), and the size formula of the C ABI.  No GPU."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from vp8_testlib import GOLDEN, load_package, oracle_decode_ivf
import scale_reference as S

LISTINGS = sorted(f for f in os.listdir(GOLDEN) if ".scale_" in f and f.endswith(".md5"))
CASE = re.compile(r"(.+)\.scale_(\d+)x(\d+)_f(\d)\.md5$")


def cases():
    out = {}
    for f in LISTINGS:
        name, w, h, flt = CASE.match(f).groups()
        out.setdefault(name, []).append((int(w), int(h), int(flt), f))
    return out


_shown = {}


def shown_frames(name):
    """(geometry, frame buffer) of every shown frame of a fixture, from the oracle"""
    if name not in _shown:
        P = load_package()
        _, kept = oracle_decode_ivf(name, keep_frames=True)
        _shown[name] = [(P.geom(hdr.width, hdr.height), hdr.width, hdr.height, buf) for hdr, _, _, _, buf in kept if hdr.show_frame]
    return _shown[name]


def test_listings_cover_every_path():
    luma, chroma = set(), set()
    for name, sizes in cases().items():
        w, h = (int(v) for v in name.rsplit("_", 1)[1].split("x"))
        for dw, dh, flt, _ in sizes:
            lp, cp = S.plan(w, h, dw, dh, flt)
            luma.add((lp, flt))
            chroma.add((cp, flt))
    want = {(n, f) for n in S.NAMES for f in (0, 1) if not (n in ("copy", "point") and f == 1) and not (n.startswith("bilinear") and f == 0)}
    assert want <= luma, sorted(want - luma)
    assert want <= chroma, sorted(want - chroma)


@pytest.mark.parametrize("name", sorted(cases()))
def test_restatement_reproduces_listings(name):
    frames = shown_frames(name)
    for dw, dh, flt, fname in cases()[name]:
        gold = [l.split()[0] for l in open(os.path.join(GOLDEN, fname))]
        assert len(gold) == len(frames), fname
        got = [hashlib.md5(S.scale_frame(buf, g, w, h, dw, dh, flt).tobytes()).hexdigest() for g, w, h, buf in frames]
        bad = [i for i, (a, b) in enumerate(zip(got, gold)) if a != b]
        assert not bad, f"{fname}: frames {bad[:8]} differ"


def test_box_filter_is_bilinear():
    """The restatement sends kFilterBox (2) down the paths of kFilterBilinear (1).  This pins the restatement's dispatch only; that
    the reference does the same is asserted by make_scale_fixtures.py (f2 == f1 on every listed case), and the device's f = 2 output
    is checked against the f = 1 listings in test_gpu_scale.py."""
    P = load_package()
    rng = np.random.default_rng(5)
    for w, h, dw, dh in ((67, 45, 34, 23), (64, 48, 48, 36), (64, 48, 24, 18), (176, 144, 22, 18), (130, 98, 65, 49), (32, 32, 100, 7)):
        g = P.geom(w, h)
        buf = rng.integers(0, 256, g.frame_size, dtype=np.uint8)
        assert np.array_equal(S.scale_frame(buf, g, w, h, dw, dh, 2), S.scale_frame(buf, g, w, h, dw, dh, 1)), (w, h, dw, dh)


def test_i420_size_abi():
    P = load_package()
    if not os.path.exists(P.HIP_LIB):
        pytest.skip("libvp8hip.so not built")
    L = ctypes.CDLL(P.HIP_LIB)
    L.vp8hip_i420_size.restype = ctypes.c_size_t
    L.vp8hip_i420_size.argtypes = [ctypes.c_int, ctypes.c_int]
    for w, h in ((1, 1), (2, 2), (67, 45), (1920, 1080), (16383, 16383), (17, 9)):
        assert L.vp8hip_i420_size(w, h) == S.i420_size(w, h) == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    assert L.vp8hip_i420_size(0, 5) == 0 and L.vp8hip_i420_size(5, 16384) == 0
