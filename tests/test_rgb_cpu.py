"""The numpy restatement of the colour conversion (tests/rgb_reference.py) against the exact float64 matrices and on fixed points,
and the size formula of the C ABI (vp8hip_rgb_size is pure: no GPU)."""
import ctypes
import itertools

import numpy as np
import pytest

import rgb_reference as R
import scale_reference as S


@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
def test_integers_within_one_of_the_exact_matrix(matrix):
    """all 2^24 (Y, U, V): every channel within 1 of clamp(rint(exact float64 matrix))"""
    yoff, ky, rows = R.exact_matrix(matrix)
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = [0, 0, 0]
    for y in range(256):
        got = R.rgb_bytes(np.full_like(u, y), u, v, matrix)
        for c in range(3):
            exact = ky * (y - yoff) + rows[c][0] * (u - 128.0) + rows[c][1] * (v - 128.0)
            want = np.clip(np.rint(exact), 0, 255).astype(np.int64)
            worst[c] = max(worst[c], int(np.abs(got[c] - want).max()))
    assert max(worst) <= 1, (matrix, worst)


def test_constants_are_the_rounded_matrices():
    for matrix, (yoff, cy, crv, cgu, cgv, cbu) in R.MATRICES.items():
        eoff, ky, rows = R.exact_matrix(matrix)
        assert yoff == eoff
        assert (cy, crv, cgu, cgv, cbu) == tuple(int(np.rint(256 * k)) for k in (ky, rows[0][1], rows[1][0], rows[1][1], rows[2][0])), matrix


def one(y, u, v, matrix):
    return tuple(int(c) for c in R.rgb_bytes(y, u, v, matrix))


def test_fixed_points():
    for m in ("bt601", "bt709"):
        assert one(16, 128, 128, m) == (0, 0, 0)
        assert one(235, 128, 128, m) == (255, 255, 255)
        assert one(126, 128, 128, m) == (128, 128, 128)
    assert one(255, 128, 128, "bt601-full") == (255, 255, 255)
    assert one(0, 128, 128, "bt601-full") == (0, 0, 0)
    assert one(77, 128, 128, "bt601-full") == (77, 77, 77)
    for m in R.MATRICES:                          # out of range: clamped
        assert one(0, 0, 0, m) == (0, {"bt601": 135, "bt601-full": 136, "bt709": 77}[m], 0), m
        assert one(255, 255, 255, m)[0] == 255 and one(255, 255, 255, m)[2] == 255
        assert all(0 <= c <= 255 for yuv in itertools.product((0, 255), repeat=3) for c in one(*yuv, m))
    # pure red of BT.601 limited range (Y 81, U 90, V 240)
    r, g, b = one(81, 90, 240, "bt601")
    assert r >= 254 and g <= 1 and b <= 1


def test_chroma_is_replicated():
    # 3x3: 9 luma, 2x2 chroma; 5x1: 5 luma, 3x1 chroma
    for w, h in ((3, 3), (5, 1)):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        rng = np.random.default_rng(w * 10 + h)
        packed = rng.integers(0, 256, S.i420_size(w, h), dtype=np.uint8)
        out = R.convert(packed, w, h, "bt601-full")
        assert out.shape == (3, h, w) and out.dtype == np.uint8
        y = packed[:w * h].reshape(h, w)
        u = packed[w * h:w * h + cw * ch].reshape(ch, cw)
        v = packed[w * h + cw * ch:].reshape(ch, cw)
        for yy in range(h):
            for xx in range(w):
                assert tuple(out[:, yy, xx]) == one(y[yy, xx], u[yy // 2, xx // 2], v[yy // 2, xx // 2], "bt601-full")
    # equal luma, one chroma sample: the four pixels of a 2x2 block are equal
    packed = np.array([100, 100, 100, 100, 60, 200], np.uint8)
    out = R.convert(packed, 2, 2)
    assert (out == out[:, :1, :1]).all()


def test_layouts_and_orders_on_a_2x2_image():
    packed = np.array([16, 81, 145, 235, 90, 240], np.uint8)           # Y: black, red's, green's, white levels; U, V of red
    px = [one(y, 90, 240, "bt601") for y in (16, 81, 145, 235)]       # pixels (0,0) (1,0) (0,1) (1,1) as (R, G, B)
    assert px[1][0] >= 254 and px[1][1] <= 1
    planar = R.convert(packed, 2, 2, layout="planar")
    assert planar.shape == (3, 2, 2)
    assert [tuple(planar[:, y, x]) for y in (0, 1) for x in (0, 1)] == px
    bgr = R.convert(packed, 2, 2, layout="planar", order="bgr")
    assert np.array_equal(bgr, planar[::-1])
    p3 = R.convert(packed, 2, 2, layout="packed3")
    assert p3.shape == (2, 2, 3) and p3.tobytes() == bytes(c for p in px for c in p)
    p3b = R.convert(packed, 2, 2, layout="packed3", order="bgr")
    assert p3b.tobytes() == bytes(c for p in px for c in p[::-1])
    p4 = R.convert(packed, 2, 2, layout="packed4")
    assert p4.shape == (2, 2, 4) and p4.tobytes() == bytes(c for p in px for c in p + (255,))
    p4b = R.convert(packed, 2, 2, layout="packed4", order="bgr")
    assert p4b.tobytes() == bytes(c for p in px for c in p[::-1] + (255,))


def test_float_definition_on_every_byte():
    scale, bias = R.scale_bias(R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert scale.dtype == np.float32 and bias.dtype == np.float32
    v = np.arange(256)
    for c in range(3):
        f32 = R.element(v, scale[c], bias[c], "f32")
        f16 = R.element(v, scale[c], bias[c], "f16")
        assert f32.dtype == np.float32 and f16.dtype == np.float16
        for b in range(256):
            d = float(b) * float(scale[c]) + float(bias[c])          # python floats are doubles: one rounding of the sum
            assert f32[b] == np.float32(d) and f16[b] == np.float16(np.float32(d))
        # close to the textbook normalisation, and monotonic
        assert np.allclose(f32, (v / 255.0 - R.IMAGENET_MEAN[c]) / R.IMAGENET_STD[c], atol=1e-5)
        assert (np.diff(f32) > 0).all() and (np.diff(f16.astype(np.float32)) >= 0).all()
    # by colour, not by position: BGR planes carry the colours' own pairs
    packed = np.array([16, 81, 145, 235, 90, 240], np.uint8)
    rgb = R.convert(packed, 2, 2, dtype="f32", scale=scale, bias=bias)
    bgr = R.convert(packed, 2, 2, dtype="f32", order="bgr", scale=scale, bias=bias)
    assert np.array_equal(rgb[::-1], bgr)
    u8 = R.convert(packed, 2, 2)
    assert np.array_equal(rgb[1], R.element(u8[1], scale[1], bias[1], "f32"))
    # defaults: v / 255 rounded once
    s1, b0 = R.scale_bias()
    assert np.array_equal(R.element(v, s1[0], b0[0], "f32"), np.float32(v.astype(np.float64) * np.float64(np.float32(1.0 / 255.0))))


def params(pkg, w, h, filt=1, matrix=0, layout=0, order=0, dtype=0):
    return pkg.RgbParams(w, h, filt, matrix, layout, order, dtype)


def test_rgb_size_abi(pkg):
    """vp8hip_rgb_size through ctypes, for every layout / type and its zeros, equal to the package's rgb_size"""
    L = ctypes.CDLL(pkg.HIP_LIB)
    L.vp8hip_rgb_size.restype = ctypes.c_size_t
    L.vp8hip_rgb_size.argtypes = [ctypes.POINTER(pkg.RgbParams)]

    def size(*a, **k):
        return L.vp8hip_rgb_size(ctypes.byref(params(pkg, *a, **k)))
    py_layout = {"planar": "nchw", "packed3": "nhwc", "packed4": "nhwc4"}
    for w, h in ((1, 1), (2, 2), (67, 45), (224, 224), (1920, 1080), (16383, 16383), (17, 9)):
        for layout, lid in R.LAYOUTS.items():
            for dtype, did in R.DTYPES.items():
                got = size(w, h, layout=lid, dtype=did)
                if layout == "packed4" and dtype != "u8":
                    assert got == 0 == pkg.rgb_size(w, h, py_layout[layout], did)
                    continue
                want = w * h * (4 if layout == "packed4" else 3) * (1, 2, 4)[did]
                assert got == want == R.frame_size(w, h, layout, dtype) == pkg.rgb_size(w, h, py_layout[layout], did), (w, h, layout, dtype)
                assert pkg.rgb_size(w, h, py_layout[layout], R.NP_DTYPES[dtype].__name__) == want
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-3, 5)):
        assert size(w, h) == 0 == pkg.rgb_size(w, h)
    assert size(8, 8) == 192
    for bad in (dict(filt=-1), dict(filt=3), dict(matrix=-1), dict(matrix=3), dict(layout=-1), dict(layout=3), dict(order=-1), dict(order=2),
                dict(dtype=-1), dict(dtype=3)):
        assert size(8, 8, **bad) == 0, bad
    assert L.vp8hip_rgb_size(None) == 0
    assert pkg.rgb_size(8, 8, "chw") == 0 and pkg.rgb_size(8, 8, "nchw", 7) == 0
