"""CPU: the definition of trace wear and of its tensor (vp8hip_frames_wear_async, vp8hip_trace_wear_async, include/vp8hip.h) as
tests/wear_reference.py restates it -- CODED and EDGE pinned by the oracle decoder on hand-built frames with coefficients, every
counter exercised over the fixtures, the special cases, the tensor and the library's size function."""
import ctypes

import numpy as np
import pytest

from vp8_testlib import oracle_decode
import trace_reference as R
import wear_reference as W
from trace_testlib import SPLITMV, frames_of, luma, make_hdr, whole_pixel_frame


def coded_frame(P, w, h, rng):
    """whole_pixel_frame with about two thirds of the macroblocks not skipped and coefficients in random luma blocks: beside a Y2
    block one at dense index 4 (eobs 2) or nothing of the block's own (eobs 1), in SPLITMV macroblocks a lone DC (eobs 1) or a DC
    and one more (eobs 2); half the macroblocks with a Y2 block give it one or two coefficients.  -> (hdr, mbs, coef, mvs)"""
    hdr, mbs, mvs = whole_pixel_frame(P, w, h, rng)
    nmb = len(mbs)
    coef = np.zeros((nmb, 400), np.int16)

    def value(n=None):
        return (rng.integers(40, 90, n) * rng.choice([-1, 1], n)).astype(np.int16)
    for i in range(nmb):
        if rng.random() < 1 / 3:
            continue
        mbs[i, W.O_FLAGS] &= ~np.uint8(W.MB_SKIP)
        eobs = mbs[i, W.O_EOBS:W.O_EOBS + 25]
        split = mbs[i, W.O_MODE] == SPLITMV
        for k in range(16):
            u = rng.random()
            if split:
                if u < 0.25:
                    eobs[k], coef[i, 16 * k] = 1, value()
                elif u < 0.5:
                    eobs[k] = 2
                    coef[i, 16 * k], coef[i, 16 * k + 4] = value(), value()
            elif u < 0.25:
                eobs[k], coef[i, 16 * k + 4] = 2, value()
            elif u < 0.6:
                eobs[k] = 1
        if not split and rng.random() < 0.5:
            eobs[24] = rng.integers(1, 3)
            coef[i, 384] = value()
            if eobs[24] == 2:
                coef[i, 388] = value()
    return hdr, mbs, coef, mvs


@pytest.mark.parametrize("size", [(16, 16), (67, 45), (176, 144)])
def test_oracle_pins_coded_and_edge(pkg, size):
    """the oracle decoder reconstructs such a frame from three random pictures: every display pixel whose CODED increment is 0 is
    ref[r][sy, sx] exactly -- a zero luma residual --, most of the others are not; the EDGE increment is "hop's clamp moved the
    position" """
    P = pkg
    w, h = size
    rng = np.random.default_rng(w * 977 + h)
    g = P.geom(w, h)
    for attempt in range(8):                             # (a lone macroblock: until it is one that is not skipped)
        hdr, mbs, coef, mvs = coded_frame(P, w, h, rng)
        inc = W.incs(hdr, mbs, mvs)
        if inc[W.CODED].any() and not inc[W.CODED].all():
            break
    pics, bufs = [], []
    for _ in range(3):
        pic = rng.integers(0, 256, (h, w)).astype(np.uint8)
        buf = np.zeros(g.frame_size, np.uint8)
        luma(buf, g, g.aligned_h, g.aligned_w, 32)[:] = np.pad(pic, ((32, g.aligned_h - h + 32), (32, g.aligned_w - w + 32)), "edge")
        pics.append(pic)
        bufs.append(buf)
    dst = np.zeros(g.frame_size, np.uint8)
    oracle_decode(hdr, mbs, coef, mvs, dst, bufs, stages=1)
    r, sy, sx = R.hop(hdr, mbs, mvs)
    pred = np.zeros((h, w), np.uint8)
    for q in (1, 2, 3):
        pred[r == q] = pics[q - 1][sy[r == q], sx[r == q]]
    got = luma(dst, g, h, w)
    coded = inc[W.CODED] != 0
    assert coded.any() and (~coded).any(), size
    assert np.array_equal(got[~coded], pred[~coded]), (size, int((got != pred)[~coded].sum()))
    changed = (got != pred)[coded]
    print(f"{size}: CODED share {coded.mean():.3f}, changed share of CODED {changed.mean():.3f}")
    assert 2 * int(changed.sum()) > int(coded.sum()), (size, int(changed.sum()), int(coded.sum()))
    # EDGE: whole-pixel vectors, so the unclamped position is the pixel plus the vector
    ys, xs = np.mgrid[0:h, 0:w]
    v = mvs[(ys >> 4) * hdr.mb_cols + (xs >> 4), ((ys >> 2) & 3) * 4 + ((xs >> 2) & 3)].astype(int) >> 3
    moved = (xs + v[..., 1] != sx) | (ys + v[..., 0] != sy)
    assert np.array_equal(inc[W.EDGE] != 0, moved) and moved.any() and not moved.all()
    assert (inc[W.HOPS] == 1).all() and not inc[W.INTRA].any()


PINNED_MAXIMA = {"p_arf_176x144": (56, 30, 11, 31), "p_prof1_640x360": (9, 7, 9, 9), "p_odd_130x98": (7, 7, 4, 7),
                 "p_split_352x288": (11, 8, 11, 11)}


@pytest.mark.parametrize("name", sorted(PINNED_MAXIMA))
def test_every_counter_is_exercised_on_the_fixtures(pkg, name):
    """the fixture chained with the restatement, the pool numbered like the frame buffers: every counter goes above zero, HOPS is at
    least each of the others pixel by pixel, and the maxima are pinned"""
    P = pkg
    pool, top = {}, np.zeros(4, int)
    for hdr, mbs, mvs, (new, lst, gld, alt) in frames_of(P, name):
        pool[new] = W.wear(hdr, mbs, mvs, [pool.get(lst), pool.get(gld), pool.get(alt)])
        c = W.unpack(pool[new])
        assert (c[W.HOPS] >= c[1:]).all()
        if hdr.frame_type == 0:
            assert not pool[new].any()
        top = np.maximum(top, c.reshape(4, -1).max(1))
    print(name, tuple(top.tolist()))
    assert (top > 0).all(), (name, top)
    assert tuple(top.tolist()) == PINNED_MAXIMA[name]


def test_key_frames_missing_references_intra_and_saturation(pkg):
    P = pkg
    w, h = 67, 45
    rng = np.random.default_rng(5)
    hdr, mbs, coef, mvs = coded_frame(P, w, h, rng)
    mvs += rng.integers(-7, 8, mvs.shape).astype(np.int16)          # sub-pixel parts
    junk = [rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32) & 0x7f7f7f7f for _ in range(3)]      # (counters below 128: no saturation)
    # a key frame is zero whatever the references and the vector area hold
    key = make_hdr(P, w, h, frame_type=0)
    assert not W.wear(key, mbs, mvs, junk).any() and not W.wear(key, mbs, mvs, [None] * 3).any()
    # a reference of -1: zero where a macroblock names it, the chained value elsewhere
    r, sy, sx = R.hop(hdr, mbs, mvs)
    inc = W.incs(hdr, mbs, mvs)
    for q in (1, 2, 3):
        refs = list(junk)
        refs[q - 1] = None
        t = W.wear(hdr, mbs, mvs, refs)
        assert not t[r == q].any() and (r == q).any()
        for o in {1, 2, 3} - {q}:
            sel = r == o
            assert np.array_equal(t[sel], junk[o - 1][sy[sel], sx[sel]] + W.pack(inc[:, sel]))
    assert not W.wear(hdr, mbs, mvs, [None] * 3).any()
    # an unknown ref_frame: zero, as the trace is the identity there
    odd = mbs.copy()
    odd[1::3, W.O_REF] = 4
    t = W.wear(hdr, odd, mvs, junk)
    is_odd = (np.arange(len(mbs)) % 3 == 1).reshape(hdr.mb_rows, hdr.mb_cols).repeat(16, 0).repeat(16, 1)[:h, :w]
    assert not t[is_odd].any() and np.array_equal(t[~is_odd], W.wear(hdr, mbs, mvs, junk)[~is_odd])
    # intra macroblocks: INTRA goes up, EDGE does not, and the position is held whatever their vectors
    intra = mbs.copy()
    intra[::2, W.O_REF] = 0
    held = (np.arange(len(mbs)) % 2 == 0).reshape(hdr.mb_rows, hdr.mb_cols).repeat(16, 0).repeat(16, 1)[:h, :w]
    ii = W.incs(hdr, intra, mvs)
    assert (ii[W.INTRA] == held).all() and not ii[W.EDGE][held].any() and inc[W.EDGE][held].any()
    assert np.array_equal(ii[W.CODED], inc[W.CODED]) and np.array_equal(ii[W.EDGE][~held], inc[W.EDGE][~held])
    t = W.wear(hdr, intra, mvs, junk)
    assert np.array_equal(t[held], junk[0][held] + W.pack(ii[:, held]))
    assert np.array_equal(t[~held], W.wear(hdr, mbs, mvs, junk)[~held])
    # a skipped macroblock has no CODED whatever its eobs say
    skipped = mbs.copy()
    skipped[:, W.O_FLAGS] |= W.MB_SKIP
    assert inc[W.CODED].any() and not W.incs(hdr, skipped, mvs)[W.CODED].any()
    # saturation: 254 goes to 255 where the increment is 1, 255 stays, and nothing wraps into a neighbour
    for fill in (254, 255):
        full = [np.full((h, w), fill * 0x01010101, np.uint32)] * 3
        c = W.unpack(W.wear(hdr, intra, mvs, full))
        assert np.array_equal(c, np.minimum(fill + ii.astype(int), 255))
        assert (c[W.HOPS] == 255).all() and c.min() >= fill
    mixed = [np.full((h, w), 0xfe00fffe, np.uint32)] * 3
    c = W.unpack(W.wear(hdr, intra, mvs, mixed))
    assert (c[0] == 255).all() and (c[1] == 255).all() and np.array_equal(c[2], ii[2]) and np.array_equal(c[3], 254 + ii[3])


def test_block_kinds_are_vp8ir_block_kind():
    """the restatement's table against the C helper's rules, case by case"""
    m = np.zeros((6, 64), np.uint8)
    m[:, W.O_MODE] = (0, 0, W.SPLITMV, W.B_PRED, 0, W.SPLITMV)
    m[:, W.O_EOBS] = (1, 2, 1, 2, 2, 1)                  # luma block 0
    m[:, W.O_EOBS + 24] = (0, 1, 1, 2, 2, 0)
    m[4:, W.O_FLAGS] = W.MB_SKIP
    k = W.block_kinds(m)
    assert k[:, 0].tolist() == [0, 2, 1, 2, 0, 0]        # (beside a Y2 block a luma block starts at 1: eob 1 is nothing)
    assert k[:, 24].tolist() == [0, 1, 0, 0, 0, 0]       # (no Y2 block in SPLITMV / B_PRED; nothing in a skipped macroblock)
    assert not k[:, 1:24].any()


def test_tensor_restatement():
    rng = np.random.default_rng(11)
    w, h = 130, 98
    t = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    c = W.unpack(t)
    assert np.array_equal(W.pack(c), t)
    at = W.tensor(t)
    assert at.shape == (4, h, w) and at.dtype == np.uint8 and np.array_equal(at, c)
    # a subset comes in bit order, however it is named
    two = W.tensor(t, planes=("coded", "intra"))
    assert two.shape == (2, h, w) and np.array_equal(two[0], c[W.INTRA]) and np.array_equal(two[1], c[W.CODED])
    assert np.array_equal(W.tensor(t, planes=W.PLANES["coded"] | W.PLANES["intra"]), two)
    assert np.array_equal(W.tensor(t, planes=("edge",))[0], c[W.EDGE])
    # the centre map
    sx, sy = R.grid_map(224, w), R.grid_map(224, h)
    f = W.tensor(t, 224, 224, 15, "f32", (0.5, 1.0 / 3, 2.0, 1e-3))
    assert f.shape == (4, 224, 224) and f.dtype == np.float32
    for k, s in enumerate((0.5, 1.0 / 3, 2.0, 1e-3)):
        assert np.array_equal(f[k], (c[k][sy][:, sx].astype(np.float64) * np.float64(np.float32(s))).astype(np.float32))
    one = W.tensor(t, 1, 1, ("hops", "coded"), "f16", (0.25, 9.0, 9.0, 3.0))       # 1x1: the centre pixel; the scale goes by counter
    assert one.shape == (2, 1, 1) and one.dtype == np.float16
    assert one[0, 0, 0] == np.float16(int(c[0, h // 2, w // 2]) * 0.25) and one[1, 0, 0] == np.float16(int(c[3, h // 2, w // 2]) * 3.0)
    odd = W.tensor(t, w + 1, h - 1)
    assert odd.shape == (4, h - 1, w + 1) and np.array_equal(odd, c[:, R.grid_map(h - 1, h)][:, :, R.grid_map(w + 1, w)])
    # the half is the float rounded: two roundings
    s = np.float32(1.0285249948501587)
    v = np.arange(256, dtype=np.uint32).reshape(16, 16)
    got = W.tensor(v, planes=1, dtype="f16", scale=(s, 0, 0, 0))[0]
    assert np.array_equal(got, (v.astype(np.float64) * np.float64(s)).astype(np.float32).astype(np.float16))
    assert W.tensor_size(w, h) == 4 * w * h and W.tensor_size(w, h, 224, 224, ("hops", "edge"), "f32") == 2 * 224 * 224 * 4


def test_size_function_of_the_library(pkg):
    P = pkg
    L = P.load_hip()

    def lib(w, h, dtype=0, planes=15):
        return int(L.vp8hip_trace_wear_size(None, ctypes.byref(P.TraceWearParams(w, h, dtype, planes))))
    for w, h in ((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3)):
        for dt, name in enumerate(("u8", "f16", "f32")):
            for planes in (15, 1, 10, 8):
                assert lib(w, h, dt, planes) == W.tensor_size(0, 0, w, h, planes, name), (w, h, name, planes)
                assert P.trace_wear_size(w, h, planes, dt) == lib(w, h, dt, planes)
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (0, 0)):       # (0 x 0: the display size needs a context)
        assert lib(w, h) == 0, (w, h)
    for dt in (-1, 3):
        assert lib(8, 8, dt) == 0
    for planes in (0, 16, 31, 1 << 31):
        assert lib(8, 8, 0, planes) == 0, planes
    assert L.vp8hip_trace_wear_size(None, None) == 0
    assert P.trace_wear_size(8, 8, ("coded", "hops"), "float16") == 2 * 64 * 2 and P.trace_wear_size(8, 8, ("nope",)) == 0
    assert P.trace_wear_size(8, 8, (), 0) == 0 and P.trace_wear_size(8, 8, 15, "int16") == 0 and P.trace_wear_size(0, 0) == 0
    # the struct as the header lays it out: two ints, an int, an unsigned, four floats
    assert ctypes.sizeof(P.TraceWearParams) == 32
    assert [f[0] for f in P.TraceWearParams._fields_] == ["dst_w", "dst_h", "dtype", "planes", "scale"]
    assert P.TraceWearParams.scale.offset == 16 and P.TraceWearParams.planes.offset == 12
    assert P.WEAR_PLANES == W.PLANES
