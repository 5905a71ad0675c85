"""CPU: the definition of the side-information tensors (vp8hip_frames_side_async, include/vp8hip.h) as tests/side_reference.py
restates it -- the size functions of the library through ctypes, the grid map, the float definition on every int16, hand-built
macroblocks for every info plane, and the fixtures' frames through the host parser."""
import ctypes
import itertools

import numpy as np
import pytest

from vp8_testlib import ivf_path
import side_reference as R

STREAMS = ["p_split_352x288", "p_arf_176x144", "p_seg_176x144", "p_roi_640x360", "p_odd_130x98"]
DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED, NEARESTMV, NEARMV, ZEROMV, NEWMV, SPLITMV = range(10)


def make_hdr(P, w, h, frame_type=1, **kw):
    hdr = P.FrameHdr()
    hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows, hdr.frame_type = w, h, (w + 15) // 16, (h + 15) // 16, frame_type
    for k, v in kw.items():
        if k == "segment_quant":
            for s in range(4):
                hdr.segment_quant[s] = v[s]
        else:
            setattr(hdr, k, v)
    return hdr


def test_size_functions_of_the_library(pkg):
    P = pkg
    L = P.load_hip()

    def lib(w, h, dtype=0, planes=0):
        p = P.SideParams(w, h, dtype, planes)
        return int(L.vp8hip_side_mv_size(None, ctypes.byref(p))), int(L.vp8hip_side_info_size(None, ctypes.byref(p)))
    hdr = make_hdr(P, 64, 48)
    for (w, h), (dt, name), planes in itertools.product(((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3), (16383, 1)),
                                                        enumerate(("i16", "f16", "f32")), (0, 1, 7, 63, 0b101010)):
        want = R.sizes(hdr, w, h, name, planes)
        assert lib(w, h, dt, planes) == want, (w, h, name, planes)
        assert P.side_sizes(w, h, dt, planes) == want
    assert lib(5, 4, 2, 63) == (2 * 4 * 5 * 4, 6 * 4 * 5)
    # everything the call refuses on the parameters alone: zero
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (-3, 5)):
        assert lib(w, h) == (0, 0), (w, h)
        assert P.side_sizes(w, h) == (0, 0)
    for dt in (-1, 3):
        assert lib(8, 8, dt, 1) == (0, 0)
    for planes in (64, 128, 1 << 31, 0xffffffff):
        assert lib(8, 8, 0, planes) == (0, 0)
    assert lib(0, 0) == (0, 0)                          # the native grid needs a context
    assert L.vp8hip_side_mv_size(None, None) == 0 and L.vp8hip_side_info_size(None, None) == 0
    assert P.side_sizes(8, 8, "float32", ("coded", "ref")) == (2 * 64 * 4, 2 * 64)
    assert P.side_sizes(8, 8, "int8") == (0, 0) and P.side_sizes(8, 8, planes=("nope",)) == (0, 0)


def test_grid_map():
    for d in range(1, 65):
        x = np.arange(d)
        assert np.array_equal(R.grid_map(d, d), x)       # at the display size the pixel itself: cell (x >> 2, y >> 2)
        for dst in range(1, 65):
            m = R.grid_map(dst, d)
            assert m.min() >= 0 and m.max() < d, (dst, d)
            assert (np.diff(m) >= 0).all(), (dst, d)
    # the extremes stay inside, in the integers the kernel uses (below 2^31)
    for dst, d in ((16383, 16383), (1, 16383), (16383, 1), (16383, 16382)):
        m = R.grid_map(dst, d)
        assert m.min() >= 0 and m.max() < d and int((2 * (dst - 1) + 1) * d) < 2 ** 31


def test_float_definition_on_every_int16():
    v = np.arange(-32768, 32768, dtype=np.int64)
    both = np.stack([v, v[::-1]]).astype(np.int16)
    for sx, sy in ((1.0, 1.0), (0.125, 0.125), (0.125 * 224 / 1920, 0.125 * 224 / 1080), (-1.0 / 3, 1e-3), (2.0 ** -20, 3.0e4), (1.0 / 7, 65504.0 / 32767)):
        scale = (np.float32(sx), np.float32(sy))
        f32 = R.convert(both, "f32", scale)
        f16 = R.convert(both, "f16", scale)
        assert f32.dtype == np.float32 and f16.dtype == np.float16
        for c in range(2):
            # the product of an int16 and a float32 has at most 40 significant bits: exact in double, one rounding to float
            exact = [int(a) * float(scale[c]) for a in both[c][::257]]
            assert all(np.float32(e) == g for e, g in zip(exact, f32[c][::257]))
            # ... so a single-precision multiply gives the same bits
            assert np.array_equal((both[c].astype(np.float32) * scale[c]).view(np.uint32), f32[c].view(np.uint32))
        # the half is the FLOAT rounded to nearest-even (numpy's astype), ties and overflow to infinity included
        with np.errstate(over="ignore"):
            assert np.array_equal(f16.view(np.uint16), f32.astype(np.float16).view(np.uint16))
    tie = np.float32(1.0 + 2.0 ** -11)                   # halfway between two halves: to the even one
    assert R.convert(np.array([[1], [2]], np.int16), "f16", (tie, tie)).tolist() == [[1.0], [2.0]]
    tie = np.float32(1.0 + 3 * 2.0 ** -11)
    assert R.convert(np.array([[1], [2]], np.int16), "f16", (tie, tie)).tolist() == [[1.001953125], [2.00390625]]
    assert R.convert(np.array([[0], [0]], np.int16), "f32", (-1.0, 1.0)).view(np.uint32).tolist() == [[0x80000000], [0]]
    # two roundings, not one: the exact product straight to a half differs where the float lands on a tie of the halves
    s = np.float32(1.0285249948501587)
    v = np.array([[-17213], [-17213]], np.int16)
    twice = R.convert(v, "f16", (s, s))
    once = (v.astype(np.float64) * np.float64(s)).astype(np.float16)
    assert np.array_equal(twice, R.convert(v, "f32", (s, s)).astype(np.float16)) and (twice != once).all()
    # denormal floats are kept
    tiny = R.convert(np.array([[3], [-5]], np.int16), "f32", (np.float32(1e-42), np.float32(1e-42)))
    assert tiny.view(np.uint32).tolist() == [[3 * 714], [0x80000000 + 5 * 714]]


def _blank(nmb):
    mbs = np.zeros((nmb, 64), np.uint8)
    mvs = np.zeros((nmb, 16, 2), np.int16)
    return mbs, mvs


def test_hand_built_modes_and_partitionings(pkg):
    P = pkg
    hdr = make_hdr(P, 64, 32, base_qindex=40)            # 4 x 2 macroblocks
    mbs, mvs = _blank(8)
    rng = np.random.default_rng(7)
    # macroblock 0: B_PRED, the ten sub-block modes; intra: whatever the vector array holds, the flow is zero
    mbs[0, R.O_Y_MODE], mbs[0, R.O_REF] = B_PRED, 0
    mbs[0, R.O_B_MODES:R.O_B_MODES + 16] = np.arange(16) % 10
    mvs[0] = rng.integers(-500, 500, (16, 2))
    # macroblocks 1..4: SPLITMV with the four partitionings (16x8, 8x16, 8x8, 4x4): a vector per partition
    split = [np.repeat(np.arange(2), 8), np.tile(np.repeat(np.arange(2), 2), 4),
             (np.arange(16) // 8) * 2 + (np.arange(16) % 4) // 2, np.arange(16)]
    for i, part in enumerate(split):
        mb = 1 + i
        mbs[mb, R.O_Y_MODE], mbs[mb, R.O_REF], mbs[mb, 5] = SPLITMV, 1 + i % 3, i
        vec = rng.integers(-2000, 2000, (16, 2))
        mvs[mb] = vec[part]
    # 5: NEWMV from golden, one vector; 6: ZEROMV; 7: DC_PRED intra
    mbs[5, R.O_Y_MODE], mbs[5, R.O_REF] = NEWMV, 2
    mvs[5] = (-32768, 32767)
    mbs[6, R.O_Y_MODE], mbs[6, R.O_REF] = ZEROMV, 3
    mbs[7, R.O_Y_MODE], mbs[7, R.O_REF] = DC_PRED, 0
    mvs[7] = 77
    mv, info = R.side(hdr, mbs, mvs, planes=63)
    assert mv.shape == (2, 8, 16) and info.shape == (6, 8, 16) and mv.dtype == np.int16 and info.dtype == np.uint8
    ref, mode = info[0], info[1]
    assert (mv[:, 0:4, 0:4] == 0).all() and (mv[:, 4:8, 12:16] == 0).all()         # the intra macroblocks
    assert np.array_equal(mode[0:4, 0:4], 10 + (np.arange(16) % 10).reshape(4, 4))
    assert (ref[0:4, 0:4] == 0).all() and (mode[4:8, 12:16] == DC_PRED).all()
    for i in range(4):
        mb = 1 + i
        y0, x0 = 4 * (mb // 4), 4 * (mb % 4)
        assert np.array_equal(mv[0, y0:y0 + 4, x0:x0 + 4], mvs[mb, :, 1].reshape(4, 4))      # x = col
        assert np.array_equal(mv[1, y0:y0 + 4, x0:x0 + 4], mvs[mb, :, 0].reshape(4, 4))      # y = row
        assert (mode[y0:y0 + 4, x0:x0 + 4] == SPLITMV).all() and (ref[y0:y0 + 4, x0:x0 + 4] == 1 + i % 3).all()
    # 16x8: the upper and the lower half; 8x16: left and right; 8x8: quadrants
    assert len({tuple(v) for v in mv[:, 0:2, 4:8].reshape(2, -1).T}) == 1 and len({tuple(v) for v in mv[:, 2:4, 4:8].reshape(2, -1).T}) == 1
    assert len({tuple(v) for v in mv[:, 0:4, 8:10].reshape(2, -1).T}) == 1 and len({tuple(v) for v in mv[:, 0:4, 10:12].reshape(2, -1).T}) == 1
    for qy, qx in itertools.product((0, 2), (0, 2)):
        assert len({tuple(v) for v in mv[:, qy:qy + 2, 12 + qx:14 + qx].reshape(2, -1).T}) == 1
    assert (mv[0, 4:8, 4:8] == 32767).all() and (mv[1, 4:8, 4:8] == -32768).all() and (ref[4:8, 4:8] == 2).all()
    assert (mv[:, 4:8, 8:12] == 0).all() and (ref[4:8, 8:12] == 3).all() and (mode[4:8, 8:12] == ZEROMV).all()
    assert (info[4] == 40).all()                         # segmentation off: base_qindex everywhere
    # a key frame: zero flow whatever the array holds
    key = make_hdr(P, 64, 32, frame_type=0)
    assert (R.side(key, mbs, mvs)[0] == 0).all()
    # sized grids pick the cell under the output's centre: at the display size (y >> 2, x >> 2)
    mvd, infod = R.side(hdr, mbs, mvs, 64, 32, planes=63)
    assert np.array_equal(mvd, mv.repeat(4, 1).repeat(4, 2)) and np.array_equal(infod, info.repeat(4, 1).repeat(4, 2))
    mv1, info1 = R.side(hdr, mbs, mvs, 1, 1, planes=3)   # 1x1: the centre pixel (32, 16): block (4, 8) = macroblock 6
    assert mv1.shape == (2, 1, 1) and info1[:, 0, 0].tolist() == [3, ZEROMV]


def test_hand_built_skip_and_coded_kinds(pkg):
    P = pkg
    hdr = make_hdr(P, 48, 16)
    mbs, mvs = _blank(3)
    eobs = np.array([0, 1, 2, 16, 0, 1, 1, 3, 0, 0, 1, 2, 5, 1, 0, 1], np.uint8)
    for mb, (y_mode, flags) in enumerate(((NEARMV, 0), (SPLITMV, 0), (B_PRED, 1))):
        mbs[mb, R.O_Y_MODE], mbs[mb, R.O_REF], mbs[mb, R.O_FLAGS] = y_mode, 0 if y_mode == B_PRED else 1, flags
        mbs[mb, R.O_EOBS:R.O_EOBS + 16] = eobs
        mbs[mb, R.O_EOBS + 24] = 4
    _, info = R.side(hdr, mbs, mvs, planes=("skip", "coded"))
    skip, coded = info
    # with a Y2 block a luma block starts at position 1: only eob > 1 counts; without: a lone DC is kind 1; skipped: nothing
    assert np.array_equal(coded[:, 0:4], np.where(eobs > 1, 2, 0).reshape(4, 4))
    assert np.array_equal(coded[:, 4:8], np.where(eobs > 1, 2, np.where(eobs == 1, 1, 0)).reshape(4, 4))
    assert (coded[:, 8:12] == 0).all()
    assert (skip[:, 0:8] == 0).all() and (skip[:, 8:12] == 1).all()
    # the C helper says the same (vp8ir_block_kind through the package's restatement)
    assert np.array_equal(R.block_kind(mbs), P.block_kinds(mbs)[:, :16])


def test_hand_built_segment_quantisers(pkg):
    P = pkg
    mbs, mvs = _blank(4)
    mbs[:, R.O_SEGMENT] = np.arange(4)
    for base, abs_delta, sq, want in ((60, 0, (-70, -5, 0, 80), (0, 55, 60, 127)), (60, 1, (0, 127, 5, 100), (0, 127, 5, 100)),
                                      (127, 0, (1, -127, 0, -128), (127, 0, 127, 0)), (0, 1, (-1, -128, 127, 64), (0, 0, 127, 64))):
        hdr = make_hdr(P, 64, 16, base_qindex=base, segmentation_enabled=1, mb_segment_abs_delta=abs_delta, segment_quant=sq)
        _, info = R.side(hdr, mbs, mvs, planes=("segment", "qindex"))
        assert info[0, 0, ::4].tolist() == [0, 1, 2, 3]
        assert info[1, 0, ::4].tolist() == list(want), (base, abs_delta, sq)
        off = make_hdr(P, 64, 16, base_qindex=base, segmentation_enabled=0, mb_segment_abs_delta=abs_delta, segment_quant=sq)
        assert (R.side(off, mbs, mvs, planes=("qindex",))[1] == base).all()


@pytest.mark.parametrize("name", STREAMS)
def test_fixtures_through_the_host_parser(pkg, name):
    P = pkg
    w, h, frames = P.read_ivf(ivf_path(name))
    parser = P.Parser()
    refs_seen, n_inter, n_split = set(), 0, 0
    rng = np.random.default_rng(11)
    try:
        for i, data in enumerate(frames):
            hdr, _, mbs, coef, mvs = P.parse_to_numpy(parser, data)
            parser.swap(hdr)
            mv, info = R.side(hdr, mbs, mvs, planes=63)
            gw, gh = 4 * hdr.mb_cols, 4 * hdr.mb_rows
            assert mv.shape == (2, gh, gw) and info.shape == (6, gh, gw)
            ref_mb = mbs[:, R.O_REF].reshape(hdr.mb_rows, hdr.mb_cols)
            assert np.array_equal(info[0], ref_mb.repeat(4, 0).repeat(4, 1))
            if hdr.frame_type == 0:
                assert (mv == 0).all() and (info[0] == 0).all(), (name, i)
                # ... whatever the vector array holds
                assert (R.side(hdr, mbs, rng.integers(-99, 99, mvs.shape).astype(np.int16))[0] == 0).all()
                continue
            n_inter += 1
            refs_seen |= set(np.unique(ref_mb).tolist())
            junk = mvs.copy()
            junk[mbs[:, R.O_REF] == 0] = rng.integers(-99, 99, (int((mbs[:, R.O_REF] == 0).sum()), 16, 2))
            assert np.array_equal(R.side(hdr, mbs, junk)[0], mv)                  # intra macroblocks: zero flow
            assert (mv[:, info[0] == 0] == 0).all()
            blocks = mv.reshape(2, hdr.mb_rows, 4, hdr.mb_cols, 4).transpose(1, 3, 0, 2, 4).reshape(-1, 2, 16)
            whole = mbs[:, R.O_Y_MODE] != SPLITMV
            assert (blocks[whole] == blocks[whole][:, :, :1]).all(), (name, i)     # one vector for all 16 cells
            n_split += int((~whole).sum())
            inter = mbs[:, R.O_REF] != 0
            assert np.array_equal(blocks[inter][:, 0], mvs[inter][:, :, 1]) and np.array_equal(blocks[inter][:, 1], mvs[inter][:, :, 0])
            assert np.array_equal(info[5].reshape(hdr.mb_rows, 4, hdr.mb_cols, 4).transpose(0, 2, 1, 3).reshape(-1, 16), P.block_kinds(mbs)[:, :16])
            # at the display size the tensors line up with the pixels
            mvd, infod = R.side(hdr, mbs, mvs, w, h, planes=63)
            assert np.array_equal(mvd, mv.repeat(4, 1).repeat(4, 2)[:, :h, :w]) and np.array_equal(infod, info.repeat(4, 1).repeat(4, 2)[:, :h, :w])
    finally:
        parser.close()
    assert n_inter > 0
    if name == "p_arf_176x144":
        assert {2, 3} <= refs_seen                        # golden and altref
    if name == "p_split_352x288":
        assert n_split > 0
