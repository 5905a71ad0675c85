"""CPU: the definition of the transform-and-quantise call (vp8hip_frames_quant_async, vp8hip_quant_factors; include/vp8hip.h) as
tests/quant_reference.py restates it -- pinned bit for bit to what the reference's own functions made of the cases of
tests/golden/quant_ref.json --, its known answers, the library's host table function and what the Python wrapper refuses with no
device."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import quant_reference as QR
import tfilter_reference as TR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_quant_fixtures import DELTA_SETS, FACTOR_ROWS, TENSORS, answers, case_inputs, unpacked  # noqa: E402

with open(os.path.join(HERE, "golden", "quant_ref.json")) as _f:
    FIXTURE = json.load(_f)
CASES = FIXTURE["cases"]


def case_id(c):
    return (f"{c['w']}x{c['h']}_{c['content']}_{c['vectors']}_q{c['qindex']}_{c['quantizer']}_{c['filter']}_" +
            "d" + ".".join(str(d) for d in c["deltas"]) + "_z" + ".".join(str(z) for z in c["zbin"]))


def run(c):
    src, ref, mv = case_inputs(c)
    return QR.quant_planes(src, ref, mv, c["qindex"], c["deltas"], c["quantizer"], c["filter"], c["zbin"])


def test_the_fixture_covers_what_it_should():
    assert {(c["w"], c["h"]) for c in CASES} == {(32, 32), (48, 32), (176, 144), (80, 48)}
    assert {tuple(c["display"]) for c in CASES if c["w"] == 80} == {(67, 45)}
    assert {0, 3, 40, 127} <= {c["qindex"] for c in CASES}
    assert any(c["deltas"] == [0, 1, 0, 0, 0] for c in CASES if c["qindex"] == 3)      # vp8_set_quantizer's 4 - Q, applied by the caller
    assert all(any(c["deltas"][k] for c in CASES) for k in range(5))
    assert {c["quantizer"] for c in CASES} == set(QR.QUANTIZERS) and {c["filter"] for c in CASES} == set(TR.FILTERS)
    assert {c["vectors"] for c in CASES} == set(TR.VECTORS) and {c["content"] for c in CASES} == set(QR.CONTENTS)
    zb = {tuple(c["zbin"]) for c in CASES}
    assert (0, 0, 0) in zb and all(any(z[k] and not z[(k + 1) % 3] and not z[(k + 2) % 3] for z in zb) for k in range(3))
    for size in ((32, 32), (48, 32), (176, 144)):                       # both quantisers and filters at every size; every kind of vector
        mine = [c for c in CASES if (c["w"], c["h"]) == size]            # recorded in full (32x32) and at more than one block row (176x144)
        assert {c["quantizer"] for c in mine} == set(QR.QUANTIZERS) and {c["filter"] for c in mine} == set(TR.FILTERS)
        assert {c["vectors"] for c in mine} == set(TR.VECTORS) or size == (48, 32)
        assert all(("levels" in c) == (size != (176, 144)) for c in mine)
    group = [c for c in CASES if c["group"] == "jobq"]
    assert len({c["qindex"] for c in group}) == len(group) == 4 and len({(c["w"], c["h"], tuple(c["deltas"]), c["quantizer"]) for c in group}) == 1
    assert [t["deltas"] for t in FIXTURE["factors"]] == [list(d) for d in DELTA_SETS]
    for c in CASES:                                                                     # no vector where the reference's short wraps
        mv = case_inputs(c)[2]
        assert mv is None or (int(mv.min()) > -32768 and int(mv.max()) < 32767)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_against_the_reference(case):
    """levels, dequantised levels, eobs, the five planes and the reconstruction of every macroblock"""
    o = run(case)
    got = answers(case, o["levels"], o["dequant"], o["eob"], QR.stats_tensor(o, 31), o["rec"])
    for name, dtype in TENSORS:
        if name in case:
            assert np.array_equal(got[name].ravel(), unpacked(case[name], dtype)), name
        else:
            assert hashlib.sha256(got[name].tobytes()).hexdigest() == case[name + "_sha256"], name
    assert not o["eob"][..., 25:].any()


def test_quant_factors_against_the_reference(pkg):
    """vp8hip_quant_factors and the restatement's table, for all 128 qindex values at three delta sets"""
    P = pkg
    L = P.load_hip()
    assert ctypes.sizeof(P.QuantTable) == 168
    for t in FIXTURE["factors"]:
        mine, lib = np.zeros((128, 84), "<i2"), np.zeros((128, 84), "<i2")
        for q in range(128):
            mine[q] = QR.factors_flat(q, t["deltas"])
            got = P.quant_factors(q, t["deltas"])
            lib[q] = np.concatenate([got[k].ravel() for k in QR.FIELDS] + [got["zrun_zbin_boost"].ravel()])
        for q in FACTOR_ROWS:
            assert mine[q].tolist() == t["rows"][str(q)] == lib[q].tolist(), (t["deltas"], q)
        assert np.array_equal(mine, lib), np.argwhere(mine != lib)[:4].tolist()
        assert hashlib.sha256(mine.tobytes()).hexdigest() == t["sha256"] == hashlib.sha256(lib.tobytes()).hexdigest(), t["deltas"]
    out = P.QuantTable()
    zero = (ctypes.c_int * 5)()
    assert L.vp8hip_quant_factors(40, None, ctypes.byref(out)) == 0                     # NULL deltas: all 0
    assert np.array_equal(np.ctypeslib.as_array(out.dequant), QR.quant_factors(40)["dequant"])
    assert L.vp8hip_quant_factors(40, zero, None) == -2
    for q in (-1, 128, 1 << 20):
        assert L.vp8hip_quant_factors(q, zero, ctypes.byref(out)) == -2
    for k in range(5):
        for v in (-16, 16):
            d = (ctypes.c_int * 5)()
            d[k] = v
            assert L.vp8hip_quant_factors(40, d, ctypes.byref(out)) == -2
            with pytest.raises(ValueError):
                P.quant_factors(40, list(d))


def flat(y, c, w=32, h=32):
    return [np.full((h, w), y, np.uint8), np.full((h // 2, w // 2), c, np.uint8), np.full((h // 2, w // 2), c, np.uint8)]


def test_known_answers():
    w, h = 48, 32
    noise, smooth = TR.picture("noise", w, h, 4), TR.picture("smooth", w, h, 5)
    # a picture against itself: all levels 0, all eobs 0, rec = the prediction = the picture; EOBS, ERRY2 and RECSSE 0.  ERRY and ERRUV
    # are NOT 0, in the reference either: vp8_short_fdct4x4_c of a zero block is not zero -- its first pass leaves 14500 >> 12 = 3 in
    # column 1 of every row, and (3 + 3 + 3 + 3 + 7) >> 4 = 1 is the block's position 1 --, so a macroblock has 16 and 8
    assert np.array_equal(QR.fdct(np.zeros((4, 4), np.int64)).ravel(), [0, 1] + [0] * 14)
    for pic in (noise, smooth):
        for quantizer in QR.QUANTIZERS:
            for q in (0, 127):
                o = QR.quant_planes(pic, pic, None, q, quantizer=quantizer)
                assert not o["levels"].any() and not o["dequant"].any() and not o["eob"].any()
                assert all(np.array_equal(r, p) and np.array_equal(r, s) for r, p, s in zip(o["rec"], o["pred"], pic))
                st = o["stats"]
                assert not st["eobs"].any() and not st["erry2"].any() and not st["recsse"].any()
                assert (st["erry"] == 16).all() and (st["erruv"] == 8).all()
    # luma flat 8 above the reference, chroma equal: every luma block's coefficient 0 is 64 (and position 1 the zero block's 1), the Y2
    # DC 512.  From qindex 104 the y1dc zero bin ((80 * 104 + 64) >> 7 = 65) is above 64, so every luma eob is 0 and only the Y2 DC
    # survives, level 2; from 112 to 118 its dequantised value 2 * y2dc is 488 .. 536, the _1 inverse Walsh gives (dq + 3) >> 3 =
    # 61 .. 67 a block, eob_adjust keeps the luma blocks in the transform, and (61 .. 67 + 4) >> 3 = 8: rec == source
    src, ref = flat(98, 90), flat(90, 90)
    survivors = []
    for q in range(128):
        o = QR.quant_planes(src, ref, None, q)
        if not o["eob"][..., :24].any() and (o["eob"][..., 24] == 1).all():
            survivors.append(q)
            assert all(np.array_equal(r, s) for r, s in zip(o["rec"], src)) == (112 <= q <= 118), q
    assert survivors == list(range(104, 128))
    o = QR.quant_planes(src, ref, None, 112)
    assert (o["coef"][..., :16, 0] == 64).all() and not o["coef"][..., :24, 2:].any() and (o["coef"][..., 24, 0] == 512).all()
    assert (o["levels"][..., 24, 0] == 2).all() and (o["dequant"][..., 24, 0] == 488).all() and not o["levels"][..., :24, :].any()
    assert (o["stats"]["eobs"] == 1).all() and (o["stats"]["recsse"] == 0).all() and (o["stats"]["erry"] == 16).all()
    assert (o["stats"]["erry2"] == (512 - 488) ** 2).all()
    assert any(c["content"] == "flatluma" and c["qindex"] == 112 for c in CASES)       # the reference itself shows exactly that
    # eob[24] > 1: a step between the left and the right half of a macroblock puts energy into the Y2 block's first row
    step = flat(90, 90)
    step[0][:, 8:16] = 130
    o = QR.quant_planes(step, ref, None, 40)
    assert (o["eob"][0, 0, 24] > 1) and o["levels"][0, 0, 24, 1] != 0 and o["eob"][0, 1, 24] == 0
    # the vector components 32767 and -32768: no wrap in the chroma vector (the reference's short would give -16384 and 16383)
    assert QR.chroma_mv(32767) == 16384 and QR.chroma_mv(-32768) == -16384
    mv = np.zeros((2, 2, 3), np.int64)
    mv[0], mv[1] = 32767, -32768
    o = QR.quant_planes(smooth, smooth, mv, 40)
    want = [np.broadcast_to(p[0:1, -1:], p.shape) for p in smooth]                      # far right of and above the picture: its top right pixel
    assert all(np.array_equal(p, q) for p, q in zip(o["pred"], want))
    # the chroma vector for luma vectors -3 .. 3: (c + sign) / 2 towards zero
    assert [QR.chroma_mv(c) for c in (-3, -2, -1, 0, 1, 2, 3)] == [-2, -1, -1, 0, 1, 1, 2]
    ramp = [np.tile(np.arange(w, dtype=np.uint8) * 4, (h, 1)), np.tile(np.arange(w // 2, dtype=np.uint8) * 8, (h // 2, 1)),
            np.tile(np.arange(w // 2, dtype=np.uint8) * 8, (h // 2, 1))]
    for c, shift in ((-3, -2), (-2, -1), (-1, -1), (1, 1), (2, 1), (3, 2)):             # 1/8 of a chroma pixel on a ramp of 8 a pixel
        p = QR.predict_mb(ramp, 1, 1, c, 0, "bilinear")
        assert (p[1] == ramp[1][8:16, 8:16].astype(np.int64) + shift).all() and np.array_equal(p[1], p[2]), c
    # FAST quantises below the REGULAR zero bin.  At qindex 40 the Y1 ac factors are dequant 44, zbin 29, round 16, quant_fast 1489,
    # quant -17873 >> 5, the boosts 0 0 2 3 4 4 5 6 8 9 11 12 13 15 15 15.  Block 0: 28 at position 1 is below both ((28 + 16) * 1489
    # >> 16 = 0) and 40 at position 15, the last step, is below 29 + 15 but (40 + 16) * 1489 >> 16 = 1.  Block 1: 100 at position 1
    # (step 1) gives ((116 * -17873 >> 16) + 116) >> 5 = 2 and resets the run, so -30 at position 4 (step 2) meets the bare bin: -1.
    # Block 2: the same 30 alone at step 2 has run 2 against it, 29 + 2: nothing -- but (30 + 16) * 1489 >> 16 = 1 in the fast form
    f = QR.quant_factors(40)
    assert [int(f[k][QR.Y1][1]) for k in ("dequant", "zbin", "round", "quant_fast", "quant", "quant_shift")] == [44, 29, 16, 1489, -17873, 5]
    assert f["zrun_zbin_boost"][QR.Y1].tolist() == [0, 0, 2, 3, 4, 4, 5, 6, 8, 9, 11, 12, 13, 15, 15, 15]
    co = np.zeros((1, 25, 16), np.int64)
    co[0, 0, 15], co[0, 0, 1], co[0, 1, 1], co[0, 1, 4], co[0, 2, 4] = 40, 28, 100, -30, 30
    q, dq, e = QR.quantise(co, f, [0, 0, 0], "regular")
    assert not q[0, 0].any() and q[0, 1].tolist() == [0, 2, 0, 0, -1] + [0] * 11 and not q[0, 2].any() and e[0, :3].tolist() == [0, 3, 0]
    assert dq[0, 1].tolist() == [0, 88, 0, 0, -44] + [0] * 11
    q, dq, e = QR.quantise(co, f, [0, 0, 0], "fast")
    assert q[0, 0].tolist() == [0] * 15 + [1] and q[0, 1].tolist() == [0, 2, 0, 0, -1] + [0] * 11 and q[0, 2].tolist() == [0] * 4 + [1] + [0] * 11
    assert e[0, :3].tolist() == [16, 3, 3] and dq[0, 0, 15] == 44
    # a zbin_over_quant large enough to zero a block that is otherwise coded; the Y2 form halves it.  Flat 97 over flat 90 at qindex
    # 40: coefficient 0 is 56 in all 24 blocks (level 1) and 448 in the Y2 block (level 6); zbin_over_quant 200 gives the extras
    # 44 * 200 >> 7 = 68 (Y1, UV) and 68 * 100 >> 7 = 53 (Y2): 56 < 24 + 68, 448 >= 49 + 53; 2000 (687, 531) zeroes the Y2 block too
    src4 = flat(97, 97)
    coded = QR.quant_planes(src4, ref, None, 40)
    assert (coded["eob"][..., :25] == 1).all() and (coded["coef"][..., :24, 0] == 56).all() and (coded["coef"][..., 24, 0] == 448).all()
    assert (coded["levels"][..., :24, 0] == 1).all() and (coded["levels"][..., 24, 0] == 6).all()
    assert QR.zbin_extra(f, 200, 0, 0).tolist() == [68, 53, 68] and QR.zbin_extra(f, 2000, 0, 0).tolist() == [687, 531, 687]
    zeroed = QR.quant_planes(src4, ref, None, 40, zbin=(200, 0, 0))
    assert not zeroed["eob"][..., :24].any() and (zeroed["eob"][..., 24] == 1).all()
    assert not QR.quant_planes(src4, ref, None, 40, zbin=(2000, 0, 0))["eob"].any()
    assert np.array_equal(QR.quant_planes(src4, ref, None, 40, quantizer="fast", zbin=(2000, 9, 9))["levels"],
                          QR.quant_planes(src4, ref, None, 40, quantizer="fast")["levels"])              # the fast form has no zero bin
    assert QR.zbin_extra(f, 0, 200, 0).tolist() == [68, 106, 68] == QR.zbin_extra(f, 0, 0, 200).tolist()  # only zbin_over_quant is halved
    assert int(QR.zbin_extra(f, -3, 0, 0)[1]) == (68 * -1) >> 7                           # -3 / 2 is -1 in C
    top = 1 << 20
    assert int(QR.zbin_extra(QR.quant_factors(127), top, top, top)[0]) == int(QR.s16((284 * 3 * top) >> 7))   # the (short) truncates
    # the crop of rec from the coded 80x48 to 67x45 keeps the right pixels
    big = TR.picture("smooth", 80, 48, 7)
    o = QR.quant_planes(big, TR.picture("noise", 80, 48, 8), None, 40)
    packed = TR.pack(o["rec"], 67, 45)
    assert packed.size == 67 * 45 + 2 * 34 * 23 and np.array_equal(packed[:67 * 45].reshape(45, 67), o["rec"][0][:45, :67])
    assert np.array_equal(packed[67 * 45 + 34 * 23:].reshape(23, 34), o["rec"][2][:23, :34])


def test_every_int16_store_fits_on_the_worst_pictures():
    """all 0 against all 255 and the reverse, at both ends of the quantiser: quant_reference.fit asserts at every int16 store;
    coefficients stay within +-2040, the Y2 block within +-16320, and with alternating blocks the Walsh intermediates within +-32641"""
    lo, hi = flat(0, 0), flat(255, 255)
    for src, ref in ((lo, hi), (hi, lo)):
        for q in (0, 40, 127):
            for quantizer in QR.QUANTIZERS:
                o = QR.quant_planes(src, ref, None, q, quantizer=quantizer)
                assert int(np.abs(o["coef"][..., :24, :]).max()) == 2040 and 16319 <= int(np.abs(o["coef"][..., 24, :]).max()) <= 16320
                assert int(np.abs(o["dequant"]).max()) <= 16320 + 157                     # within half a step of the coefficient
    chk = flat(0, 0)
    chk[0][:, 4:8] = chk[0][:, 12:16] = chk[0][:, 20:24] = chk[0][:, 28:32] = 255           # blocks alternate: +2040, -2040 along a row of DCs
    for src, ref in ((chk, [255 - p for p in chk]), ([255 - p for p in chk], chk)):
        for q in (0, 127):
            o = QR.quant_planes(src, ref, None, q)
            assert int(np.abs(o["coef"][..., 24, :]).max()) <= 16320
    t = QR.walsh(np.tile(np.array([2040, 2040, 2040, 2040]), (4, 1)))                     # the first pass's largest: 8 * 2040 * 2 + 1
    assert int(np.abs(t).max()) == 16320 and (2040 * 16 + 1) == 32641


def test_sizes_structs_and_what_the_wrapper_refuses(pkg):
    P = pkg
    assert P.quant_sizes(176, 144, ("erry", "eobs")) == (79200, 3168, 792, 38016) and P.quant_sizes(67, 45) == (12000, 480, 0, 67 * 45 + 2 * 34 * 23)
    assert P.quant_sizes(0, 16) == (0, 0, 0, 0) and P.quant_sizes(16, 16384) == (0, 0, 0, 0)
    names = [f[0] for f in P.QuantParams._fields_]
    assert names == ["qindex", "delta", "quantizer", "filter", "stage", "zbin_over_quant", "zbin_mode_boost", "act_zbin_adj", "planes", "job_qindex"]
    assert ctypes.sizeof(P.QuantParams) == 64 and P.QuantParams.job_qindex.offset == 56
    assert P.QUANT_QUANTIZERS == {"regular": 0, "fast": 1} and P.QUANT_PLANES == QR.STATS and P.QUANT_ZBIN_MAX == QR.ZBIN_TERM_MAX
    L = P.load_hip()
    assert L.vp8hip_quant_coef_size(None) == 0 and L.vp8hip_quant_eob_size(None) == 0 and L.vp8hip_quant_stats_size(None, None) == 0
    ctx = P.Vp8Hip.__new__(P.Vp8Hip)                 # no device, no context: only what the wrapper sees before the call
    for kw in (dict(jobs=[]), dict(jobs=[0]), dict(jobs=[(0, 1, 2)]), dict(jobs=[(0, -1)]), dict(jobs=[(-1, 0)]), dict(qindex=-1), dict(qindex=128),
               dict(qindex=[40, 40]), dict(qindex=[128]), dict(deltas=(0, 0, 0, 0)), dict(deltas=(16, 0, 0, 0, 0)), dict(deltas=(0, 0, 0, 0, -16)),
               dict(quantizer="exact"), dict(filter="bicubic"), dict(stage="tokens"), dict(zbin=(0, 0)), dict(zbin=((1 << 20) + 1, 0, 0)),
               dict(zbin=(0, 0, -(1 << 20) - 1)), dict(planes=("psnr",)), dict(planes=32), dict(want=("tokens",)), dict(want=()),
               dict(want=("stats",))):
        with pytest.raises(ValueError):
            ctx.frames_quant(**dict(dict(jobs=[(0, 1)]), **kw))


def test_header_declares_the_calls():
    """(tests/test_abi_cpu.py then checks that the library exports what the header declares)"""
    with open(os.path.join(HERE, "..", "include", "vp8hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("vp8hip_quant_factors", "vp8hip_quant_coef_size", "vp8hip_quant_eob_size", "vp8hip_quant_stats_size", "vp8hip_frames_quant_async"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
    for name, value in (("REGULAR", 0), ("FAST", 1), ("ERRY", 1), ("ERRY2", 2), ("ERRUV", 4), ("EOBS", 8), ("RECSSE", 16)):
        assert re.search(r"#define\s+VP8HIP_QUANT_%s\s+%d\b" % (name, value), src), name
    assert re.search(r"typedef struct vp8hip_quant\s*{\s*int qindex;\s*int delta\[5\];\s*int quantizer;\s*int filter;\s*int stage;\s*"
                     r"int zbin_over_quant, zbin_mode_boost, act_zbin_adj;\s*unsigned planes;\s*const uint8_t \*job_qindex;\s*}", src)
