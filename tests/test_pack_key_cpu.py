"""CPU: the host side of the key-frame packer (vp8hip_pack_key_header, vp8hip_pack_key_bound's formula; include/vp8hip.h) against
the bool encoder of tests/vp8_writer.py, what is refused, and the restatement the GPU test compares with
(tests/pack_key_reference.py): its frames are decoded by the REAL reference decoder -- oracle/_ref/ref_md5 where the reference is
built, else its listing recorded for the same stream bytes in tests/golden/pack_key_ref_md5.json (VP8_RECORD_REF_DIGESTS=1 with
the reference built rewrites it) -- to the frames the oracle produces."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import intra_reference as IR
import pack_key_reference as K
from vp8_testlib import GOLDEN, ROOT, oracle_decode
from vp8_writer import write_ivf

REF_MD5 = os.path.join(ROOT, "oracle", "_ref", "ref_md5")
LISTINGS = os.path.join(GOLDEN, "pack_key_ref_md5.json")
RECORD = os.environ.get("VP8_RECORD_REF_DIGESTS") == "1"

EXTREMES = dict(version=(0, 3), show_frame=(0, 1), color_space=(0, 1), clamping_type=(0, 1), filter_type=(0, 1), filter_level=(0, 63),
                sharpness=(0, 7), log2_parts=(0, 3), prob_skip_false=(1, 255))
HEADER_CASES = [dict(qindex=q) for q in (0, 40, 127)] + \
    [dict(deltas=tuple((-1) ** k * (3 + 3 * k) if i == k else 0 for i in range(5))) for k in range(5)] + \
    [{name: v} for name, ends in EXTREMES.items() for v in ends] + \
    [dict(qindex=127, deltas=(15, -15, 15, -15, 15), **{name: ends[1] for name, ends in EXTREMES.items()}),
     dict(qindex=0, deltas=(-15, 15, -15, 15, -15), **{name: ends[0] for name, ends in EXTREMES.items()})]


@pytest.mark.parametrize("case", HEADER_CASES, ids=lambda c: "_".join(f"{k}{v}" for k, v in c.items()).replace(" ", ""))
def test_header_is_the_bool_encoders(pkg, case):
    """bytes and state of vp8hip_pack_key_header equal a BoolEncoder driven through the same fields; the carry form describes the
    same; it fits VP8HIP_PACK_HEAD_MAX at both extremes of every field"""
    got = pkg.pack_key_header(**case)
    e = K.header_encoder(**case)
    assert got["bytes"] == bytes(e.out) and (got["bottom"], got["range"], got["bit_count"]) == (e.bottom, e.range, e.bit_count)
    b = got["bytes"]
    assert got["settled"] + 1 + got["pending"] == len(b) and b[got["settled"]] == got["cache"] != 255
    assert b[got["settled"] + 1:] == b"\xff" * got["pending"] and len(b) <= 64


def test_the_header_follows_every_field(pkg):
    """no field is ignored: each changes the bytes or the state (version and show_frame are the tag's)"""
    base = pkg.pack_key_header()
    for name, v in dict(version=1, show_frame=0).items():
        assert pkg.pack_key_header(**{name: v}) == base, name
    for name, v in dict(color_space=1, clamping_type=1, filter_type=1, filter_level=9, sharpness=2, log2_parts=1, prob_skip_false=7).items():
        assert pkg.pack_key_header(**{name: v}) != base, name
    assert pkg.pack_key_header(41) != base and pkg.pack_key_header(deltas=(0, 0, 0, 0, 1)) != base


@pytest.mark.parametrize("bad", [dict(qindex=-1), dict(qindex=128), dict(deltas=(16, 0, 0, 0, 0)), dict(deltas=(0, 0, 0, 0, -16)), dict(deltas=(0, 0, 0)),
                                 dict(version=4), dict(version=-1), dict(show_frame=2), dict(color_space=2), dict(color_space=-1), dict(clamping_type=2),
                                 dict(filter_type=2), dict(filter_level=64), dict(filter_level=-1), dict(sharpness=8), dict(log2_parts=4),
                                 dict(log2_parts=-1), dict(prob_skip_false=0), dict(prob_skip_false=256), dict(ref_frame=1), dict(no_such_field=1)], ids=str)
def test_out_of_range_parameters_are_refused(pkg, bad):
    with pytest.raises(ValueError):
        pkg.pack_key_header(**bad)


def test_the_bound_holds_on_the_worst_macroblock(pkg):
    """B_PRED, the longest path of the sub-block tree sixteen times, 24 blocks of sixteen levels of +-2114: within the bound; the
    formula; 0 for what has no bound"""
    modes = np.zeros((1, 1, 32), np.uint8)
    modes[0, 0, 0], modes[0, 0, 1], modes[0, 0, 4:20] = K.B_PRED, 3, 9
    worst = np.full((1, 1, 25, 16), K.MAX_LEVEL, np.int16) * np.where(np.arange(16) & 1, -1, 1).astype(np.int16)
    r = K.restate(modes, worst, prob_skip_false=255)
    assert r["status"] == 0 and r["info"][12] == 1 and r["info"][11] == 0
    assert pkg.pack_key_bound(16, 16, 0) >= len(r["data"]) > 1500
    assert pkg.pack_key_bound(16, 16) == (10 + 64 + 8 + 103 + 6672 + 4 + 15) // 16 * 16
    for lp in (0, 3):
        lv = K.make_levels("dense", 9, 11, 0)
        bound = pkg.pack_key_bound(176, 144, lp)
        assert bound % 16 == 0 and bound >= K.restate(K.make_modes("bpred", 9, 11, 0), lv, log2_parts=lp)["info"][1] > 30000
    assert pkg.pack_key_bound(0, 16) == pkg.pack_key_bound(16, 16384) == pkg.pack_key_bound(16, 16, 4) == pkg.pack_key_bound(16, 16, -1) == 0


def test_the_restatement_flags_what_the_call_refuses():
    modes, lv = K.make_modes("mixed", 2, 3, 5), K.make_levels("sparse", 2, 3, 5)
    modes[0, 0, 0], modes[1, 2, 0] = K.B_PRED, 2
    good = K.restate(modes, lv)
    assert good["status"] == 0 and good["info"][12] >= 1
    for at, v in (((0, 0, 0), 5), ((1, 1, 1), 4), ((0, 0, 9), 10)):
        bad = modes.copy(); bad[at] = v
        r = K.restate(bad, lv)
        assert r["status"] == K.BAD_MODE and r["data"] is None and r["info"][1] == 0
    free = modes.copy(); free[1, 2, 4:20] = 255; free[..., 2:4] = 255; free[..., 20:] = 255       # what is not read
    assert K.restate(free, lv)["data"] == good["data"]
    big = lv.copy(); big[0, 0, 3, 0] = 2115                              # luma position 0 of a B_PRED macroblock is coded
    assert K.restate(modes, big)["status"] == K.BAD_LEVEL
    big = lv.copy(); big[1, 2, 3, 0] = 2115; big[0, 0, 24, 7] = -2115    # ... of a 16x16 one is not, nor block 24 of a B_PRED one
    assert K.restate(modes, big)["data"] == good["data"]
    n = len(good["data"])
    assert K.restate(modes, lv, cap=n)["status"] == 0 and K.restate(modes, lv, cap=n - 1)["status"] == K.OVERFLOW
    hidden = K.restate(modes, lv, show_frame=0)["data"]
    assert hidden[0] == good["data"][0] & 0xef and hidden[1:] == good["data"][1:] and good["data"][0] & 0x11 == 0x10


def reference_listing(key, ivf):
    """test_pack_cpu.py's: the reference decoder's per-frame MD5s of the stream in `ivf`, live where it is built, else as recorded"""
    sha = hashlib.sha256(open(ivf, "rb").read()).hexdigest()
    table = json.load(open(LISTINGS)) if os.path.exists(LISTINGS) else {}
    live = None
    if os.path.exists(REF_MD5):
        out = str(ivf) + ".md5"
        r = subprocess.run([REF_MD5, str(ivf), out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        live = [l.split()[0] for l in open(out)]
    if RECORD:
        assert live is not None, "VP8_RECORD_REF_DIGESTS=1 needs the reference build (make -C oracle ref)"
        table[key] = {"stream_sha256": sha, "md5": live}
        with open(LISTINGS, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    rec = table.get(key)
    assert rec is not None, f"{key}: no reference listing recorded in {LISTINGS}"
    assert rec["stream_sha256"] == sha, f"{key}: the written stream is not the one the reference listing was recorded from"
    if live is not None:
        assert live == rec["md5"], key
    return rec["md5"]


def decoded_like_the_reference(pkg, name, r, display, tmp_path):
    """the restated frame as a one-frame stream: the real reference decoder's frame is the oracle's from the IR the feeder reads
    back, and that IR is the one the frame was written from.  -> the frame's MD5"""
    w, h = display
    ivf = tmp_path / f"{name}.ivf"
    write_ivf(ivf, w, h, [r["data"]])
    ref = reference_listing(name, ivf)
    g = pkg.geom(w, h)
    bufs = [np.zeros(g.frame_size, np.uint8) for _ in range(4)]
    parser = pkg.Parser()
    try:
        hdr, _, mbs, coef, mvs = pkg.parse_to_numpy(parser, r["data"])
        f = parser.refs
        new, lst, gld, alt = f.new_idx, f.lst_idx, f.gld_idx, f.alt_idx
        parser.swap(hdr)
        oracle_decode(hdr, mbs, coef, mvs, bufs[new], (bufs[lst], bufs[gld], bufs[alt]))
        mine = [pkg.frame_md5(bufs[parser.refs.show_idx], g, w, h)]
        live = (r["mbs"][:, 3] & 1) == 0
        assert np.array_equal(coef[live], r["coef"][live])
    finally:
        parser.close()
    assert mine == ref
    return mine[0]


def test_intra_planes_frame_decodes_like_the_oracle(pkg, tmp_path):
    """(a) 48x32: the modes and levels of the intra restatement on the decoded picture with all ten sub-block modes tried"""
    costs = pkg.intra_costs()
    rdm, rdd = IR.intra_rd(40)
    o = IR.intra_planes(IR.picture("decoded", 48, 32, 61), 40, rdmult=rdm, rddiv=rdd, mbmode_cost=costs[0], bmode_cost=costs[1], bmode_last=9)
    assert (o["modes"][..., 0] == K.B_PRED).any() and o["seen"]["bmodes"] - set(range(4))
    r = K.restate(o["modes"], o["levels"], qindex=40)
    assert r["status"] == 0 and np.array_equal(r["mbs"][:, 3], o["modes"].reshape(-1, 32)[:, 2])     # the skip rule is frames_intra's
    decoded_like_the_reference(pkg, "48x32_intra_planes", r, (48, 32), tmp_path)


COVER_SEED = 0                          # (the first seed at which the draw meets all 100 pairs)


def test_every_mode_and_every_context_pair_decodes_like_the_oracle(pkg, tmp_path):
    """(b) 64x64 whose modes are drawn so that all five y modes, four uv modes, ten sub-block modes and 100 (A, L) pairs occur"""
    modes = K.make_cover_modes(4, 4, COVER_SEED)
    ys, uvs, subs, pairs = K.coverage(modes)
    assert ys == set(range(5)) and uvs == set(range(4)) and subs == set(range(10)) and len(pairs) == 100
    r = K.restate(modes, K.make_levels("sparse", 4, 4, COVER_SEED), qindex=20, filter_level=20, sharpness=3)
    assert r["status"] == 0 and 0 < r["info"][11] < 16
    decoded_like_the_reference(pkg, "64x64_every_mode_and_pair", r, (64, 64), tmp_path)


@pytest.mark.parametrize("column", (True, False), ids=("column", "row"))
def test_the_y2_context_skips_b_pred_macroblocks(pkg, tmp_path, column):
    """(c) a Y2 macroblock, two B_PRED ones (one skipped), a Y2 macroblock: the last one's Y2 context is the first one's, so the
    frames with and without a coded Y2 level in the first differ, and both decode as the reference decodes them"""
    frames = []
    for has in (True, False):
        modes, lv = K.y2_context_case(has, column)
        r = K.restate(modes, lv, qindex=30)
        assert r["status"] == 0 and r["info"][12] == 2 and r["info"][11] == 13
        decoded_like_the_reference(pkg, f"y2_context_{'column' if column else 'row'}_{int(has)}", r, (64, 64), tmp_path)
        frames.append(r["data"])
    assert frames[0] != frames[1]


def test_display_size_and_8_partitions_decode_like_the_oracle(pkg, tmp_path):
    """(d) 80x48 shown as 67x45 with 8 partitions"""
    r = K.restate(K.make_modes("mixed", 3, 5, 9), K.make_levels("sparse", 3, 5, 9), qindex=60, display=(67, 45), log2_parts=3, filter_level=8,
                  deltas=(2, -3, 4, -5, 6))
    assert r["status"] == 0 and all(r["info"][3:11]) and r["data"][6:10] == bytes([67, 0, 45, 0])
    decoded_like_the_reference(pkg, "80x48_shown_67x45_8_partitions", r, (67, 45), tmp_path)
