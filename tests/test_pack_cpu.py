"""CPU: the host side of the frame packer (vp8hip_pack_header, vp8hip_pack_bound's formula; include/vp8hip.h) against the bool
encoder of tests/vp8_writer.py, what is refused, and the restatement the GPU test compares with (tests/pack_reference.py): its
frames are decoded by the REAL reference decoder -- oracle/_ref/ref_md5 where the reference is built, else its listing recorded
for the same stream bytes in tests/golden/pack_ref_md5.json (VP8_RECORD_REF_DIGESTS=1 with the reference built rewrites it) -- to
the frames the oracle produces."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import pack_reference as R
from vp8_testlib import GOLDEN, ROOT, oracle_decode, synth_ir
from vp8_writer import write_ivf, write_key_frame

REF_MD5 = os.path.join(ROOT, "oracle", "_ref", "ref_md5")
LISTINGS = os.path.join(GOLDEN, "pack_ref_md5.json")
RECORD = os.environ.get("VP8_RECORD_REF_DIGESTS") == "1"

HEADER_CASES = [dict(qindex=q) for q in (0, 40, 127)] + \
    [dict(deltas=tuple((-1) ** k * (3 + 3 * k) if i == k else 0 for i in range(5))) for k in range(5)] + \
    [dict(ref_frame=r) for r in (1, 2, 3)] + \
    [{name: v} for name in ("prob_skip_false", "prob_intra", "prob_last", "prob_gf") for v in (1, 255)] + \
    [dict(version=3, show_frame=0, filter_type=1, filter_level=63, sharpness=7, log2_parts=3, qindex=127, deltas=(15, -15, 15, -15, 15)),
     dict(refresh_golden=1, refresh_alt=1, copy_buffer_to_gf=2, copy_buffer_to_arf=1, sign_bias_golden=1, sign_bias_alt=1, refresh_last=0),
     dict(refresh_golden=0, refresh_alt=0, copy_buffer_to_gf=2, copy_buffer_to_arf=1, sign_bias_alt=1, log2_parts=2)]


@pytest.mark.parametrize("case", HEADER_CASES, ids=lambda c: "_".join(f"{k}{v}" for k, v in c.items()).replace(" ", ""))
def test_header_is_the_bool_encoders(pkg, case):
    """bytes and state of vp8hip_pack_header equal a BoolEncoder driven through the same fields; the carry form describes the same"""
    got = pkg.pack_header(**case)
    e = R.header_encoder(**case)
    assert got["bytes"] == bytes(e.out) and (got["bottom"], got["range"], got["bit_count"]) == (e.bottom, e.range, e.bit_count)
    b = got["bytes"]
    assert got["settled"] + 1 + got["pending"] == len(b) and b[got["settled"]] == got["cache"] != 255
    assert b[got["settled"] + 1:] == b"\xff" * got["pending"] and len(b) <= 64


def test_the_header_follows_every_field(pkg):
    """no field is ignored: each changes the bytes or the state (ref_frame is per macroblock: not in the header)"""
    base = pkg.pack_header()
    for name, v in dict(version=1, show_frame=0, ref_frame=2).items():
        assert pkg.pack_header(**{name: v}) == base, name         # (the tag's, the macroblocks')
    for name, v in dict(filter_type=1, filter_level=9, sharpness=2, refresh_last=0, refresh_golden=1, refresh_alt=1, copy_buffer_to_gf=1,
                        copy_buffer_to_arf=2, sign_bias_golden=1, sign_bias_alt=1, log2_parts=1, prob_skip_false=7, prob_intra=9, prob_last=11,
                        prob_gf=13).items():
        assert pkg.pack_header(**{name: v}) != base, name
    assert pkg.pack_header(41) != base and pkg.pack_header(deltas=(0, 0, 0, 0, 1)) != base


@pytest.mark.parametrize("bad", [dict(qindex=-1), dict(qindex=128), dict(deltas=(16, 0, 0, 0, 0)), dict(deltas=(0, 0, 0, 0, -16)), dict(deltas=(0, 0, 0)),
                                 dict(version=4), dict(version=-1), dict(show_frame=2), dict(filter_type=2), dict(filter_level=64), dict(sharpness=8),
                                 dict(ref_frame=0), dict(ref_frame=4), dict(refresh_last=2), dict(refresh_golden=-1), dict(refresh_alt=2),
                                 dict(copy_buffer_to_gf=3), dict(copy_buffer_to_arf=-1), dict(sign_bias_golden=2), dict(sign_bias_alt=2),
                                 dict(log2_parts=4), dict(log2_parts=-1), dict(prob_skip_false=0), dict(prob_intra=0), dict(prob_last=256),
                                 dict(prob_gf=0), dict(no_such_field=1)], ids=str)
def test_out_of_range_parameters_are_refused(pkg, bad):
    with pytest.raises(ValueError):
        pkg.pack_header(**bad)


def test_the_bound_holds_on_the_dense_case(pkg):
    """a multiple of 16, not below the restatement's frame of the dense case with 1 and with 8 partitions, 0 for what has no bound"""
    mv, lv = R.make_field("alphabet", 9, 11, 0), R.make_levels("dense", 9, 11, 0)
    for lp in (0, 3):
        bound = pkg.pack_bound(176, 144, lp)
        assert bound % 16 == 0 and bound >= R.restate(mv, lv, log2_parts=lp)["info"][1] > 30000
    # the worst the token tree has: every level at the end of DCT_CAT6, signs mixed
    worst = np.full((1, 1, 25, 16), R.MAX_LEVEL, np.int16) * np.where(np.arange(16) & 1, -1, 1).astype(np.int16)
    assert pkg.pack_bound(16, 16, 0) >= len(R.restate(None, worst)["data"]) > 1500
    assert pkg.pack_bound(16, 16) == (3 + 64 + 8 + 28 + 6672 + 4 + 15) // 16 * 16
    assert pkg.pack_bound(0, 16) == pkg.pack_bound(16, 16384) == pkg.pack_bound(16, 16, 4) == pkg.pack_bound(16, 16, -1) == 0


def test_the_restatement_flags_what_the_call_refuses():
    lv = R.make_levels("sparse", 2, 3, 5)
    mv = R.make_field("alphabet", 2, 3, 5)
    assert R.restate(mv, lv)["status"] & 7 == 0
    odd = mv.copy(); odd[0, 1, 1] += 1
    assert R.restate(odd, lv)["status"] & 7 == R.BAD_VECTOR and R.restate(odd, lv)["data"] is None
    wide = np.zeros_like(mv); wide[0, 0, 0] = 2048                       # a difference of 1024 coded units from (0, 0)
    assert R.restate(wide, lv)["status"] & R.BAD_VECTOR
    wide[0, 0, 0] = 2046
    assert R.restate(wide, lv)["status"] == R.CLAMPS                     # 1023: in range, but far beyond the border
    big = lv.copy(); big[1, 2, 17, 5] = 2115
    assert R.restate(mv, big)["status"] & 7 == R.BAD_LEVEL
    big[1, 2, 17, 5] = 0; big[1, 2, 3, 0] = -2115                        # luma position 0 is not coded
    assert R.restate(mv, big)["data"] == R.restate(mv, lv)["data"]
    n = len(R.restate(mv, lv)["data"])
    assert R.restate(mv, lv, cap=n)["status"] & 7 == 0 and R.restate(mv, lv, cap=n - 1)["status"] & 7 == R.OVERFLOW


def test_the_carry_cases_have_their_carries():
    """the seeds the GPU test relies on (found by search on the CPU) and the frame made to carry through 0xFF bytes"""
    first = R.restate(R.make_field("far", 9, 11, 897), R.make_levels("zero", 9, 11, 897))
    assert first["carries"][0][0] >= 1                                   # into a finished byte of a first partition
    tokens = R.restate(R.make_field("alphabet", 2, 3, 1937), R.make_levels("edges", 2, 3, 1937), log2_parts=1)
    assert sum(c for c, _ in tokens["carries"][1:]) >= 1                 # ... of a token partition
    through = R.restate(None, R.carry_levels())
    assert through["carries"][1][1] >= 1 and through["status"] == 0      # ... through a 0xFF byte


def reference_listing(key, ivf):
    """the reference decoder's per-frame MD5s of the stream in `ivf`: printed by oracle/_ref/ref_md5 where it is built (and then
    equal to the recorded listing), else the listing recorded from it for a stream with the same SHA-256"""
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


DECODE_CASES = {  # width, height, vector field, levels, seed, log2 partitions
    "48x32_four_modes_and_a_skip": (48, 32, "alphabet", "sparse", 341, 0),
    "176x144_dense_8_partitions": (176, 144, "alphabet", "dense", 0, 3),
}


@pytest.mark.parametrize("name", DECODE_CASES)
def test_the_reference_decodes_restated_frames_like_the_oracle(pkg, name, tmp_path):
    """a key frame and the restatement's inter frame: the real reference decoder's frames are the oracle's from the IR the feeder
    reads back, and that IR is the one the frame was written from"""
    w, h, kind, content, seed, lp = DECODE_CASES[name]
    rows, cols = h // 16, w // 16
    hdr_k, mbs_k, coef_k, _ = synth_ir(w, h, seed + 1, inter=False, dense=0.3, segmented=False)
    r = R.restate(R.make_field(kind, rows, cols, seed), R.make_levels(content, rows, cols, seed), qindex=40, log2_parts=lp, filter_level=12)
    info = r["info"]
    if name.startswith("48x32"):
        assert all(info[12:16]) and 0 < info[11] < rows * cols and r["status"] == 0
    else:
        assert all(info[3:11]) and r["status"] & 7 == 0
    frames = [write_key_frame(hdr_k, mbs_k, coef_k), r["data"]]
    ivf = tmp_path / "s.ivf"
    write_ivf(ivf, w, h, frames)
    ref = reference_listing(name, ivf)
    g = pkg.geom(w, h)
    bufs = [np.zeros(g.frame_size, np.uint8) for _ in range(4)]
    parser = pkg.Parser()
    mine = []
    try:
        for k, data in enumerate(frames):
            hdr, _, mbs, coef, mvs = pkg.parse_to_numpy(parser, data)
            f = parser.refs
            new, lst, gld, alt = f.new_idx, f.lst_idx, f.gld_idx, f.alt_idx
            parser.swap(hdr)
            oracle_decode(hdr, mbs, coef, mvs, bufs[new], (bufs[lst], bufs[gld], bufs[alt]))
            mine.append(pkg.frame_md5(bufs[parser.refs.show_idx], g, w, h))
            if k == 1:
                assert hdr.base_qindex == 40 and hdr.num_token_partitions == 1 << lp and hdr.filter_level == 12
                assert np.array_equal(mbs[:, 0], r["mbs"][:, 0]) and np.array_equal(mbs[:, 2], r["mbs"][:, 2])
                assert np.array_equal(mbs[:, 3] & 1, r["mbs"][:, 3] & 1) and np.array_equal(mvs, r["mvs"])
                live = (r["mbs"][:, 3] & 1) == 0
                assert np.array_equal(coef[live], r["coef"][live])
    finally:
        parser.close()
    assert mine == ref
