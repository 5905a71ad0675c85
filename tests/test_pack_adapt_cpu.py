"""CPU: the probability adaptation of the frame packer (vp8hip_frames_pack_adapt_async; include/vp8hip.h).  The restatement the GPU
test compares with (tests/pack_adapt_reference.py) is held to what the reference's exported functions answer for seeded count sets
(tests/golden/pack_adapt_ref.json, written by tests/golden/make_pack_adapt_fixtures.py), to pack_reference's frame where nothing is
adapted, and -- its frames being decoded by the REAL reference decoder, oracle/_ref/ref_md5 where the reference is built, else its
listing recorded for the same stream bytes in tests/golden/pack_adapt_ref_md5.json (VP8_RECORD_REF_DIGESTS=1 with the reference built
rewrites it) -- to the frames the oracle produces.  Beside it the host side: the header prefix against BoolEncoder, the bound."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import pack_adapt_reference as A
import pack_reference as R
import vp8_writer as W
from vp8_testlib import GOLDEN, ROOT, oracle_decode, synth_ir
from vp8_writer import write_ivf, write_key_frame

REF_MD5 = os.path.join(ROOT, "oracle", "_ref", "ref_md5")
LISTINGS = os.path.join(GOLDEN, "pack_adapt_ref_md5.json")
RECORD = os.environ.get("VP8_RECORD_REF_DIGESTS") == "1"
FIXTURE = json.load(open(os.path.join(GOLDEN, "pack_adapt_ref.json")))

PREFIX_CASES = [dict(qindex=q, refresh_entropy_probs=r) for q in (0, 40, 127) for r in (0, 1)] + \
    [dict(deltas=tuple((-1) ** k * (3 + 3 * k) if i == k else 0 for i in range(5))) for k in range(5)] + \
    [dict(version=3, show_frame=0, filter_type=1, filter_level=63, sharpness=7, log2_parts=3, qindex=127, deltas=(15, -15, 15, -15, 15)),
     dict(refresh_golden=1, refresh_alt=1, copy_buffer_to_gf=2, copy_buffer_to_arf=1, sign_bias_golden=1, sign_bias_alt=1, refresh_last=0,
          refresh_entropy_probs=0),
     dict(refresh_golden=0, refresh_alt=0, copy_buffer_to_gf=2, copy_buffer_to_arf=1, sign_bias_alt=1, log2_parts=2)]


@pytest.mark.parametrize("case", PREFIX_CASES, ids=lambda c: "_".join(f"{k}{v}" for k, v in c.items()).replace(" ", ""))
def test_header_prefix_is_the_bool_encoders(pkg, case):
    """bytes and state of vp8hip_pack_header_prefix equal a BoolEncoder driven through the same fields, field by field; the carry
    form describes the same; continued through an empty probability section it is vp8hip_pack_header"""
    got = pkg.pack_header_prefix(**case)
    e = A.prefix_encoder(**case)
    assert got["bytes"] == bytes(e.out) and (got["bottom"], got["range"], got["bit_count"]) == (e.bottom, e.range, e.bit_count)
    b = got["bytes"]
    if b:
        assert got["settled"] + 1 + got["pending"] == len(b) and b[got["settled"]] == got["cache"] != 255
        assert b[got["settled"] + 1:] == b"\xff" * got["pending"] and len(b) <= 64
    else:
        assert got["cache"] == -1 and got["pending"] == got["settled"] == 0
    if case.get("refresh_entropy_probs", 1) == 1:
        T, f = W.tables(), {**R.DEFAULTS, **{k: v for k, v in case.items() if k in R.DEFAULTS}}
        for p in T["coef_update"]:
            e.put(0, p)
        e.literal(1, 1)
        for name in ("prob_skip_false", "prob_intra", "prob_last", "prob_gf"):
            e.literal(f[name], 8)
        e.literal(0, 2)
        for p in T["mv_update"]:
            e.put(0, p)
        whole = pkg.pack_header(**{k: v for k, v in case.items() if k != "refresh_entropy_probs"})
        assert whole["bytes"] == bytes(e.out) and (whole["bottom"], whole["range"], whole["bit_count"]) == (e.bottom, e.range, e.bit_count)


def test_the_prefix_follows_its_fields_and_refuses(pkg):
    base = pkg.pack_header_prefix()
    for name, v in dict(filter_type=1, filter_level=9, sharpness=2, refresh_last=0, refresh_golden=1, sign_bias_alt=1, log2_parts=1,
                        refresh_entropy_probs=0).items():
        assert pkg.pack_header_prefix(**{name: v}) != base, name
    for name, v in dict(prob_skip_false=7, prob_intra=9, prob_last=11, prob_gf=13, ref_frame=2).items():
        assert pkg.pack_header_prefix(**{name: v}) == base, name           # (behind the prefix; the macroblocks')
    for bad in (dict(qindex=128), dict(refresh_entropy_probs=2), dict(refresh_entropy_probs=-1), dict(deltas=(0, 0, 0, 0, 16)), dict(log2_parts=4),
                dict(prob_gf=0), dict(nonsense=1)):
        with pytest.raises(ValueError):
            pkg.pack_header_prefix(**bad)


def test_the_tables_are_the_references(pkg):
    """vp8t_prob_cost is vp8_prob_cost; both update tables lie above 127, where the reference's unsigned `cost_one - cost_zero`
    cannot wrap; the default set is the default tables"""
    assert A.prob_cost() == FIXTURE["cost"]
    T = W.tables()
    assert min(T["coef_update"]) >= 128 and min(T["mv_update"]) >= 128
    d = pkg.pack_probs_default()
    assert d.dtype == np.uint8 and d.shape == (1104,) and d[:1056].tolist() == list(T["coef"]) and d[1056:1094].tolist() == list(T["mvc"])
    assert not d[1094:].any() and np.array_equal(d, A.default_probs())


def test_tree_probabilities_are_the_references():
    for c in FIXTURE["tree"]:
        br = A.coef_branches(c["counts"])
        assert [list(b) for b in br] == c["branch"] and A.tree_probs(br) == c["probs"], c["counts"]


@pytest.mark.parametrize("case", FIXTURE["savings"], ids=lambda c: c["name"].replace(" ", "_"))
def test_coefficient_choice_is_the_references(case):
    """the fitted probabilities of every context, and the sum of the positive savings the reference returns"""
    counts = np.zeros(1152, np.int64)
    for i, n in case["counts"].items():
        counts[int(i)] = n
    base = A.default_probs()[:1056] if case["base"] == "default" else np.array(case["base"], np.uint8)
    newp = [p for row in range(96) for p in A.tree_probs(A.coef_branches(counts[row * 12:row * 12 + 12]))]
    assert newp == case["newp"]
    eff, flag, saved = A.choose_coef(counts, base)
    assert saved == case["saving"] & 0xffffffff                             # (its int wraps in the saturated cases; the call's uint32 alike)
    assert all(eff[i] == (newp[i] if flag[i] else base[i]) for i in range(1056))
    if case["name"].startswith("saving of exactly"):
        assert sum(flag) == saved == int(case["name"][-1])                  # s = 0: no update; s = 1: the one update
    if case["name"] == "empty":
        assert not any(flag)
    assert A.choose_coef(counts, base, on=False)[1:] == ([0] * 1056, 0)


@pytest.mark.parametrize("case", FIXTURE["mv"], ids=lambda c: c["name"].replace(" ", "_"))
def test_vector_choice_is_the_references(case):
    """the context after vp8_write_mvprobs and the bytes it wrote"""
    T = W.tables()
    before = np.array(case["before"], np.uint8)
    e = W.BoolEncoder()
    after, flags = [], []
    for comp in range(2):
        events = np.zeros(2047, np.int64)
        for d, n in case["events"][str(comp)].items():
            events[1023 + int(d)] = n
        m = A.reduce_events(events)
        direct = [0] * 32                                                   # the same reduction event by event, as the device counts
        for d, n in case["events"][str(comp)].items():
            for k in A.component_bins(int(d)):
                direct[k] = (direct[k] + n) & 0xffffffff
        assert [v & 0xffffffff for v in m] == direct
        eff, flag = A.choose_mv(m, before[19 * comp:19 * comp + 19], comp)
        for k in range(19):
            e.put(flag[k], T["mv_update"][19 * comp + k])
            if flag[k]:
                e.literal(eff[k] >> 1, 7)
                assert (eff[k] >> 1 << 1 or 1) == eff[k]                    # what a decoder makes of the literal
        after += eff
        flags += flag
    assert after == case["after"]
    for _ in range(32):                                                     # vp8_stop_encode
        e.put(0, 128)
    assert bytes(e.out).hex() == case["bytes"]
    if case["name"] == "empty":
        assert not any(flags)
    if case["name"].startswith("is_short"):
        assert flags[0] == ("above" in case["name"])


def test_without_flags_the_frame_is_pack_references():
    """no flags, the default baseline, refresh_entropy_probs 1, the same prob_skip_false: byte for byte pack_reference's frame"""
    for rows, cols, field, levels, seed, lp in ((2, 3, "alphabet", "sparse", 341, 0), (9, 11, "far", "dense", 0, 3), (1, 1, "zero", "edges", 2, 1)):
        r = A.restate(R.make_field(field, rows, cols, seed), R.make_levels(levels, rows, cols, seed), flags=0, log2_parts=lp, prob_skip_false=77,
                      ref_frame=2)
        assert r["data"] == r["default"] and r["info"][:16].tolist() == r["plain"]["info"].tolist()
        assert r["info"][16:].tolist() == [0, 0, 77, 0] + [0] * 12 and np.array_equal(r["probs_out"], A.default_probs()) and not any(r["flag"])
        assert r["counts"].sum() > 0


def test_the_adapted_dense_frame_is_smaller():
    """176x144 dense at qindex 40: fitted tables pay; every flag alone never costs more than a handful of bytes"""
    mv, lv = R.make_field("alphabet", 9, 11, 0), R.make_levels("dense", 9, 11, 0)
    r = A.restate(mv, lv, qindex=40, log2_parts=3)
    assert len(r["data"]) < len(r["default"]) * 0.6 and r["info"][16] > 200 and r["info"][19] > 8 * (len(r["default"]) - len(r["data"])) * 0.9
    assert r["info"][18] == 255 and r["info"][1] == len(r["data"])


def test_the_bound_holds_with_every_probability_updated(pkg):
    """the probability section with all 1094 updates, against the bound's share for it"""
    f = dict(R.DEFAULTS)
    eff = [255] * 1094
    mbs, tokens = A.mb_events(np.zeros((1, 1, 2), np.int64), 1, 1), [[]]
    full, sizes = A.write_frame(f, 40, (0,) * 5, 1, mbs, [True], tokens, eff, [1] * 1094, (255, 255, 255, 255))
    none, sizes0 = A.write_frame(f, 40, (0,) * 5, 1, mbs, [True], tokens, eff, [0] * 1094, (255, 255, 255, 255))
    assert 1094 < sizes[0] - sizes0[0] <= A.UPDATE_BYTES == (7 * (1056 * 9 + 35 + 38 * 8) + 7) // 8 // 16 * 16 + 16
    assert pkg.pack_adapt_bound(16, 16) == pkg.pack_bound(16, 16) + A.UPDATE_BYTES >= len(full)
    worst = np.full((1, 1, 25, 16), R.MAX_LEVEL, np.int16) * np.where(np.arange(16) & 1, -1, 1).astype(np.int16)
    assert pkg.pack_adapt_bound(16, 16) >= len(A.restate(None, worst)["data"])
    assert pkg.pack_adapt_bound(0, 16) == pkg.pack_adapt_bound(16, 16, 4) == 0 and pkg.pack_adapt_bound(176, 144, 3) % 16 == 0


def test_refused_jobs_count_nothing():
    mv, lv = R.make_field("alphabet", 2, 3, 5), R.make_levels("sparse", 2, 3, 5)
    odd = mv.copy(); odd[0, 1, 1] += 1
    r = A.restate(odd, lv)
    assert r["status"] & 7 == R.BAD_VECTOR and r["data"] is None and not r["counts"].any() and not r["info"][16:].any()
    n = len(A.restate(mv, lv)["data"])
    assert A.restate(mv, lv, cap=n)["status"] & 7 == 0 and A.restate(mv, lv, cap=n - 1)["status"] & 7 == R.OVERFLOW


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


DECODE_CASES = {  # width, height, vector field, levels, seed, log2 partitions, refresh_entropy_probs
    "48x32_four_modes_and_a_skip": (48, 32, "alphabet", "sparse", 341, 0, 1),
    "176x144_dense_8_partitions": (176, 144, "alphabet", "dense", 0, 3, 0),
    "176x144_long_vectors": (176, 144, "far", "sparse", 897, 1, 1),
}


@pytest.mark.parametrize("name", DECODE_CASES)
def test_the_reference_decodes_adapted_frames_like_the_oracle(pkg, name, tmp_path):
    """a key frame and the restatement's adapted inter frame: the real reference decoder's frames are the oracle's from the IR the
    feeder reads back, and that IR is the one the frame was written from -- so every update was coded as a decoder reads it"""
    w, h, kind, content, seed, lp, refresh = DECODE_CASES[name]
    rows, cols = h // 16, w // 16
    hdr_k, mbs_k, coef_k, _ = synth_ir(w, h, seed + 1, inter=False, dense=0.3, segmented=False)
    r = A.restate(R.make_field(kind, rows, cols, seed), R.make_levels(content, rows, cols, seed), qindex=40, log2_parts=lp, filter_level=12,
                  refresh_entropy_probs=refresh)
    info, ir = r["info"], r["plain"]
    assert info[16] > 0 and r["status"] & 7 == 0
    if name.startswith("48x32"):
        assert all(info[12:16]) and 0 < info[11] < rows * cols
    if name.endswith("long_vectors"):
        assert info[17] > 0 and info[15] > 90
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
                assert np.array_equal(mbs[:, 0], ir["mbs"][:, 0]) and np.array_equal(mbs[:, 2], ir["mbs"][:, 2])
                assert np.array_equal(mbs[:, 3] & 1, ir["mbs"][:, 3] & 1) and np.array_equal(mvs, ir["mvs"])
                live = (ir["mbs"][:, 3] & 1) == 0
                assert np.array_equal(coef[live], ir["coef"][live])
    finally:
        parser.close()
    assert mine == ref
