"""CPU: the key-frame stream writer (tests/vp8_writer.py) against the two decoders that matter:
 * the host feeder must read back exactly the IR the stream was written from (modes, segments, sub-block modes, eobs,
   coefficients) -- a round trip through bool coder, mode trees, token trees and contexts;
 * the REAL reference decoder must decode the stream to the frames the oracle produces from that IR: oracle/_ref/ref_md5
   where the reference is built here (oracle/Makefile), else its listing recorded for the same stream bytes
   (tests/golden/writer_ref_md5.json; VP8_RECORD_REF_DIGESTS=1 with the reference built rewrites it).  This pins feeder
   AND oracle on content no encoder would choose: every mode everywhere, all segment / delta features, 1..8 token
   partitions, coefficients up to +-2047, odd sizes."""
import numpy as np
import pytest

from stream_testlib import (EXTREME_CASES, extreme_key, extreme_listing, extreme_sequence, inter_sequence,
                            writer_reference_listing as reference_listing)
from vp8_testlib import load_package, oracle_decode, synth_ir
from vp8_writer import write_ivf, write_key_frame

CASES = [  # width, height, seed, log2 partitions, filter_type, dense, big coefficients, segmented
    (16, 16, 1, 0, 0, 0.5, False, True), (48, 32, 2, 1, 1, 0.4, False, True), (176, 144, 3, 2, 0, 0.3, True, True),
    (130, 98, 4, 3, 0, 0.3, False, False), (33, 200, 5, 0, 1, 0.2, True, True), (640, 368, 6, 2, 0, 0.08, False, True),
    (320, 16, 7, 3, 0, 0.6, True, False),
]


def _stream(case):
    w, h, seed, lp, ftype, dense, big, seg = case
    hdr, mbs, coef, mvs = synth_ir(w, h, seed, inter=False, filter_type=ftype, dense=dense, big=big, segmented=seg)
    hdr.num_token_partitions = 1 << lp
    return hdr, mbs, coef, mvs, write_key_frame(hdr, mbs, coef, log2_parts=lp)


@pytest.mark.parametrize("case", CASES)
def test_feeder_reads_back_the_ir(pkg, case):
    hdr, mbs, coef, mvs, data = _stream(case)
    parser = pkg.Parser()
    h2, _, m2, c2, _ = pkg.parse_to_numpy(parser, data)
    parser.close()
    for f in ("width", "height", "mb_cols", "mb_rows", "frame_type", "version", "filter_type", "filter_level",
              "sharpness_level", "segmentation_enabled", "mode_ref_lf_delta_enabled", "base_qindex", "y1dc_delta_q",
              "y2dc_delta_q", "y2ac_delta_q", "uvdc_delta_q", "uvac_delta_q", "num_token_partitions"):
        assert getattr(h2, f) == getattr(hdr, f), f
    if hdr.segmentation_enabled:
        assert h2.mb_segment_abs_delta == hdr.mb_segment_abs_delta
        assert list(h2.segment_quant) == list(hdr.segment_quant) and list(h2.segment_lf) == list(hdr.segment_lf)
        assert np.array_equal(m2[:, 4], mbs[:, 4])
    if hdr.mode_ref_lf_delta_enabled:
        assert list(h2.ref_lf_deltas) == list(hdr.ref_lf_deltas) and list(h2.mode_lf_deltas) == list(hdr.mode_lf_deltas)
    assert np.array_equal(m2[:, 0], mbs[:, 0]) and np.array_equal(m2[:, 1], mbs[:, 1])
    assert np.array_equal(m2[:, 3] & 1, mbs[:, 3] & 1)
    bp = mbs[:, 0] == 4
    assert np.array_equal(m2[bp, 40:56], mbs[bp, 40:56])
    live = (mbs[:, 3] & 1) == 0
    assert np.array_equal(m2[live, 8:33], mbs[live, 8:33])
    assert np.array_equal(c2[live], coef[live])


@pytest.mark.parametrize("case", CASES)
def test_reference_decodes_written_streams_like_the_oracle(pkg, case, tmp_path, request):
    hdr, mbs, coef, mvs, data = _stream(case)
    ivf = tmp_path / "s.ivf"
    write_ivf(ivf, hdr.width, hdr.height, [data, data])
    ref = reference_listing(request.node.name, ivf)
    g = pkg.geom(hdr.width, hdr.height)
    buf = np.zeros(g.frame_size, np.uint8)
    oracle_decode(hdr, mbs, coef, mvs, buf, (None, None, None))
    mine = pkg.frame_md5(buf, g, hdr.width, hdr.height)
    assert ref == [mine, mine]


INTER_CASES = [  # width, height, seed, plan, log2 partitions, big coefficients
    (64, 48, 11, ("keep", "data", "keep", "map", "keep", "both", "keep"), 0, False),
    (176, 144, 12, ("keep", "keep", "data", "off", "both", "keep"), 1, False),
    (130, 98, 13, ("both", "keep", "map", "data"), 2, True),
    (33, 200, 14, ("off", "off", "both", "keep"), 0, False),
    (320, 192, 15, ("keep", "data", "map"), 3, False),
]


def _feed(pkg, frames):
    """feeder over the frames -> per frame (hdr, mbs, coef, mvs) and the frame-buffer indices before / after"""
    parser = pkg.Parser()
    out = []
    for data in frames:
        hdr, changed, mbs, coef, mvs = pkg.parse_to_numpy(parser, data)
        r = parser.refs
        idx = (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx)
        parser.swap(hdr)
        out.append((hdr, mbs, coef, mvs, idx, parser.refs.show_idx))
    parser.close()
    return out


@pytest.mark.parametrize("case", INTER_CASES)
def test_feeder_reads_back_inter_frames(pkg, case):
    w, h, seed, plan, lp, big = case
    frames, expect = inter_sequence(w, h, seed, plan, lp, big=big)
    got = _feed(pkg, frames)
    for k, ((hdr, mbs, coef, mvs, known), (h2, m2, c2, v2, _, _)) in enumerate(zip(expect, got)):
        for f in ("frame_type", "show_frame", "filter_type", "filter_level", "sharpness_level", "segmentation_enabled", "base_qindex",
                  "refresh_last", "refresh_golden", "refresh_alt", "copy_buffer_to_gf", "copy_buffer_to_arf", "sign_bias_golden",
                  "sign_bias_alt", "num_token_partitions"):
            if k == 0 and f.startswith(("refresh", "copy", "sign")):
                continue
            assert getattr(h2, f) == getattr(hdr, f), (k, f)
        if hdr.segmentation_enabled:
            assert h2.mb_segment_abs_delta == hdr.mb_segment_abs_delta, k
            assert list(h2.segment_quant) == list(hdr.segment_quant) and list(h2.segment_lf) == list(hdr.segment_lf), k
            if known:
                assert np.array_equal(m2[:, 4], mbs[:, 4]), k
        assert np.array_equal(m2[:, 0], mbs[:, 0]) and np.array_equal(m2[:, 2], mbs[:, 2]), k
        intra = mbs[:, 2] == 0
        assert np.array_equal(m2[intra, 1], mbs[intra, 1]), k
        assert np.array_equal(m2[:, 3] & 3, mbs[:, 3] & 3), k
        split = mbs[:, 0] == 9
        assert np.array_equal(m2[split, 5], mbs[split, 5]), k
        assert np.array_equal(v2, mvs), k
        live = (mbs[:, 3] & 1) == 0
        assert np.array_equal(m2[live, 8:33], mbs[live, 8:33]) and np.array_equal(c2[live], coef[live]), k


@pytest.mark.parametrize("case", INTER_CASES)
def test_reference_decodes_written_inter_streams_like_the_oracle(pkg, case, tmp_path, request):
    w, h, seed, plan, lp, big = case
    frames, _ = inter_sequence(w, h, seed, plan, lp, big=big)
    ivf = tmp_path / "s.ivf"
    write_ivf(ivf, w, h, frames)
    ref = reference_listing(request.node.name, ivf)
    g = pkg.geom(w, h)
    bufs = [np.zeros(g.frame_size, np.uint8) for _ in range(4)]
    mine = []
    for hdr, mbs, coef, mvs, (new, lst, gld, alt), show in _feed(pkg, frames):
        oracle_decode(hdr, mbs, coef, mvs, bufs[new], (bufs[lst], bufs[gld], bufs[alt]))
        if hdr.show_frame:
            mine.append(pkg.frame_md5(bufs[show], g, w, h))
    assert mine == ref


@pytest.mark.parametrize("case", EXTREME_CASES, ids=extreme_key)
def test_extreme_sizes_feeder_oracle_and_reference(pkg, case, tmp_path):
    """At 16383x16 and 16x16383 the feeder reads back the IR the stream was written from, and the reference decoder's listing is
    what feeder + oracle decode: the oracle had only been held to the reference at small sizes."""
    w, h = case[:2]
    frames, expect = extreme_sequence(case)
    _, ref = extreme_listing(case, tmp_path)
    got = _feed(pkg, frames)
    assert len(got) == 4 and [x[0].frame_type for x in got] == [0, 1, 1, 1]
    g = pkg.geom(w, h)
    bufs = [np.zeros(g.frame_size, np.uint8) for _ in range(4)]
    mine = []
    for k, ((hdr, mbs, coef, mvs, known), (h2, m2, c2, v2, (new, lst, gld, alt), show)) in enumerate(zip(expect, got)):
        assert (h2.width, h2.height, h2.mb_cols, h2.mb_rows) == (w, h, (w + 15) // 16, (h + 15) // 16), k
        assert h2.num_token_partitions == 1 << case[4], k
        assert np.array_equal(m2[:, 0], mbs[:, 0]) and np.array_equal(m2[:, 2], mbs[:, 2]), k
        assert np.array_equal(m2[:, 3] & 3, mbs[:, 3] & 3), k
        if known and hdr.segmentation_enabled:
            assert np.array_equal(m2[:, 4], mbs[:, 4]), k
        assert np.array_equal(v2, mvs), k
        live = (mbs[:, 3] & 1) == 0
        assert np.array_equal(m2[live, 8:33], mbs[live, 8:33]) and np.array_equal(c2[live], coef[live]), k
        oracle_decode(h2, m2, c2, v2, bufs[new], (bufs[lst], bufs[gld], bufs[alt]))
        if h2.show_frame:
            mine.append(pkg.frame_md5(bufs[show], g, w, h))
    inter = np.concatenate([e[1] for e in expect[1:]])
    assert (inter[:, 2] != 0).any() and (inter[:, 2] == 0).any() and (inter[inter[:, 2] != 0, 0] == 9).any()
    assert len(mine) >= 3 and mine == ref


@pytest.mark.parametrize("w,h,seed", [(176, 144, 12), (130, 98, 13), (33, 200, 14)])
def test_mv_reach_that_covers_the_picture_changes_nothing(w, h, seed):
    """synth_ir's mv_reach draws no random number: a reach at or above the picture's own span (in eighth-pel units) gives the
    arrays None gives, for seeds the suite uses."""
    span = (max((w + 15) // 16, (h + 15) // 16) * 16) * 8
    for reach in (span, span + 1, 1 << 20):
        a = synth_ir(w, h, seed, inter=True, dense=0.25)
        b = synth_ir(w, h, seed, inter=True, dense=0.25, mv_reach=reach)
        assert bytes(a[0]) == bytes(b[0])
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y)
    # ... and a reach below it does bound them (the generator would otherwise prove nothing at the large sizes)
    c = synth_ir(w, h, seed, inter=True, dense=0.25, mv_reach=64)
    assert np.abs(c[3]).max() <= 64 + 400 and not np.array_equal(c[3], a[3])


def test_mv_reach_makes_the_widest_inter_frame():
    """16383 pixels are 131064 eighth-pel units: without a reach the vectors leave int16 (synth_ir raises OverflowError).  With
    4000 they fit, go both ways, and some are flagged for clamping."""
    with pytest.raises(OverflowError):
        synth_ir(16383, 16, 5, inter=True)
    hdr, mbs, coef, mvs = synth_ir(16383, 16, 5, inter=True, mv_reach=4000)
    assert mvs.dtype == np.int16 and mbs.shape[0] == 1024
    inter = mbs[:, 2] != 0
    assert inter.sum() > 700
    assert np.abs(mvs.astype(np.int32)).max() <= 4000 + 400
    cols = mvs[inter, :, 1]
    assert (cols > 2000).any() and (cols < -2000).any()           # (far both ways: the reach is used, not just the sign)
    assert (mvs[inter, :, 0] > 0).any() and (mvs[inter, :, 0] < 0).any()
    assert (mbs[inter, 3] & 2).any() and not (mbs[~inter, 3] & 2).any()


def fuzz_case(seed):
    """a small inter sequence from a seed: size, plan, partitions, coefficient range"""
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(1, 14)) * 16 + int(rng.integers(-15, 1)), int(rng.integers(1, 11)) * 16 + int(rng.integers(-15, 1))
    w, h = max(w, 2), max(h, 2)
    plan = tuple(rng.choice(["keep", "data", "map", "both", "off"], size=int(rng.integers(2, 7))))
    return w, h, seed, plan, int(rng.integers(0, 4)), bool(rng.integers(0, 2))


FUZZ_SEEDS = list(range(100, 124))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_reference_decodes_fuzzed_inter_streams_like_the_oracle(pkg, seed, tmp_path, request):
    test_reference_decodes_written_inter_streams_like_the_oracle(pkg, fuzz_case(seed), tmp_path, request)


@pytest.mark.parametrize("seed", FUZZ_SEEDS[:8])
def test_feeder_reads_back_fuzzed_inter_frames(pkg, seed):
    test_feeder_reads_back_inter_frames(pkg, fuzz_case(seed))
