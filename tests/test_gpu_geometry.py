"""GPU (-m gpu): pictures at the ends of the size range vp8hip_configure accepts, through the C ABI, against the oracle.
The decoder's launch plan depends on the picture's geometry ("Launch plans at the ends of the size range"):
 * the wave-per-row reconstruction runs 12, 10, 8, 6, 4 or 2 waves a workgroup, by what two line buffers a wave cost in 160 KB of
   LDS -- every count at the first aligned width past its threshold or the last one before it, and every count again (and the
   loop filter's) by the library's knobs at ordinary widths; the workgroups per CU of a launch of more frame pairs than CUs;
 * 1024 macroblock columns: the lane-per-row family's row period and the tile rows.  (Not the cross-CU plan: it takes frames of
   five macroblock rows or more on two waves a workgroup, 5120 macroblocks at that width, and the pictures here have 3072 at the
   most.  The widest it takes here is 9104x80, 569 columns: granule rows of cols * 8 + 2 and cols * 32 granules.)
 * 1024 macroblock rows: a wave's hundreds of rounds, the cross-CU plan clipped to 32 workgroups of 8 waves, the border kernel's
   capped grid;
 * the device's entropy decoder takes a partition per lane up to 256 columns and 4096 column words a wave, a frame per lane past
   either: both sides of both limits.
Whole frame buffers are compared, borders included.  The content is seeded random IR (tests/vp8_testlib.py: synth_ir -- every
mode, sparse and dense coefficients, +-2047 on one seed, segments), inter frames over three random references with vectors up to
4000 eighth-pel units either way.  IR and the oracle's frames are made once and shared by the kernel families."""
import numpy as np
import pytest

from vp8_testlib import TALL_SIZES, WIDE_SIZES, bordered_area_equal, oracle_decode, random_frame, recon_waves_by_rule, synth_ir

pytestmark = pytest.mark.gpu

FAMILIES = ["wave1cu", "wave", "lane"]
MV_REACH = 4000
# inter, version, filter_type: key frames; inter frames with the six-tap filters; bilinear (1) / full-pixel (3) with the simple loop filter
MODES = [(False, 0, 0), (True, 0, 0), (True, 1, 1), (True, 3, 1)]
# (dense, big) by seed: sparse, dense with coefficients up to +-2047
CONTENT = [(0.15, False), (0.9, True)]


def set_family(monkeypatch, family):
    """The kernel families as tests/test_gpu_parity.py's fixture sets them: "wave1cu" = a wave per macroblock row, a frame pair on
    one CU; "wave" = the same with the cross-CU plan where the library chooses it; "lane" = a macroblock row per lane.  The knobs
    are read by vp8hip_configure: set them before it."""
    monkeypatch.setenv("VP8HIP_RECON", "simt" if family == "lane" else "wave")
    for k in ("VP8HIP_XCU", "VP8HIP_INTER_SPLIT", "VP8HIP_RECON_NW", "VP8HIP_LF_NW", "VP8HIP_WG_PER_CU"):
        monkeypatch.delenv(k, raising=False)
    if family == "wave1cu":
        monkeypatch.setenv("VP8HIP_XCU", "0")
        monkeypatch.setenv("VP8HIP_INTER_SPLIT", "0")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Vp8Hip(0)
    yield c
    c.close()


_made = {}


def made(pkg, w, h, seed, inter, version, ftype, dense, big, level=None):
    """-> (IR, the seeds of the three reference frames or None, the oracle's frame buffer) of one seeded frame; made once, never
    changed.  level: the frame's loop-filter level where the seed's own is not wanted (0: an unfiltered frame)."""
    key = (w, h, seed, inter, version, ftype, dense, big, level)
    if key not in _made:
        g = pkg.geom(w, h)
        ir = synth_ir(w, h, seed, inter=inter, version=version, filter_type=ftype, dense=dense, big=big, mv_reach=MV_REACH)
        if level is not None:
            ir[0].filter_level = level
        refs = [500 + 3 * seed + k for k in range(3)] if inter else None
        o = np.zeros(g.frame_size, np.uint8)
        oracle_decode(*ir, o, tuple(random_frame(g, r) for r in refs) if inter else (o, o, o), 7)
        _made[key] = (ir, refs, o)
    return _made[key]


def upload_refs(ctx, first, refs):
    for k in range(3):
        ctx.upload_frame(first + k, random_frame(ctx.g, refs[k]))


def decode_one(ctx, ir, refs):
    """the frame in slot 0 into buffer 0, its references uploaded into 1..3 -> the whole buffer"""
    if refs is not None:
        upload_refs(ctx, 1, refs)
    ctx.fill_slot(0, *ir)
    ctx.decode([(0, 0, (1, 2, 3) if refs is not None else None)], 7)
    return ctx.download_full(0)


# ---- the waves per workgroup of the wave-per-row reconstruction, by width (the sizes and their counts: tests/vp8_testlib.py,
# held to the rule on LDS by tests/test_geometry_cpu.py)
WIDE, TALL = WIDE_SIZES, TALL_SIZES
# what vp8hip_stats says of ONE frame of these sizes under the automatic cross-CU plan on the 256 CUs of an MI355X: (waves per
# workgroup, workgroups).  9104x80: five rows on workgroups of two waves -> two workgroups of four waves on two CUs of each XCD's
# round-robin slot, 8 * 2; the tall ones: 32 workgroups of eight waves, 8 * 32.  Every other wide size stays on one CU: four rows
# or fewer are one workgroup of four waves, and 2304x112 .. 2992x80 get no more waves from two CUs than they have on one.
CROSS_CU = {(9104, 80): (4, 16), (16, 16383): (8, 256), (48, 4112): (8, 256), (33, 8200): (8, 256)}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inter,version,ftype", MODES)
@pytest.mark.parametrize("w,h,nw", WIDE)
def test_wide_pictures(pkg, ctx, monkeypatch, family, w, h, nw, inter, version, ftype):
    set_family(monkeypatch, family)
    ctx.configure(w, h, 4, 1)
    for s, (dense, big) in enumerate(CONTENT):
        ir, refs, o = made(pkg, w, h, 11 + 2 * s + w % 97 + 3 * version, inter, version, ftype, dense, big)
        d = bordered_area_equal(decode_one(ctx, ir, refs), o, ctx.g)
        st = ctx.stats()
        print("%dx%d %s inter=%d v%d: recon_waves %d lf_waves %d workgroups %d" % (w, h, family, inter, version, st.recon_waves,
                                                                                 st.lf_waves, st.workgroups))
        assert not d, (w, h, family, s, d)
        if family == "wave1cu":
            assert st.recon_waves == nw == recon_waves_by_rule(w, h) and st.workgroups == 1, (w, h, st.recon_waves, st.workgroups)
        elif family == "wave":
            waves, groups = CROSS_CU.get((w, h), (nw, 1))
            assert (st.recon_waves, st.workgroups) == (waves, groups), (w, h, st.recon_waves, st.workgroups)
            assert st.lf_waves == waves or groups == 1 or not st.lf_kernels
        else:
            assert st.fused == 1 and st.recon_waves == 1


def test_every_wave_count_runs(pkg, ctx, monkeypatch):
    """What vp8hip_stats reports over the wide sizes, a key frame each on one CU: every count the rule has.  A rule that changes
    must not leave a count untested without anybody noticing."""
    set_family(monkeypatch, "wave1cu")
    seen = {}
    for w, h, nw in WIDE:
        ctx.configure(w, h, 4, 1)
        ir, refs, o = made(pkg, w, h, 11 + w % 97, False, 0, 0, *CONTENT[0])
        assert not bordered_area_equal(decode_one(ctx, ir, refs), o, ctx.g), (w, h)
        seen[(w, h)] = ctx.stats().recon_waves
    print("recon_waves by size:", seen)
    assert seen == {(w, h): nw for w, h, nw in WIDE} and set(seen.values()) == {12, 10, 8, 6, 4, 2}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inter,version,ftype", MODES)
@pytest.mark.parametrize("w,h", TALL)
def test_tall_pictures(pkg, ctx, monkeypatch, family, w, h, inter, version, ftype):
    set_family(monkeypatch, family)
    ctx.configure(w, h, 4, 1)
    for s, (dense, big) in enumerate(CONTENT):
        ir, refs, o = made(pkg, w, h, 21 + 2 * s + h % 89 + 3 * version, inter, version, ftype, dense, big)
        d = bordered_area_equal(decode_one(ctx, ir, refs), o, ctx.g)
        st = ctx.stats()
        print("%dx%d %s inter=%d v%d: recon_waves %d lf_waves %d workgroups %d" % (w, h, family, inter, version, st.recon_waves,
                                                                                 st.lf_waves, st.workgroups))
        assert not d, (w, h, family, s, d)
        if family == "wave1cu":
            assert st.recon_waves == 12 and st.lf_waves == 16
        elif family == "wave":          # (the plan this size is here for was taken, not the fall-back to a workgroup per pair)
            assert (st.recon_waves, st.workgroups) == CROSS_CU[(w, h)], (w, h, st.recon_waves, st.workgroups)
            assert st.lf_waves == 8 or not st.lf_kernels


# ---- several different frames in one launch
def launch_of(pkg, w, h, n, inter):
    """n frames of their own content, filter type and level; the second one unfiltered -> [(IR, references, oracle's buffer)]"""
    out = []
    for i in range(n):
        version, ftype = ((0, 0), (1, 1), (3, 1))[i % 3] if inter else (i % 4, i % 2)
        dense, big = ((0.15, False), (0.9, True), (0.4, False))[i % 3]
        out.append(made(pkg, w, h, 301 + 7 * i + w % 53, inter, version, ftype, dense, big, level=0 if i == 1 else 9 + 11 * i))
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("w,h,n", [(4016, 64, 3), (16383, 16, 3), (16, 16383, 5)])
def test_several_frames_in_one_launch(pkg, ctx, monkeypatch, family, w, h, n, inter):
    """An odd number of frames (the wave-per-row kernels take them in pairs: the last wave holds one), each with its own content
    and, inter frames, its own three references; every frame is compared."""
    set_family(monkeypatch, family)
    frames = launch_of(pkg, w, h, n, inter)
    assert sum(1 for ir, _, _ in frames if ir[0].filter_level == 0) == 1
    ctx.configure(w, h, 4 * n, n)
    jobs = []
    for i, (ir, refs, _) in enumerate(frames):
        if inter:
            upload_refs(ctx, n + 3 * i, refs)
        ctx.fill_slot(i, *ir)
        jobs.append((i, i, tuple(n + 3 * i + k for k in range(3)) if inter else None))
    ctx.decode(jobs, 7)
    st = ctx.stats()
    for i, (_, _, o) in enumerate(frames):
        d = bordered_area_equal(ctx.download_full(i), o, ctx.g)
        assert not d, (w, h, family, i, d)
    if family == "wave":                # (three pairs of 1024 rows: a pair to an XCD's slot, 32 workgroups of eight waves each)
        assert (st.recon_waves, st.workgroups) == ((8, 256) if h == 16383 else (recon_waves_by_rule(w, h), n)), (w, h, st.workgroups)


# ---- the wave counts apart from the width: the library's knobs, read by vp8hip_configure
def knob_frames(pkg, w, h, inter, n):
    return [made(pkg, w, h, 401 + 5 * i + w % 31, inter, (0, 1, 3)[i % 3] if inter else i % 4, i % 2, (0.15, 0.9, 0.4)[i % 3], i % 3 == 1,
                 level=0 if i == 1 else None) for i in range(n)]


def run_launch(ctx, w, h, frames, n, inter):
    """n jobs over the frames in turn (job i decodes frame i % len(frames)), references shared by the jobs of a frame -> stats;
    every job's buffer is compared"""
    m = len(frames)
    ctx.configure(w, h, n + 3 * m, n)
    for j, (ir, refs, _) in enumerate(frames):
        if inter:
            upload_refs(ctx, n + 3 * j, refs)
    jobs = []
    for i in range(n):
        j = i % m
        ctx.fill_slot(i, *frames[j][0])
        jobs.append((i, i, tuple(n + 3 * j + k for k in range(3)) if inter else None))
    ctx.decode(jobs, 7)
    st = ctx.stats()
    for i in range(n):
        d = bordered_area_equal(ctx.download_full(i), frames[i % m][2], ctx.g)
        assert not d, (w, h, n, i, d)
    return st


@pytest.mark.parametrize("family", ["wave1cu", "wave"])
@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("w,h", [(176, 144), (640, 368)])
def test_wave_counts_by_knob(pkg, ctx, monkeypatch, family, w, h, inter):
    """VP8HIP_RECON_NW and VP8HIP_LF_NW at widths where LDS allows every count: the line buffers, the progress flags and the "row
    above two macroblocks ahead" rule with 2..10 waves on 9 and 23 macroblock rows (rows a multiple of the count and not), the loop
    filter with 2..16.  (Neither kernel of the lane-per-row family reads these knobs.)  VP8HIP_WG_PER_CU with 40 frames changes
    nothing: 20 pairs never reach the cap of CUs x workgroups per CU, so these launches are the default's, asserted as such; the
    launch in which the knob decides is test_workgroups_per_cu's."""
    three = knob_frames(pkg, w, h, inter, 3)
    for nw in (2, 4, 6, 8, 10):
        set_family(monkeypatch, family)
        monkeypatch.setenv("VP8HIP_RECON_NW", str(nw))
        st = run_launch(ctx, w, h, three, 3, inter)
        print("%dx%d %s inter=%d VP8HIP_RECON_NW=%d: recon_waves %d workgroups %d" % (w, h, family, inter, nw, st.recon_waves, st.workgroups))
        # (on one CU the knob is the count; the cross-CU plan, where the library takes it, has four or eight waves of its own)
        assert st.recon_waves == nw if family == "wave1cu" else st.recon_waves in (nw, 4, 8), (nw, st.recon_waves)
    for nw in (2, 4, 8, 16):
        set_family(monkeypatch, family)
        monkeypatch.setenv("VP8HIP_LF_NW", str(nw))
        st = run_launch(ctx, w, h, three, 3, inter)
        print("%dx%d %s inter=%d VP8HIP_LF_NW=%d: lf_waves %d workgroups %d" % (w, h, family, inter, nw, st.lf_waves, st.workgroups))
        assert st.lf_kernels == 1
        assert st.lf_waves == nw if family == "wave1cu" else st.lf_waves in (nw, 4, 8), (nw, st.lf_waves)
    eight = knob_frames(pkg, w, h, inter, 8)
    for per_cu in (2, 8):
        set_family(monkeypatch, family)
        monkeypatch.setenv("VP8HIP_WG_PER_CU", str(per_cu))
        st = run_launch(ctx, w, h, eight, 40, inter)
        print("%dx%d %s inter=%d VP8HIP_WG_PER_CU=%d: workgroups %d" % (w, h, family, inter, per_cu, st.workgroups))
        assert st.workgroups == 40 or family == "wave"
        if family == "wave1cu":
            assert st.recon_waves == 12 and st.lf_waves == 16


@pytest.mark.parametrize("inter", [False, True])
def test_workgroups_per_cu(pkg, ctx, monkeypatch, inter):
    """VP8HIP_WG_PER_CU decides the grid only once a launch has more frame pairs than the device has CUs: 1100 frames of 48x32
    (550 pairs, 6 macroblocks each; eight different frames in turn) on one, two and eight workgroups per CU.  vp8hip_stats
    reports min(frames, CUs x workgroups per CU): a cap that doubles from 1 to 2 and is out of reach at 8.  With one workgroup per
    CU every workgroup decodes two or three pairs one after the other -- the persistent loop and its line-slot reuse guard --,
    with eight every pair has its own.  Every frame is compared.  (A launch of this size is a workgroup per pair in the "wave"
    family too: one run.)"""
    family = "wave1cu"
    w, h, n = 48, 32, 1100
    eight = knob_frames(pkg, w, h, inter, 8)
    groups = {}
    for per_cu in (1, 2, 8):
        set_family(monkeypatch, family)
        monkeypatch.setenv("VP8HIP_WG_PER_CU", str(per_cu))
        st = run_launch(ctx, w, h, eight, n, inter)
        print("%dx%d x %d %s inter=%d VP8HIP_WG_PER_CU=%d: workgroups %d recon_waves %d" % (w, h, n, family, inter, per_cu, st.workgroups,
                                                                                      st.recon_waves))
        groups[per_cu] = st.workgroups
        assert st.lf_kernels == 1 and st.fused == 0
    cus = groups[1]
    assert 0 < cus <= n // 4, groups             # (the knob decides: at least two pairs a workgroup at 1, more than one at 2)
    assert groups[2] == 2 * cus and groups[8] == min(n, 8 * cus), groups


# ---- the device's entropy decoder either side of its limits on the columns
ENTROPY = [  # width, height, log2 partitions: a partition per lane while cols <= 256 and cols * (64 / partitions) <= 4096
    (2048, 32, 1), (2064, 32, 1),                                  # 128 columns x 32 frames a wave = 4096: the last that stays; 129
    (4096, 32, 2), (4096, 32, 3), (4112, 32, 2), (4112, 32, 3),    # 256 columns; 257
    (16383, 16, 3),
]
_written = {}


def written(pkg, w, h, lp):
    """three key frames of the suite's writer, two contents and three skip probabilities -> (frames, the host feeder's IR)"""
    from vp8_writer import write_key_frame
    if (w, h, lp) not in _written:
        frames = []
        for seed, p, dense, big in ((31, 200, 0.3, False), (32, 1, 0.6, True), (31, 255, 0.3, False)):
            hdr, mbs, coef, mvs = synth_ir(w, h, seed + w % 41, inter=False, filter_type=seed & 1, dense=dense, big=big)
            hdr.num_token_partitions = 1 << lp
            frames.append(write_key_frame(hdr, mbs, coef, log2_parts=lp, prob_skip_false=p))
        parser, host = pkg.Parser(), []
        for data in frames:
            hdr, _, mbs, coef, mvs = pkg.parse_to_numpy(parser, data)
            parser.swap(hdr)
            o = np.zeros(pkg.geom(w, h).frame_size, np.uint8)
            oracle_decode(hdr, mbs, coef, mvs, o, (o, o, o), 7)
            host.append((hdr, mbs, coef, o))
        parser.close()
        _written[(w, h, lp)] = (frames, host)
    return _written[(w, h, lp)]


@pytest.mark.parametrize("w,h,lp", ENTROPY)
def test_device_entropy_decoder_at_the_column_limits(pkg, monkeypatch, w, h, lp):
    """As test_written_streams of tests/test_gpu_entropy.py: no status, the host feeder's IR; and the frames decoded from that IR
    -- by each kernel family in turn: the entropy decoder does not depend on the family, so its IR is read back once -- are the
    oracle's.  (Which of the two kernels ran, vp8hip_stats does not say: the sizes stand either side of each limit.)"""
    from test_gpu_entropy import _compare, _export
    for k in ("VP8HIP_ENTROPY_PARTS", "VP8HIP_ENTROPY_LANES"):
        monkeypatch.delenv(k, raising=False)
    frames, host = written(pkg, w, h, lp)
    efs = _export(pkg, frames)
    assert all(e.num_tok == 1 << lp for e in efs)
    n = len(frames)
    c = pkg.Vp8Hip(0)                    # (a context of its own: the entropy decoder reads its knobs once a context)
    try:
        for family in FAMILIES:
            set_family(monkeypatch, family)
            c.configure(w, h, n, n)      # (the families' knobs are read here; the slots start over)
            assert not c.entropy_decode(0, efs, frames).any()
            if family == FAMILIES[0]:
                for i, (_, mbs, coef, _) in enumerate(host):
                    _compare(c, i, mbs, coef, (w, h, lp, i))
            c.decode([(i, i, (-1, -1, -1)) for i in range(n)], pkg.STAGE_ALL)
            for i, (_, _, _, o) in enumerate(host):
                d = bordered_area_equal(c.download_full(i), o, c.g)
                assert not d, (w, h, lp, family, i, d)
    finally:
        c.close()


# ---- whole streams at 16383x16 and 16x16383 against the reference decoder's recorded listing
@pytest.mark.parametrize("family", ["wave", "lane"])
@pytest.mark.parametrize("which", [0, 1])
def test_extreme_streams_frame_by_frame(pkg, monkeypatch, tmp_path, family, which):
    """pkg.decode_ivf_gpu -- the host feeder, one frame per launch -- over the streams tests/test_writer_cpu.py pins to the
    reference decoder: every shown frame has the reference's MD5."""
    from stream_testlib import EXTREME_CASES, extreme_key, extreme_listing
    set_family(monkeypatch, family)
    case = EXTREME_CASES[which]
    _, ref = extreme_listing(case, tmp_path)
    assert pkg.decode_ivf_gpu(str(tmp_path / (extreme_key(case) + ".ivf")), device=0) == ref, extreme_key(case)
