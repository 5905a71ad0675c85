"""Streams written at test time from seeds (tests/vp8_writer.py), and what the tests around them share:
 * inter_sequence: a key frame and inter frames of one size (tests/test_writer_cpu.py);
 * writer_reference_listing: what the REFERENCE decoder gave for a written stream, live or as recorded in
   tests/golden/writer_ref_md5.json; EXTREME_CASES: the two streams at 16383x16 and 16x16383 that the CPU and the GPU tests share;
 * size_change_stream: sections of different sizes one after the other -- every section's key frame makes the decoder allocate
   again (vp8/decoder/decodframe.c:771-808 -> vp8_alloc_frame_buffers, alloccommon.c:59-152) -- with the three streams MAIN, MFQE
   and ALIGNED of tests/test_sizechange_cpu.py and tests/test_gpu_sizechange.py;
 * decode_with_oracle: feeder + oracle (+ the oracle's post-processing) over a list of frames -> a listing in the format of
   oracle/ref_md5.c;
 * recorded: what the REFERENCE gave for a stream, live where oracle/_ref is built and else as recorded for a stream with the same
   SHA-256 in tests/golden/sizechange_ref.json (VP8_RECORD_REF_DIGESTS=1 with the reference built rewrites it);
 * the vpx_codec API of libvpx_hip.so through ctypes."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from vp8_testlib import GOLDEN, ROOT, load_package, oracle_frames, oracle_postproc_frames, synth_ir
from vp8_writer import write_inter_frame, write_ivf, write_key_frame

REFDIR = os.path.join(ROOT, "oracle", "_ref")
REF_MD5 = os.path.join(REFDIR, "ref_md5")
REF_MD5_EC = os.path.join(REFDIR, "ref_md5_ec")
REF_LIB = os.path.join(REFDIR, "libvpxref.so")
REF_VPXDEC = os.path.join(REFDIR, "vpxdec_ref")
SIZECHANGE_REF = os.path.join(GOLDEN, "sizechange_ref.json")
RECORD = os.environ.get("VP8_RECORD_REF_DIGESTS") == "1"


# ---- inter frames: every inter mode, all three references with sign biases, split vectors, and the segment map's three lives
# (coded, kept with new data, kept untouched) -- content the reference ENCODER never produces (it codes no map on inter frames)
def inter_sequence(w, h, seed, plan, lp=0, dense=0.25, big=False, tweak=None, mv_reach=None):
    """A key frame and one inter frame per entry of plan ("keep": segmentation on, nothing coded; "data": new segment data, map
    kept; "map": new map, data kept; "both"; "off": segmentation off).  Returns the frames and, per frame, the IR the stream was
    written from as a decoder is to read it back: (hdr, mbs, coef, mvs, segment map known).  tweak(k, hdr), if given, may change
    frame k's header just before it is written (it draws no random numbers: without it the streams are what they always were).
    mv_reach: synth_ir's bound on the inter frames' vectors, for pictures too large to draw them over (None: as ever)."""
    rng = np.random.default_rng(seed)
    hdr, mbs, coef, mvs = synth_ir(w, h, seed, inter=False, dense=dense, big=big, segmented=True)
    hdr.num_token_partitions = 1 << lp
    if tweak:
        tweak(0, hdr)
    frames, expect = [write_key_frame(hdr, mbs, coef, log2_parts=lp)], [(hdr, mbs, coef, mvs, True)]
    segmap, absd = mbs[:, 4].copy(), hdr.mb_segment_abs_delta
    segq, seglf = list(hdr.segment_quant), list(hdr.segment_lf)
    known = True
    for i, step in enumerate(plan):
        hdr, mbs, coef, mvs = synth_ir(w, h, seed * 100 + i + 1, inter=True, dense=dense, big=big, segmented=step != "off",
                                       mv_reach=mv_reach)
        hdr.num_token_partitions = 1 << lp
        hdr.refresh_last = int(rng.integers(0, 4) > 0)
        hdr.refresh_golden, hdr.refresh_alt = int(rng.integers(0, 3) == 0), int(rng.integers(0, 3) == 0)
        hdr.copy_buffer_to_gf = 0 if hdr.refresh_golden else int(rng.integers(0, 3))
        hdr.copy_buffer_to_arf = 0 if hdr.refresh_alt else int(rng.integers(0, 3))
        hdr.sign_bias_golden, hdr.sign_bias_alt = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        hdr.show_frame = int(rng.integers(0, 5) > 0)
        um = step in ("map", "both")
        ud = step in ("data", "both")
        if step != "off":
            if not um:
                mbs[:, 4] = segmap
            if not ud:
                hdr.mb_segment_abs_delta = absd
                for k in range(4):
                    hdr.segment_quant[k], hdr.segment_lf[k] = segq[k], seglf[k]
        if tweak:
            tweak(i + 1, hdr)
        data, mbs2, mvs2 = write_inter_frame(hdr, mbs, coef, mvs, log2_parts=lp, update_map=um, update_data=ud)
        if um:
            segmap, known = mbs[:, 4].copy(), True
        if ud:
            absd, segq, seglf = hdr.mb_segment_abs_delta, list(hdr.segment_quant), list(hdr.segment_lf)
        if step == "off":
            known = False                               # (what a later frame that keeps "the" map sees is the decoder's business)
        frames.append(data)
        expect.append((hdr, mbs2, coef, mvs2, known))
    return frames, expect


# ---- the reference decoder's listings of streams of the writer (tests/test_writer_cpu.py and the GPU tests over the same streams)
WRITER_LISTINGS = os.path.join(GOLDEN, "writer_ref_md5.json")


def writer_reference_listing(key, ivf):
    """The reference decoder's per-frame MD5s of the stream in `ivf`: printed by oracle/_ref/ref_md5 where it is built (and then
    equal to the recorded listing), else the listing recorded from it for a stream with the same SHA-256."""
    sha = hashlib.sha256(open(ivf, "rb").read()).hexdigest()
    table = json.load(open(WRITER_LISTINGS)) if os.path.exists(WRITER_LISTINGS) else {}
    live = None
    if os.path.exists(REF_MD5):
        out = str(ivf) + ".md5"
        r = subprocess.run([REF_MD5, str(ivf), out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        live = [l.split()[0] for l in open(out)]
    if RECORD:
        assert live is not None, "VP8_RECORD_REF_DIGESTS=1 needs the reference build (make -C oracle ref)"
        table[key] = {"stream_sha256": sha, "md5": live}
        with open(WRITER_LISTINGS, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    rec = table.get(key)
    assert rec is not None, f"{key}: no reference listing recorded in {WRITER_LISTINGS}"
    assert rec["stream_sha256"] == sha, f"{key}: the written stream is not the one the reference listing was recorded from"
    if live is not None:
        assert live == rec["md5"], key
    return rec["md5"]


# The ends of the size range vp8hip_configure accepts (16383 either way): a key frame and three inter frames, 1024 macroblocks in
# one row under eight token partitions, and in one column.  Vectors no further than 2040 eighth-pel units: what the writer can
# code as one difference.  width, height, seed, plan, log2 partitions, big coefficients, mv_reach
EXTREME_CASES = [
    (16383, 16, 27, ("keep", "both", "data"), 3, False, 2040),
    (16, 16383, 26, ("keep", "map", "both"), 0, False, 2040),
]
_extreme = {}


def extreme_sequence(case):
    """-> (frames, expect) of inter_sequence for one of EXTREME_CASES; written once a process (a second or two each)"""
    if case not in _extreme:
        w, h, seed, plan, lp, big, reach = case
        _extreme[case] = inter_sequence(w, h, seed, plan, lp, big=big, mv_reach=reach)
    return _extreme[case]


def extreme_key(case):
    """the name the reference's listing of the stream is recorded under in tests/golden/writer_ref_md5.json"""
    return "extreme_%dx%d_seed%d" % case[:3]


def extreme_listing(case, directory):
    """-> (frames, the reference decoder's per-frame MD5s) of one of EXTREME_CASES"""
    frames, _ = extreme_sequence(case)
    ivf = os.path.join(str(directory), extreme_key(case) + ".ivf")
    write_ivf(ivf, case[0], case[1], frames)
    return frames, writer_reference_listing(extreme_key(case), ivf)


# ---- streams that change their size: sections of (width, height, seed, plan, log2 token partitions)
def size_change_stream(sections, qindex=None):
    """One inter_sequence per section, the frames one after the other: every section's key frame carries its own size.  Returns the
    frames and, per frame, (hdr, mbs, coef, mvs) as a decoder reads them back.  Plans hold no "off", so every frame's segment
    map is known.  qindex(section, frame in the section) -> the frame's base_qindex, or None to leave what the seed gave."""
    frames, expect = [], []
    for s, (w, h, seed, plan, lp) in enumerate(sections):
        if "off" in plan:
            raise ValueError("size_change_stream: plans without \"off\"")

        def tweak(k, hdr, s=s):
            q = qindex(s, k) if qindex else None
            if q is not None:
                hdr.base_qindex = q
        f, e = inter_sequence(w, h, seed, plan, lp, tweak=tweak)
        frames += f
        expect += [x[:4] for x in e]
    return frames, expect


def section_starts(sections):
    """the index of every section's key frame in the stream's frames"""
    out, at = [], 0
    for _, _, _, plan, _ in sections:
        out.append(at)
        at += 1 + len(plan)
    return out


def size_changing(sections):
    """the indices of the key frames that change the size (the first frame included: nothing -> first size)"""
    starts = section_starts(sections)
    return [at for i, at in enumerate(starts) if i == 0 or sections[i][:2] != sections[i - 1][:2]]


# Every plan begins with "keep": the segment map an inter frame keeps right after the reallocation is the new key frame's.  Token
# partitions rotate through 1, 2, 4, 8.  The seeds are the first from 201 + section (ALIGNED: 301 +
# section), in steps of 20, whose section passes assert_stream_covers -- and, for three sections of MAIN, hides one of its frames.
MAIN = [
    (48, 32, 201, ("keep", "data", "map"), 0),
    (176, 144, 222, ("keep", "both", "keep"), 1),
    (67, 45, 203, ("keep", "map", "data"), 2),
    (67, 45, 204, ("keep", "data"), 3),               # a key frame of the same size: no reallocation, references not reset
    (80, 48, 205, ("keep", "keep", "both"), 0),       # the same 5x3 macroblocks ...
    (70, 40, 206, ("keep", "map"), 1),                # ... and another display size
    (16, 16, 207, ("keep", "data"), 2),               # one macroblock: mb_rows 1 under 4 parser threads
    (130, 98, 228, ("keep", "both", "data"), 3),
    (48, 32, 209, ("keep", "map", "keep"), 0),        # back to an earlier size
    (16, 400, 230, ("keep", "data", "keep"), 1),
    (1040, 16, 211, ("keep", "both"), 2),
]
MFQE_SECTIONS = MAIN[:9]
ALIGNED = [
    (48, 32, 341, ("keep", "data", "map"), 0),
    (176, 144, 302, ("keep", "both"), 1),
    (16, 16, 303, ("keep", "data"), 2),
    (64, 48, 324, ("keep", "map", "keep"), 3),
    (48, 32, 305, ("keep", "both", "data"), 0),
]


def mfqe_qindex(section, k):
    """Key frames at 20, the inter frames after them at 45, 60, 70: a key frame is never above the frame shown before it, so MFQE
    (which acts on frames 10 or more above the running quantiser, postproc.c:948) cannot fire on a key frame, and every shown inter
    frame is 10 or more above the running value (20 -> 26 -> 34 -> 43 when all are shown)."""
    return (20, 45, 60, 70)[k]


# (stream, post-processing configuration {post_proc_flag, deblocking_level, noise_level} or None) of every listing the reference
# decoder is asked for: MFQE (1024) only where it cannot act on a key frame that changes the size, and together with a deblocking
# filter only at sizes that are multiples of 16 (elsewhere the reference dies: tests/golden/make_fixtures.py)
LISTINGS = ([("MAIN", None)] + [("MAIN", pp) for pp in ((1, 0, 0), (2, 4, 0), (6, 6, 2), (5, 0, 1), (4, 0, 3))]
            + [("MFQE", (1024, 0, 0)), ("MFQE", (1028, 0, 3)), ("ALIGNED", (1027, 4, 0)), ("ALIGNED", (1030, 6, 2))])
STREAMS = {"MAIN": (MAIN, None), "MFQE": (MFQE_SECTIONS, mfqe_qindex), "ALIGNED": (ALIGNED, mfqe_qindex)}
_built = {}


def stream(name):
    """-> (sections, frames, expect) of MAIN, MFQE or ALIGNED; written once a process"""
    if name not in _built:
        sections, q = STREAMS[name]
        _built[name] = (sections,) + size_change_stream(sections, q)
    return _built[name]


def stream_ivf(name, directory):
    """the stream as an IVF file in `directory` (the header carries the first section's size, which no decoder here reads)"""
    sections, frames, _ = stream(name)
    path = os.path.join(str(directory), name.lower() + ".ivf")
    if not os.path.exists(path):
        write_ivf(path, sections[0][0], sections[0][1], frames)
    return path


def assert_stream_covers(sections, expect, hidden=0):
    """The stream still has its point: every section of two or more macroblocks has inter macroblocks on LAST, GOLDEN and ALTREF,
    a SPLITMV macroblock and a vector the decoder has to clamp; the frame after every key frame is an inter frame; `hidden`
    frames or more are not shown."""
    starts = section_starts(sections) + [len(expect)]
    for s, (w, h, _, plan, _) in enumerate(sections):
        part = expect[starts[s]:starts[s + 1]]
        assert part[0][0].frame_type == 0 and (part[0][0].width, part[0][0].height) == (w, h), s
        assert len(part) >= 3 and all(p[0].frame_type == 1 for p in part[1:]), s
        if part[0][0].mb_cols * part[0][0].mb_rows < 2:
            continue
        mbs = np.concatenate([p[1] for p in part[1:]])
        refs = set(mbs[:, 2].tolist())
        assert {1, 2, 3} <= refs, (s, refs)
        inter = mbs[:, 2] != 0
        assert (mbs[inter, 0] == 9).any(), (s, "no SPLITMV")
        assert (mbs[inter, 3] & 2).any(), (s, "no clamped vector")
    assert sum(1 for p in expect if not p[0].show_frame) >= hidden


# ---- the oracle's side
def listing_line(md5, w, h, k):
    return "%s  img-%dx%d-%04d.i420" % (md5, w, h, k)


def decode_with_oracle(frames, pp=None, lose=None):
    """Feeder + oracle over `frames`, with pp = (flags, deblocking level, noise level) the oracle's post-processing behind them:
    the listing oracle/ref_md5.c prints for the reference -- per shown frame "<md5>  img-<w>x<h>-<packet, 1-based>.i420".  With pp
    -> (listing, the OraclePostproc: its mfqe_frames says how often MFQE acted).  lose: 1-based packets that never arrive, with
    the feeder's error concealment on (what `ref_md5_ec --damage --ec --lose` does to the reference)."""
    P = load_package()
    if pp is not None:
        got, state = oracle_postproc_frames(frames, *pp)
        return [listing_line(md5, w, h, k) for md5, k, (w, h) in got], state
    out = []
    for k, (hdr, changed, mbs, coef, mvs, new, shown) in enumerate(oracle_frames(frames, lose=lose), 1):
        if shown is not None:
            out.append(listing_line(P.frame_md5(shown, P.geom(hdr.width, hdr.height), hdr.width, hdr.height), hdr.width, hdr.height, k))
    return out


def _headers(frames):
    """the frames' headers as the feeder reads them"""
    P = load_package()
    parser = P.Parser()
    out = []
    for data in frames:
        hdr, _, mbs, coef, mvs = P.parse_to_numpy(parser, data)
        parser.swap(hdr)
        out.append((hdr, mbs, mvs))
    parser.close()
    return out


def mfqe_fires(frames):
    """From the quantisers of the frames as read back: the 0-based indices of the shown frames MFQE acts on when VP8_MFQE is set
    (postproc.c:948-969 and :982-986: from the second shown frame on, where base_qindex is 10 or more above the running value,
    which then moves a quarter of the way; elsewhere the running value becomes the frame's)."""
    fires, last, shown = [], 0, 0
    for i, (hdr, _, _) in enumerate(_headers(frames)):
        if not hdr.show_frame:
            continue
        shown += 1
        if shown >= 2 and hdr.base_qindex - last >= 10:
            fires.append(i)
            last = (3 * last + hdr.base_qindex) >> 2
        else:
            last = hdr.base_qindex
    return fires


# ---- the reference's side
def recorded(key, ivf, live, what="lines"):
    """What the reference gave for the stream in `ivf`: live() where it returns something (the tool is built; then equal to what
    is recorded), else what was recorded under `key` for a stream with the same SHA-256."""
    sha = hashlib.sha256(open(ivf, "rb").read()).hexdigest()
    table = json.load(open(SIZECHANGE_REF)) if os.path.exists(SIZECHANGE_REF) else {}
    now = live()
    if RECORD:
        assert now is not None, "VP8_RECORD_REF_DIGESTS=1 needs the reference build (make -C oracle ref)"
        table[key] = {"stream_sha256": sha, what: now}
        with open(SIZECHANGE_REF, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    rec = table.get(key)
    assert rec is not None, f"{key}: nothing recorded in {SIZECHANGE_REF}"
    assert rec["stream_sha256"] == sha, f"{key}: the written stream is not the one the reference's answer was recorded from"
    if now is not None:
        assert now == rec[what], key
    return rec[what]


def run_ref_md5(ivf, args=(), tool=REF_MD5):
    """-> the listing `tool` writes for ivf, the tool's exit status where it is not 0 (a crash: negative), None where it is not built"""
    if not os.path.exists(tool):
        return None
    out = str(ivf) + ".ref.md5"
    r = subprocess.run([tool, *[str(a) for a in args], str(ivf), out], capture_output=True, text=True)
    if r.returncode:
        return r.returncode
    return open(out).read().splitlines()


def pp_key(name, pp):
    return name + ("" if pp is None else "-pp_%d_%d_%d" % tuple(pp))


def reference_listing(name, directory, pp=None):
    """the reference decoder's listing of stream `name`, plain or post-processed (oracle/_ref/ref_md5 [--pp F L N])"""
    ivf = stream_ivf(name, directory)
    return recorded(pp_key(name, pp), ivf, lambda: run_ref_md5(ivf, () if pp is None else ("--pp",) + tuple(pp)))


def reference_controls(ivf):
    """What the REFERENCE decoder answers, packet by packet, to VP8D_GET_LAST_REF_UPDATES, VP8D_GET_LAST_REF_USED and
    VP8D_GET_FRAME_CORRUPTED, through its public API in oracle/_ref/libvpxref.so (as tests/golden/make_fixtures.py records its
    .refctl files) -- in a process of its own: the library exports the names libvpx_hip.so exports.  None where it is not built."""
    if not os.path.exists(REF_LIB):
        return None
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ref-controls", str(ivf)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _ref_controls_main(ivf):
    L = ctypes.CDLL(REF_LIB)
    L.vpx_codec_vp8_dx.restype = ctypes.c_void_p
    L.vpx_codec_dec_init_ver.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    L.vpx_codec_decode.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long]
    L.vpx_codec_control_.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    data = open(ivf, "rb").read()
    pos, out = 32, []
    ctx = ctypes.create_string_buffer(256)
    assert L.vpx_codec_dec_init_ver(ctx, L.vpx_codec_vp8_dx(), None, 0, VPX_DECODER_ABI_VERSION) == 0
    while pos + 12 <= len(data):
        sz = int.from_bytes(data[pos:pos + 4], "little")
        fr = data[pos + 12:pos + 12 + sz]
        pos += 12 + sz
        assert L.vpx_codec_decode(ctx, fr, len(fr), None, 0) == 0
        v = [ctypes.c_int(-1) for _ in range(3)]
        for k, ctl in enumerate((VP8D_GET_LAST_REF_UPDATES, VP8D_GET_LAST_REF_USED, VP8D_GET_FRAME_CORRUPTED)):
            assert L.vpx_codec_control_(ctx, ctl, ctypes.byref(v[k])) == 0
        out.append([x.value for x in v])
    L.vpx_codec_destroy(ctx)
    print(json.dumps(out))


# ---- the vpx_codec API of libvpx_hip.so (include/vpx/*.h) through ctypes
VPX_DECODER_ABI_VERSION = 2 + 2 + 1
VPX_IMG_FMT_I420 = 0x100 | 2
VP8_SET_REFERENCE, VP8_COPY_REFERENCE, VP8_SET_POSTPROC = 1, 2, 3
VP8_LAST_FRAME, VP8_GOLD_FRAME, VP8_ALTR_FRAME = 1, 2, 4
VP8D_GET_LAST_REF_UPDATES, VP8D_GET_FRAME_CORRUPTED, VP8D_GET_LAST_REF_USED = 256, 257, 258
VPX_CODEC_USE_POSTPROC = 0x10000


class VpxImage(ctypes.Structure):        # include/vpx/vpx_image.h (vpx/vpx_image.h:103-147 in the reference)
    _fields_ = [("fmt", ctypes.c_int), ("w", ctypes.c_uint), ("h", ctypes.c_uint), ("d_w", ctypes.c_uint),
                ("d_h", ctypes.c_uint), ("x_chroma_shift", ctypes.c_uint), ("y_chroma_shift", ctypes.c_uint),
                ("planes", ctypes.POINTER(ctypes.c_ubyte) * 4), ("stride", ctypes.c_int * 4), ("bps", ctypes.c_int),
                ("user_priv", ctypes.c_void_p), ("img_data", ctypes.c_void_p), ("img_data_owner", ctypes.c_int),
                ("self_allocd", ctypes.c_int)]


class VpxRefFrame(ctypes.Structure):     # include/vpx/vp8.h (vpx/vp8.h:94-98)
    _fields_ = [("frame_type", ctypes.c_int), ("img", VpxImage)]


class PostprocCfg(ctypes.Structure):     # vp8_postproc_cfg_t, include/vpx/vp8.h (vpx/vp8.h:76-81)
    _fields_ = [("post_proc_flag", ctypes.c_int), ("deblocking_level", ctypes.c_int), ("noise_level", ctypes.c_int)]


class StreamInfo(ctypes.Structure):      # vpx_codec_stream_info_t, include/vpx/vpx_decoder.h
    _fields_ = [("sz", ctypes.c_uint), ("w", ctypes.c_uint), ("h", ctypes.c_uint), ("is_kf", ctypes.c_uint)]


def codec_lib():
    L = ctypes.CDLL(os.path.join(ROOT, "libvpx.opencl_amd", "lib", "libvpx_hip.so"))
    L.vpx_codec_vp8_dx.restype = ctypes.c_void_p
    L.vpx_codec_dec_init_ver.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    L.vpx_codec_decode.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long]
    L.vpx_codec_get_frame.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    L.vpx_codec_get_frame.restype = ctypes.POINTER(VpxImage)
    L.vpx_codec_get_stream_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(StreamInfo)]
    L.vpx_codec_control_.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.vpx_codec_destroy.argtypes = [ctypes.c_void_p]
    L.vpx_img_alloc.argtypes = [ctypes.POINTER(VpxImage), ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
    L.vpx_img_alloc.restype = ctypes.POINTER(VpxImage)
    L.vpx_img_free.argtypes = [ctypes.POINTER(VpxImage)]
    return L


def image_plane(img, k, w, h):
    st = img.stride[k]
    return b"".join(ctypes.string_at(ctypes.addressof(img.planes[k].contents) + r * st, w) for r in range(h))


def image_md5(img):
    w, h = img.d_w, img.d_h
    m = hashlib.md5()
    for k, (pw, ph) in enumerate(((w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2))):
        m.update(image_plane(img, k, pw, ph))
    return m.hexdigest()


class Decoder:
    """one vpx_codec decoder of libvpx_hip.so: decode(packet) -> (status, the image shown or None)"""

    def __init__(self, flags=0, pp=None):
        self.L = codec_lib()
        self.ctx = ctypes.create_string_buffer(256)
        assert self.L.vpx_codec_dec_init_ver(self.ctx, self.L.vpx_codec_vp8_dx(), None, flags, VPX_DECODER_ABI_VERSION) == 0
        if pp is not None:
            cfg = PostprocCfg(*pp)
            assert self.control(VP8_SET_POSTPROC, cfg) == 0

    def decode(self, data):
        rc = self.L.vpx_codec_decode(self.ctx, data, len(data), None, 0)
        it = ctypes.c_void_p()
        img = self.L.vpx_codec_get_frame(self.ctx, ctypes.byref(it)) if rc == 0 else None
        return rc, (img.contents if img else None)

    def control(self, ctl, arg):
        return self.L.vpx_codec_control_(self.ctx, ctl, ctypes.byref(arg))

    def get_int(self, ctl):
        v = ctypes.c_int(-1)
        assert self.control(ctl, v) == 0
        return v.value

    def stream_info(self):
        si = StreamInfo()
        si.sz = ctypes.sizeof(StreamInfo)
        assert self.L.vpx_codec_get_stream_info(self.ctx, ctypes.byref(si)) == 0
        return si.w, si.h

    def close(self):
        self.L.vpx_codec_destroy(self.ctx)


def codec_listing(frames, flags=0, pp=None):
    """the listing of `frames` through the vpx_codec API, in ref_md5's format"""
    d = Decoder(flags, pp)
    out = []
    for k, data in enumerate(frames, 1):
        rc, img = d.decode(data)
        assert rc == 0, k
        if img is not None:
            out.append(listing_line(image_md5(img), img.d_w, img.d_h, k))
    d.close()
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--ref-controls":
        _ref_controls_main(sys.argv[2])
