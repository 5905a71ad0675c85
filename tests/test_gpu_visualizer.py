"""GPU: the decoder's debug overlays (vp8/common/postproc.c:1007-1362, CONFIG_POSTPROC_VISUALIZER) drawn by vp8hip_visualize.
 * VP8_SET_DBG_* / VP8_SET_POSTPROC through the vpx_codec API against what the reference decoder built with the visualizer showed
   (tests/golden/<stream>.vis_<tag>.md5, tests/golden/make_vis_fixtures.py), for the whole matrix;
 * the product's vpxdec and the reference's vpxdec.c built against the product with the reference's option names
   (tests/golden/vis.vpxdec_md5);
 * random macroblocks -- every SPLITMV partitioning, vectors far outside the frame, steep and shallow lines, frames 16 to 80
   pixels wide -- through vp8hip_visualize against tests/vis_reference.py over the whole frame buffer, borders included;
 * the reference frames stay what they are with the overlays on."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_vis_fixtures import STREAMS, TAGS, tag_args  # noqa: E402
import vis_reference as V  # noqa: E402
from test_gpu_codec_api import (VP8_ALTR_FRAME, VP8_COPY_REFERENCE, VP8_GOLD_FRAME, VP8_LAST_FRAME, VPX_DECODER_ABI_VERSION,  # noqa: E402
                                VpxRefFrame, _lib, _md5, _plane)
from vp8_testlib import GOLDEN, ROOT, golden_md5, ivf_path, load_package, synth_ir  # noqa: E402

pytestmark = pytest.mark.gpu

VPX_CODEC_USE_POSTPROC = 0x10000
VP8_SET_POSTPROC = 3
VP8_SET_DBG = (4, 5, 6, 7)            # VP8_SET_DBG_COLOR_REF_FRAME, _MB_MODES, _B_MODES, VP8_SET_DBG_DISPLAY_MV
VPX_IMG_FMT_I420 = 0x102
REF_VPXDEC_ON_HIP = os.path.join(ROOT, "oracle", "_ref", "vpxdec_ref_on_hip")


class PostprocCfg(ctypes.Structure):     # vp8_postproc_cfg_t, include/vpx/vp8.h
    _fields_ = [("post_proc_flag", ctypes.c_int), ("deblocking_level", ctypes.c_int), ("noise_level", ctypes.c_int)]


def _decoder(L, args):
    """a decoder configured as the reference's vpxdec configures it for `args` (or a plain one for args None)"""
    ctx = ctypes.create_string_buffer(256)
    assert L.vpx_codec_dec_init_ver(ctx, L.vpx_codec_vp8_dx(), None, 0 if args is None else VPX_CODEC_USE_POSTPROC,
                                    VPX_DECODER_ABI_VERSION) == 0
    if args is not None:
        cfg, dbg = V.vpxdec_config(args)
        c = PostprocCfg(*cfg)
        assert L.vpx_codec_control_(ctx, VP8_SET_POSTPROC, ctypes.byref(c)) == 0
        for ctrl, value in zip(VP8_SET_DBG, dbg):
            if value:
                assert L.vpx_codec_control_(ctx, ctrl, ctypes.c_void_p(value)) == 0      # (an int, passed in a register)
    return ctx


def _listing(name, args):
    P = load_package()
    _, _, frames = P.read_ivf(ivf_path(name))
    L = _lib()
    ctx = _decoder(L, args)
    got = []
    for data in frames:
        assert L.vpx_codec_decode(ctx, data, len(data), None, 0) == 0
        it = ctypes.c_void_p()
        img = L.vpx_codec_get_frame(ctx, ctypes.byref(it))
        if img:
            got.append(_md5(img.contents))
    L.vpx_codec_destroy(ctx)
    return got


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("name", STREAMS)
def test_codec_api_against_the_reference_decoder(name, tag):
    gold = [l.split()[0] for l in open(os.path.join(GOLDEN, f"{name}.vis_{tag}.md5"))]
    assert _listing(name, tag_args(name, tag)) == gold


def _cli_cases():
    return [(l.split()[0], l.split()[1], l.split()[2:]) for l in open(os.path.join(GOLDEN, "vis.vpxdec_md5"))]


@pytest.mark.parametrize("name,md5,args", _cli_cases())
def test_vpxdec_options(name, md5, args):
    r = subprocess.run([os.path.join(ROOT, "libvpx.opencl_amd", "bin", "vpxdec"), *args, "--md5", "--i420", ivf_path(name)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == md5


@pytest.mark.skipif(not os.path.exists(REF_VPXDEC_ON_HIP), reason="oracle/_ref/vpxdec_ref_on_hip not built (make -C oracle ref)")
@pytest.mark.parametrize("name,md5,args", _cli_cases())
def test_reference_vpxdec_on_the_product(name, md5, args):
    """the reference's own vpxdec.c, linked with the product, passes VP8_SET_DBG_* and must get the reference's output"""
    r = subprocess.run([REF_VPXDEC_ON_HIP, *args, "--md5", "--i420", ivf_path(name)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == md5


def _random_macroblocks(hdr, mbs, mvs, rng, far):
    """modes of every kind over the synthetic IR: B_PRED with random sub-block modes, the inter modes, SPLITMV with all four
    partitionings; vectors short, long, or (far) reaching hundreds of pixels out, and some purely horizontal / vertical"""
    n = mbs.shape[0]
    inter = hdr.frame_type != 0
    modes = rng.integers(0, 10 if inter else 5, size=n)
    mbs[:, 0] = modes
    mbs[:, 2] = np.where(modes <= 4, 0, rng.integers(1, 4, size=n))
    mbs[:, 3] = (mbs[:, 3] & 0xfe) | rng.integers(0, 2, size=n)        # skip flag
    mbs[:, 5] = rng.integers(0, 4, size=n)
    mbs[:, 40:56] = rng.integers(0, 10, size=(n, 16))
    lim = 2047 if far else 160
    mvs[:] = rng.integers(-lim, lim + 1, size=mvs.shape)
    axis = rng.random(n) < 0.25
    mvs[axis, :, rng.integers(0, 2)] = 0
    small = rng.random(n) < 0.2
    mvs[small] = rng.integers(-9, 10, size=mvs[small].shape)
    for i in np.nonzero(modes != 9)[0]:                                 # one vector per macroblock outside SPLITMV
        mvs[i, :] = mvs[i, 0]


CASES = [(16, 16), (17, 33), (33, 17), (48, 32), (67, 45), (80, 16), (80, 80), (16, 80), (31, 47), (64, 48)]
VIS = [  # flags, (ref_frame, mb_modes, b_modes, mvs)
    (0x3f8, (15, 1023, 1023, 1023)),
    (0x3f8, (6, 4, 0, 992)),
    (V.CLR_BLK_MODES | V.DRAW_MV, (0, 0, 1 << 4, 512)),
    (V.CLR_BLK_MODES | V.CLR_FRM_REF_BLKS, (9, 0x3eb, 0, 0)),
    (V.TXT_FRAME_INFO | V.TXT_RATE_INFO | V.DRAW_MV, (0, 0, 0, 1023)),
]


@pytest.mark.parametrize("w,h", CASES)
def test_random_frames_against_the_restatement(w, h):
    P = load_package()
    ctx = P.Vp8Hip()
    ctx.configure(w, h, 1, 1)
    g = ctx.g
    rng = np.random.default_rng(w * 131 + h)
    drawn = 0
    try:
        for trial in range(10):
            inter = trial % 5 != 0
            hdr, mbs, coef, mvs = synth_ir(w, h, seed=w * 1000 + h * 10 + trial, inter=inter)
            _random_macroblocks(hdr, mbs, mvs, rng, far=trial % 2 == 1)
            ctx.fill_slot(0, hdr, mbs, coef, mvs)
            flags, dbg = VIS[trial % len(VIS)]
            info = V.frame_info(hdr, flags) if trial % 3 else "a string long enough to run on into the rows below: " * 2
            before = rng.integers(0, 256, size=g.frame_size).astype(np.uint8)
            ctx.upload_frame(0, before)
            ctx.visualize(0, 0, flags, *dbg, frame_info=info, rate_info=V.RATE_INFO)
            got = ctx.download_full(0)
            expect = V.visualize(before.copy(), g, hdr, mbs, mvs, flags, dbg, info=info)
            drawn += not np.array_equal(expect, before)
            bad = np.nonzero(got != expect)[0]
            assert bad.size == 0, (w, h, trial, flags, dbg, bad[:8], got[bad[:8]], expect[bad[:8]])
        assert drawn >= 5
    finally:
        ctx.close()


def test_bad_arguments():
    P = load_package()
    ctx = P.Vp8Hip()
    ctx.configure(64, 48, 2, 1)
    L = ctx.L
    try:
        v = P.VisParams(0x3f8, 15, 1023, 1023, 1023, b"x", b"y")
        assert L.vp8hip_visualize(ctx.h, 2, 0, ctypes.byref(v)) == -2
        assert L.vp8hip_visualize(ctx.h, 0, 1, ctypes.byref(v)) == -2
        assert L.vp8hip_visualize(ctx.h, 0, 0, None) == -2
        v.frame_info = b"x" * 600
        assert L.vp8hip_visualize(ctx.h, 0, 0, ctypes.byref(v)) == -2
    finally:
        ctx.close()


def _ref_planes(L, ctx, frame_type, w, h):
    ref = VpxRefFrame()
    ref.frame_type = frame_type
    assert L.vpx_img_alloc(ctypes.byref(ref.img), VPX_IMG_FMT_I420, w, h, 1)
    assert L.vpx_codec_control_(ctx, VP8_COPY_REFERENCE, ctypes.byref(ref)) == 0
    out = (_plane(ref.img, 0, w, h), _plane(ref.img, 1, w // 2, h // 2), _plane(ref.img, 2, w // 2, h // 2))
    L.vpx_img_free(ctypes.byref(ref.img))
    return out


@pytest.mark.parametrize("name", ["p_arf_176x144", "p_split_352x288"])
def test_reference_frames_are_untouched(name):
    """the overlays go into the post-processing buffer only: after every frame the three references of a decoder with all of
    them on are those of a plain decoder, and what the plain decoder shows is the stream's listing"""
    P = load_package()
    w, h, frames = P.read_ivf(ivf_path(name))
    aw, ah = (w + 15) & ~15, (h + 15) & ~15
    L = _lib()
    vis = _decoder(L, TAGS["all_mfqe"])
    plain = _decoder(L, None)
    shown = []
    for data in frames:
        for c in (vis, plain):
            assert L.vpx_codec_decode(c, data, len(data), None, 0) == 0
        it = ctypes.c_void_p()
        img = L.vpx_codec_get_frame(plain, ctypes.byref(it))
        if img:
            shown.append(_md5(img.contents))
        for rf in (VP8_LAST_FRAME, VP8_GOLD_FRAME, VP8_ALTR_FRAME):
            assert _ref_planes(L, vis, rf, aw, ah) == _ref_planes(L, plain, rf, aw, ah)
    L.vpx_codec_destroy(vis)
    L.vpx_codec_destroy(plain)
    assert shown == golden_md5(name)
