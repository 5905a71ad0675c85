"""The decoder's debug overlays (VP8_SET_DBG_*, vpxdec --pp-debug-info / --pp-dbg-*) on the CPU: the restatement in
tests/vis_reference.py, over the oracle's decode and post-processing, against what the reference decoder built with
CONFIG_POSTPROC_VISUALIZER showed (tests/golden/<stream>.vis_<tag>.md5, tests/golden/make_vis_fixtures.py); the product's
constant tables against the recorded ones."""
import ctypes
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_vis_fixtures import STREAMS, TAGS, tag_args  # noqa: E402
import vis_reference as V  # noqa: E402
from vp8_testlib import GOLDEN, ROOT, OraclePostproc, load_package, oracle_decode_ivf  # noqa: E402

_kept = {}


def vis_listing(name, tag):
    return [l.split()[0] for l in open(os.path.join(GOLDEN, f"{name}.vis_{tag}.md5"))]


def restated_listing(name, args):
    """oracle decode -> the oracle's post-processing in the configuration vpxdec makes of `args` -> the overlays, drawn into
    the post-processing buffer (which MFQE reads back for the next frame)"""
    P = load_package()
    if name not in _kept:
        _kept[name] = oracle_decode_ivf(name, keep_frames=True)[1]
    (pp_flag, level, noise), dbg = V.vpxdec_config(args)
    flags = V.flags_word(pp_flag, dbg)
    ctypes.CDLL(None).srand(1)
    pp = OraclePostproc(pp_flag & (1 | 2 | 4 | 1024), level, noise)
    out = []
    for hdr, mbs, coef, mvs, frame in _kept[name]:
        if not hdr.show_frame:
            continue
        g = P.geom(hdr.width, hdr.height)
        post = pp.frame(frame, g, hdr.filter_level, hdr, mbs, mvs)
        V.visualize(post, g, hdr, mbs, mvs, flags, dbg)
        pp.post[:] = post
        out.append(P.frame_md5(post, g, hdr.width, hdr.height))
    return out


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("name", STREAMS)
def test_restatement_reproduces_the_reference(name, tag):
    assert restated_listing(name, tag_args(name, tag)) == vis_listing(name, tag)


def test_constrain_line_and_bresenham():
    # clipping is inclusive of the width / height and goes one side after the other
    assert V.constrain_line(8, 40, 8, 8, 32, 32) == (32, 8)
    assert V.constrain_line(8, -20, 8, -20, 32, 32) == (0, 0)
    assert V.constrain_line(24, 60, 8, 44, 32, 32) == (32, 16)
    assert V.constrain_line(4, -3, 4, 40, 16, 16) == (2, 16)          # C division truncates towards zero (floor: 1)
    pts = V.line_points(0, 5, 0, 2)
    assert pts[0] == (0, 0) and pts[-1] == (5, 2) and len(pts) == 6
    assert V.line_points(3, 3, 9, 1) == [(3, y) for y in range(1, 10)]


def _c_table(text, name):
    m = re.search(name + r"\[[^\]]*\](?:\[[^\]]*\])?\s*=\s*\{(.*?)\};", text, re.S)
    assert m, name
    return [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1))]


def test_device_tables_are_the_recorded_ones():
    """csrc/hip/vp8_visualize.hip's glyphs and colours are the numbers tests/golden/vis_tables.json recorded from the reference"""
    T = json.load(open(os.path.join(GOLDEN, "vis_tables.json")))
    src = open(os.path.join(ROOT, "libvpx.opencl_amd", "csrc", "hip", "vp8_visualize.hip")).read()
    assert _c_table(src, "vis_glyph") == T["glyphs"][:128]
    assert all(g == 0 for g in T["glyphs"][128:])             # (bytes above 127 are negative chars: the blank glyph)
    assert _c_table(src, "vis_mb_colour") == sum(T["mb_mode_colours"], [])
    assert _c_table(src, "vis_b_colour") == sum(T["b_mode_colours"][:10], [])
    assert _c_table(src, "vis_ref_colour") == sum(T["ref_frame_colours"], [])


def test_vpxdec_parsing():
    assert V.vpxdec_config(["--pp-dbg-mvs=1023"]) == ((1027, 4, 0), (0, 0, 0, 1023))
    assert V.vpxdec_config(["--deblock", "--pp-debug-info=16"]) == ((16, 0, 0), (0, 0, 0, 0))
    assert V.vpxdec_config(["--mfqe", "--pp-debug-info=121", "--pp-dbg-ref-frame=0"]) == ((1145, 0, 0), (0, 0, 0, 0))


def test_dbg_controls_are_accepted():
    """VP8_SET_DBG_* on a decoder that has not touched the device yet: VPX_CODEC_OK, as the reference's vp8_set_dbg_options"""
    L = ctypes.CDLL(os.path.join(ROOT, "libvpx.opencl_amd", "lib", "libvpx_hip.so"))
    L.vpx_codec_vp8_dx.restype = ctypes.c_void_p
    L.vpx_codec_dec_init_ver.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    L.vpx_codec_control_.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.vpx_codec_destroy.argtypes = [ctypes.c_void_p]
    ctx = ctypes.create_string_buffer(256)
    assert L.vpx_codec_dec_init_ver(ctx, L.vpx_codec_vp8_dx(), None, 0x10000, 2 + 2 + 1) == 0     # VPX_CODEC_USE_POSTPROC
    for ctrl, value in ((4, 15), (5, 1023), (6, 1023), (7, 1023), (7, 0)):   # VP8_SET_DBG_COLOR_REF_FRAME .. VP8_SET_DBG_DISPLAY_MV
        assert L.vpx_codec_control_(ctx, ctrl, ctypes.c_int(value)) == 0, ctrl
    assert L.vpx_codec_destroy(ctx) == 0
