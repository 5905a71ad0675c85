"""The decoder's debug overlays (vp8/common/postproc.c:1007-1362, CONFIG_POSTPROC_VISUALIZER) restated in Python from what they
mean, for the tests: text, motion vectors, block-mode colours and reference-frame colours drawn, in that order, into a frame buffer
of the vp8ir_geom layout (include/vp8_ir.h) in place.

Everything is addressed linearly from the luma plane's origin with the luma stride, as the reference does: a string longer than
a row runs on into the rows below, a line that leaves the picture lands in the border or in the next plane.  What would land
outside the frame buffer is dropped (the reference writes past its allocation there).

The numbers -- glyphs and colour triples -- are the reference's, recorded in tests/golden/vis_tables.json."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# VP8D_DEBUG_* (vp8/common/ppflags.h)
TXT_FRAME_INFO, TXT_MBLK_MODES, TXT_DC_DIFF, TXT_RATE_INFO = 1 << 3, 1 << 4, 1 << 5, 1 << 6
DRAW_MV, CLR_BLK_MODES, CLR_FRM_REF_BLKS = 1 << 7, 1 << 8, 1 << 9
B_PRED, NEARESTMV, SPLITMV = 4, 5, 9
ALPHA = 0xc000
# the rate string: the reference never computes bitrate or frame rate (onyxd_if.c:653 is compiled out), both stay 0
RATE_INFO = "Bitrate: %10.2f frame_rate: %10.2f " % (0.0, 0.0)

_tables = None


def tables():
    global _tables
    if _tables is None:
        with open(os.path.join(HERE, "golden", "vis_tables.json")) as f:
            _tables = json.load(f)
    return _tables


def frame_info(hdr, flags):
    """the frame-info string (postproc.c:1010-1017): key frame, golden refresh, quantiser, loop-filter level, the flags word, size
    in macroblocks"""
    return "F%1dG%1dQ%3dF%3dP%d_s%dx%d" % (hdr.frame_type == 0, hdr.refresh_golden, hdr.base_qindex, hdr.filter_level, flags,
                                           hdr.mb_cols, hdr.mb_rows)


def vpxdec_config(args):
    """what the reference's vpxdec (vpxdec.c:779-857) makes of its post-processing options: ((post_proc_flag, deblocking_level,
    noise_level) handed to VP8_SET_POSTPROC -- the decoder's default when the flag word is 0 --, (ref_frame, mb_modes, b_modes, mvs)
    handed to the VP8_SET_DBG_* controls)"""
    flag, level, noise = 0, 0, 0
    dbg = [0, 0, 0, 0]
    names = ("--pp-dbg-ref-frame=", "--pp-dbg-mb-modes=", "--pp-dbg-b-modes=", "--pp-dbg-mvs=")
    for a in args:
        if a == "--deblock":
            flag |= 1
        elif a == "--mfqe":
            flag |= 1024
        elif a.startswith("--demacroblock-level="):
            flag |= 2
            level = int(a.split("=")[1])
        elif a.startswith("--noise-level="):
            flag |= 4
            noise = int(a.split("=")[1])
        elif a.startswith("--pp-debug-info="):
            flag &= ~7
            flag |= int(a.split("=")[1])
        else:
            k = [i for i, n in enumerate(names) if a.startswith(n)]
            assert k, a
            v = int(a.split("=")[1])
            if v:
                dbg[k[0]] = v
    if not flag:
        flag, level, noise = 1 | 2 | 1024, 4, 0          # vp8_dx_iface.c:421-431
    return (flag, level, noise), tuple(dbg)


def flags_word(post_proc_flag, dbg):
    """vp8_dx_iface.c:446-465: the configured flags and a debug bit for every nonzero VP8_SET_DBG_* value"""
    ref, mb, b, mv = dbg
    return (post_proc_flag | (CLR_FRM_REF_BLKS if ref else 0) | (CLR_BLK_MODES if mb or b else 0) | (DRAW_MV if mv else 0))


def _blit_text(buf, off, stride, text):
    glyphs = tables()["glyphs"]
    for i, ch in enumerate(text.encode("latin-1")):
        bits = glyphs[ch]
        for r in range(5):
            for c in range(7):
                p = off + 7 * i + r * stride + c
                if 0 <= p < buf.size:
                    buf[p] = 255 if (bits >> (r * 7 + c)) & 1 else 0


def _cdiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def constrain_line(x0, x1, y0, y1, width, height):
    """the far end of a line clipped to 0..width, 0..height (both inclusive), one side after the other"""
    if x1 > width:
        dx, dy = x1 - x0, y1 - y0
        x1 = width
        if dx:
            y1 = _cdiv((width - x0) * dy, dx) + y0
    if x1 < 0:
        dx, dy = x1 - x0, y1 - y0
        x1 = 0
        if dx:
            y1 = _cdiv((0 - x0) * dy, dx) + y0
    if y1 > height:
        dx, dy = x1 - x0, y1 - y0
        y1 = height
        if dy:
            x1 = _cdiv((height - y0) * dx, dy) + x0
    if y1 < 0:
        dx, dy = x1 - x0, y1 - y0
        y1 = 0
        if dy:
            x1 = _cdiv((0 - y0) * dx, dy) + x0
    return x1, y1


def line_points(x0, x1, y0, y1):
    """Bresenham from (x0, y0) to (x1, y1): one point per step along the longer axis, ends included"""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    dx, dy = x1 - x0, abs(y1 - y0)
    err, y = dx // 2, y0
    ystep = 1 if y0 < y1 else -1
    pts = []
    for x in range(x0, x1 + 1):
        pts.append((y, x) if steep else (x, y))
        err -= dy
        if err < 0:
            y += ystep
            err += dx
    return pts


def _line(buf, g, x0, x1, y0, y1):
    for x, y in line_points(x0, x1, y0, y1):
        p = g.y_off + x + y * g.y_stride
        if 0 <= p < buf.size:
            buf[p] ^= 255


def _blend(buf, off, stride, rows, cols, colour):
    idx = off + np.add.outer(np.asarray(rows) * stride, np.asarray(cols))
    buf[idx] = (buf[idx].astype(np.int64) * ALPHA + colour * (0x10000 - ALPHA)) >> 16


def mv_lines(mode, partitioning, mvs16, x0, y0):
    """the lines one macroblock draws (postproc.c:1111-1249), before clipping, in order: [(kind, x0, y0, x1, y1)].  kind 'clip':
    clipped to the picture; 'pair': the 16x16 case's two lines a row above and below the centre, the second clipped from where the
    first one's clipping left the far end; 'plain': a horizontal or vertical 16x16 vector, drawn as it is."""
    def end(sx, sy, mv):
        return sx + (int(mv[1]) >> 3), sy + (int(mv[0]) >> 3)
    out = []
    if mode == SPLITMV:
        starts = {0: [(8, 4), (8, 12)], 1: [(4, 8), (12, 8)], 2: [(4, 4), (12, 4), (4, 12), (12, 12)]}
        if partitioning in starts:
            # every line of these three takes block 0's vector: the reference moves its block pointer and not the vector's
            for sx, sy in starts[partitioning]:
                out.append(("clip", x0 + sx, y0 + sy) + end(x0 + sx, y0 + sy, mvs16[0]))
        else:
            for k in range(16):
                sx, sy = x0 + (k % 4) * 4 + 2, y0 + (k // 4) * 4 + 2
                out.append(("clip", sx, sy) + end(sx, sy, mvs16[k]))
    elif mode >= NEARESTMV:
        lx0, ly0 = x0 + 8, y0 + 8
        x1, y1 = end(lx0, ly0, mvs16[0])
        out.append(("pair" if (x1 != lx0 and y1 != ly0) else "plain", lx0, ly0, x1, y1))
    return out


def visualize(buf, g, hdr, mbs, mvs, flags, dbg, info=None, rate=RATE_INFO):
    """Draw the overlays the flags word asks for onto frame buffer `buf` (uint8, vp8ir_geom layout) in place.  mbs: the dense
    descriptors (uint8 [nmb, 64], vp8ir_mb), mvs: int16 [nmb, 16, 2] (row, col) -- read for inter frames only.  dbg: the four
    VP8_SET_DBG_* values (ref_frame, mb_modes, b_modes, mvs).  info: the frame-info string (default: formatted from hdr)."""
    ref_mask, mb_mask, b_mask, mv_mask = dbg
    T = tables()
    W, H, ys, uvs = g.aligned_w, g.aligned_h, g.y_stride, g.uv_stride
    cols, rows = W // 16, H // 16
    inter = hdr.frame_type != 0
    if flags & TXT_FRAME_INFO:
        _blit_text(buf, g.y_off, ys, frame_info(hdr, flags) if info is None else info)
    if flags & (TXT_MBLK_MODES | TXT_DC_DIFF):
        for kind in (TXT_MBLK_MODES, TXT_DC_DIFF):
            if not flags & kind:
                continue
            for i in range(rows * cols):
                m = mbs[i]
                if kind == TXT_MBLK_MODES:
                    ch = chr(m[0] + ord("a"))
                elif not inter:
                    ch = "a"
                else:
                    ch = "0" if (m[0] != B_PRED and m[0] != SPLITMV and (m[3] & 1)) else "1"
                _blit_text(buf, g.y_off + (16 * (i // cols) + 4) * ys + 16 * (i % cols) + 4, ys, ch)
    if flags & TXT_RATE_INFO:
        _blit_text(buf, g.y_off, ys, rate)
    if (flags & DRAW_MV) and mv_mask and inter:
        for i in range(rows * cols):
            mode = int(mbs[i][0])
            if not mv_mask & (1 << mode):
                continue
            x0, y0 = 16 * (i % cols), 16 * (i // cols)
            for kind, sx, sy, x1, y1 in mv_lines(mode, int(mbs[i][5]), mvs[i], x0, y0):
                if kind == "clip":
                    x1, y1 = constrain_line(sx, x1, sy, y1, W, H)
                    _line(buf, g, sx, x1, sy, y1)
                elif kind == "pair":
                    x1, y1 = constrain_line(sx, x1, sy - 1, y1, W, H)
                    _line(buf, g, sx, x1, sy - 1, y1)
                    x1, y1 = constrain_line(sx, x1, sy + 1, y1, W, H)
                    _line(buf, g, sx, x1, sy + 1, y1)
                else:
                    _line(buf, g, sx, x1, sy, y1)
    if (flags & CLR_BLK_MODES) and (mb_mask or b_mask):
        for i in range(rows * cols):
            m = mbs[i]
            mode = int(m[0])
            x0, y0 = 16 * (i % cols), 16 * (i // cols)
            yo, uo, vo = g.y_off + y0 * ys + x0, g.u_off + (y0 // 2) * uvs + x0 // 2, g.v_off + (y0 // 2) * uvs + x0 // 2
            if mode == B_PRED and ((mb_mask & B_PRED) or b_mask):       # (the value 4, not 1 << B_PRED)
                if (b_mask & (1 << mode)) or (mb_mask & B_PRED):
                    for k in range(16):
                        by, bx = (k // 4) * 4, (k % 4) * 4
                        Y, U, V = T["b_mode_colours"][int(m[40 + k])]
                        _blend(buf, yo + by * ys + bx, ys, range(4), range(4), Y)
                        _blend(buf, uo + (by // 2) * uvs + bx // 2, uvs, range(2), range(2), U)
                        _blend(buf, vo + (by // 2) * uvs + bx // 2, uvs, range(2), range(2), V)
            elif mb_mask & (1 << mode):
                Y, U, V = T["mb_mode_colours"][mode]
                _blend(buf, yo, ys, range(2, 14), range(2, 14), Y)
                _blend(buf, uo, uvs, range(1, 7), range(1, 7), U)
                _blend(buf, vo, uvs, range(1, 7), range(1, 7), V)
    if (flags & CLR_FRM_REF_BLKS) and ref_mask:
        for i in range(rows * cols):
            rf = int(mbs[i][2])
            if not ref_mask & (1 << rf):
                continue
            x0, y0 = 16 * (i % cols), 16 * (i // cols)
            yo, uo, vo = g.y_off + y0 * ys + x0, g.u_off + (y0 // 2) * uvs + x0 // 2, g.v_off + (y0 // 2) * uvs + x0 // 2
            Y, U, V = T["ref_frame_colours"][rf]
            _blend(buf, yo, ys, (0, 1, 14, 15), range(16), Y)
            _blend(buf, yo, ys, range(2, 14), (0, 1, 14, 15), Y)
            for off, c in ((uo, U), (vo, V)):
                _blend(buf, off, uvs, (0, 7), range(8), c)
                _blend(buf, off, uvs, range(1, 7), (0, 7), c)
    return buf
