"""libyuv's I420Scale (third_party/libyuv/source/scale.c:3762, version 102, its C rows: YUV_DISABLE_ASM) restated in numpy from
what it computes, for the tests: the checker of vp8hip_frames_scale_async on sizes no listing covers.

A plane is read from a frame buffer of the vp8ir_geom layout (include/vp8_ir.h): its decoded, 16-aligned area, with every
coordinate clamped to it.  For a decoded frame that is what the reference's bordered buffer gives for every read I420Scale makes
(Down38 reads up to three rows below the picture, the 16-bit bilinear path of a one-pixel-wide plane reads column 1); the
listings tests/golden/*.scale_*.md5 that the reference's own scaler wrote pin it (tests/test_scale_cpu.py)."""
import numpy as np

# ScalePlane's dispatch (scale.c:3702), one plane at a time
COPY, DOWN2, DOWN4, DOWN8, DOWN34, DOWN38, POINT, BILIN8, BILIN16 = range(9)
NAMES = ("copy", "down2", "down4", "down8", "down34", "down38", "point", "bilinear8", "bilinear16")
MAX_INPUT_WIDTH = 2560      # kMaxInputWidth (scale.c:2920): the 8-bit bilinear rows take planes up to this width
MAX_OUTPUT_WIDTH = 640      # kMaxOutputWidth (scale.c:2794): Down8 filters up to this output width


def plane_path(sw, sh, dw, dh, filt):
    """(path, filtered) of ScalePlane for a sw x sh plane scaled to dw x dh with FilterMode filt"""
    f = filt != 0
    if dw == sw and dh == sh:
        return COPY, False
    if dw <= sw and dh <= sh:
        if 4 * dw == 3 * sw and 4 * dh == 3 * sh:
            return DOWN34, f
        if 2 * dw == sw and 2 * dh == sh:
            return DOWN2, f
        if 8 * dw == 3 * sw and dh == (sh * 3 + 7) // 8:
            return DOWN38, f
        if 4 * dw == sw and 4 * dh == sh:
            return DOWN4, f
        if 8 * dw == sw and 8 * dh == sh:
            return DOWN8, f and dw <= MAX_OUTPUT_WIDTH
    # ScalePlaneDown / ScalePlaneAnySize: kFilterBox is bilinear here (src_height * 2 > dst_height holds for every downscale)
    if not f:
        return POINT, False
    if sw % 8 == 0 and sw <= MAX_INPUT_WIDTH:
        return BILIN8, True
    return BILIN16, True


def plan(w, h, dw, dh, filt):
    """(luma path, chroma path) names: chroma is dispatched on its own sizes, (v + 1) >> 1 on both sides"""
    c = lambda v: (v + 1) >> 1
    return NAMES[plane_path(w, h, dw, dh, filt)[0]], NAMES[plane_path(c(w), c(h), c(dw), c(dh), filt)[0]]


def _sampler(src):
    ah, aw = src.shape
    s = src.astype(np.int64)

    def at(x, y):
        return s[np.clip(y, 0, ah - 1), np.clip(x, 0, aw - 1)]
    return at


def scale_plane(src, sw, sh, dw, dh, filt):
    """src: the plane's aligned area (rows x columns, uint8).  Returns dh x dw uint8."""
    path, f = plane_path(sw, sh, dw, dh, filt)
    at = _sampler(src)
    ox = np.arange(dw, dtype=np.int64)[None, :]
    oy = np.arange(dh, dtype=np.int64)[:, None]
    if path == COPY:
        out = at(ox, oy)
    elif path in (DOWN2, DOWN4):
        k = 2 if path == DOWN2 else 4
        if not f:
            out = at(k * ox, k * oy)
        else:
            acc = sum(at(k * ox + i, k * oy + j) for i in range(k) for j in range(k))
            out = (acc + k * k // 2) >> (2 if k == 2 else 4)
    elif path == DOWN8:
        if not f:
            out = at(8 * ox, 8 * oy)
        else:
            # ScaleRowDown8Int_C: two Down4Int rows (rounded) into one buffer, the second at [640], then Down2Int over them with a
            # stride of 640 (rounded again).  Past 320 output pixels the second row overwrites the first one's tail: element
            # i >= 640 of the "upper" row is element i - 640 of the lower one.
            def box4(x4, y4):
                return (sum(at(4 * x4 + i, y4 + j) for i in range(4) for j in range(4)) + 8) >> 4

            def upper(i):
                return np.where(i < MAX_OUTPUT_WIDTH, box4(i, 8 * oy), box4(i - MAX_OUTPUT_WIDTH, 8 * oy + 4))
            out = (upper(2 * ox) + upper(2 * ox + 1) + box4(2 * ox, 8 * oy + 4) + box4(2 * ox + 1, 8 * oy + 4) + 2) >> 2
    elif path == DOWN34:
        c, j = ox // 3, ox % 3
        g, k = oy // 3, oy % 3
        if not f:
            out = at(4 * c + np.array([0, 1, 3])[j], 4 * g + np.array([0, 1, 3])[k])
        else:
            def hrow(y):         # the horizontal 4 -> 3 of ScaleRowDown34_*_Int_C, rounded
                s0, s1, s2, s3 = (at(4 * c + i, y) for i in range(4))
                return np.where(j == 0, (s0 * 3 + s1 + 2) >> 2, np.where(j == 1, (s1 + s2 + 1) >> 1, (s2 + s3 * 3 + 2) >> 2))
            r0, r1, r2, r3 = (hrow(4 * g + i) for i in range(4))
            # the third row of a group: ScaleRowDown34_0 from row 3 with a negative stride (scale.c:3250) -> rows 3 and 2, 3 : 1
            out = np.where(k == 0, (r0 * 3 + r1 + 2) >> 2, np.where(k == 1, (r1 + r2 + 1) >> 1, (r3 * 3 + r2 + 2) >> 2))
    elif path == DOWN38:
        c, j = ox // 3, ox % 3
        g, k = oy // 3, oy % 3
        x0, y0 = 8 * c + 3 * j, 8 * g + 3 * k
        if not f:
            out = at(x0, y0)
        else:
            nc = np.where(j == 2, 2, 3)
            nr = np.where(k == 2, 2, 3)
            acc = np.zeros((dh, dw), np.int64)
            for jj in range(3):
                for ii in range(3):
                    acc += np.where((ii < nc) & (jj < nr), at(x0 + ii, y0 + jj), 0)
            out = (acc * (65536 // (nc * nr))) >> 16
    elif path == POINT:
        # ScalePlaneSimple: x from 0 in 16.16 steps, rows y * sh / dh
        dx = (sw << 16) // dw
        out = at((ox * dx) >> 16, oy * sh // dh)
    elif path == BILIN8:
        # ScalePlaneBilinear's rows: ScaleFilterRows_C with an 8-bit fraction, element [sw] duplicated from [sw - 1], then
        # ScaleFilterCols_C with 16-bit fractions from x = 0; y clamped to maxy after each step (the first row unclamped)
        dx, dy = (sw << 16) // dw, (sh << 16) // dh
        maxy = ((sh - 1) << 16) - 1
        y = np.where(oy == 0, 0, np.minimum(oy * dy, maxy))
        iy, fy = y >> 16, (y >> 8) & 255
        xs = np.arange(sw + 1, dtype=np.int64)[None, :]
        xr = np.minimum(xs, sw - 1)
        row = (at(xr, iy) * (256 - fy) + at(xr, iy + 1) * fy) >> 8          # dh x (sw + 1)
        x = ox * dx
        xi, xf = x >> 16, x & 0xffff
        xi_b = np.broadcast_to(xi, (dh, dw))
        a = np.take_along_axis(row, xi_b, axis=1)
        b = np.take_along_axis(row, xi_b + 1, axis=1)
        out = (a * (65536 - xf) + b * xf) >> 16
    else:
        # ScalePlaneBilinearSimple: 16-bit fractions both ways, a half-pixel start, maxx / maxy clamps after each step
        dx, dy = (sw << 16) // dw, (sh << 16) // dh
        maxx, maxy = ((sw - 1) << 16) - 1, ((sh - 1) << 16) - 1
        x0 = 32768 if dw < sw else (sw << 16) // dw - 32768
        y0 = 32768 if dh < sh else (sh << 16) // dh - 32768
        x = np.where(ox == 0, x0, np.minimum(x0 + ox * dx, maxx))
        y = np.where(oy == 0, y0, np.minimum(y0 + oy * dy, maxy))
        x, y = np.maximum(x, 0), np.maximum(y, 0)
        xi, xf = x >> 16, x & 0xffff
        yi, yf = y >> 16, y & 0xffff
        r0 = (at(xi, yi) * (65536 - xf) + at(xi + 1, yi) * xf) >> 16
        r1 = (at(xi, yi + 1) * (65536 - xf) + at(xi + 1, yi + 1) * xf) >> 16
        out = (r0 * (65536 - yf) + r1 * yf) >> 16
    return np.broadcast_to(out, (dh, dw)).astype(np.uint8)


def i420_size(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def planes(buf, g):
    """the three aligned areas of a frame buffer (views)"""
    out = []
    for off, stride, w, h in ((g.y_off, g.y_stride, g.aligned_w, g.aligned_h), (g.u_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2),
                              (g.v_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2)):
        out.append(np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w), strides=(stride, 1)))
    return out


def scale_frame(buf, g, w, h, dw, dh, filt):
    """I420Scale of the w x h picture in frame buffer `buf` to dw x dh: packed I420, i420_size(dw, dh) bytes"""
    c = lambda v: (v + 1) >> 1
    y, u, v = planes(buf, g)
    return np.concatenate([scale_plane(y, w, h, dw, dh, filt).ravel(), scale_plane(u, c(w), c(h), c(dw), c(dh), filt).ravel(),
                           scale_plane(v, c(w), c(h), c(dw), c(dh), filt).ravel()])
