"""The definition of vp8hip_frames_quant_async and vp8hip_quant_factors (include/vp8hip.h) a second time, in numpy: the prediction of a
16x16 vector (luma as the temporal filter's, chroma by the decoder's rule), the residual, the forward DCT and Walsh transform, the two
quantisers with their tables, the error figures, and the reconstruction through the inverse transforms.  Every `short` the
reference stores goes through fit(), which asserts that the value is an int16 already: nothing here wraps except the two places
the definition says do (the zero-bin extra's `(short)`; the chroma vector does NOT wrap).  Nothing here knows how the kernel goes
about it.  Also the generator of the pictures and vectors the fixture tests/golden/quant_ref.json was recorded for."""
import numpy as np

import tfilter_reference as TR
from residual_reference import AC_Q, DC_Q, idct, inv_walsh, s16

QUANTIZERS = ("regular", "fast")
STAGES = {"dequant": 0, "levels": 1}                      # VP8HIP_COEF_DEQUANT, VP8HIP_COEF_LEVELS
STATS = {"erry": 1, "erry2": 2, "erruv": 4, "eobs": 8, "recsse": 16}
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)
ZBIN_BOOST = (0, 0, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 44, 44, 44)
ZBIN_TERM_MAX = 1 << 20                                   # |zbin_over_quant|, |zbin_mode_boost|, |act_zbin_adj| at most
Y1, Y2, UV = 0, 1, 2                                      # the three tables
BLOCK_TABLE = np.array([Y1] * 16 + [UV] * 8 + [Y2])       # of block 0..24
FIELDS = ("quant", "quant_shift", "quant_fast", "zbin", "round", "dequant")


def fit(x):
    """an int16 store: the value must be one already"""
    x = np.asarray(x, np.int64)
    assert x.size == 0 or (-32768 <= int(x.min()) and int(x.max()) <= 32767), (int(x.min()), int(x.max()))
    return x


def chroma_mv(c):
    """a luma vector component -> the chroma one: (c + (c < 0 ? -1 : 1)) / 2, C's truncating division, in int"""
    c = int(c)
    s = c + (-1 if c < 0 else 1)
    return -((-s) // 2) if s < 0 else s // 2


def quant_factors(q, deltas=(0, 0, 0, 0, 0)):
    """vp8cx_init_quantizer with improved_quant for one qindex: {field: int64 [3, 2] (Y1, Y2, UV; dc, ac)} plus
    "zrun_zbin_boost": int64 [3, 16].  deltas: y1dc, y2dc, y2ac, uvdc, uvac"""
    q = int(q)
    y1dc, y2dc, y2ac, uvdc, uvac = (int(d) for d in deltas)
    assert 0 <= q <= 127 and all(-15 <= d <= 15 for d in (y1dc, y2dc, y2ac, uvdc, uvac))

    def qi(v):
        return min(max(v, 0), 127)
    d = np.array([[DC_Q[qi(q + y1dc)], AC_Q[q]],
                  [DC_Q[qi(q + y2dc)] * 2, max(AC_Q[qi(q + y2ac)] * 155 // 100, 8)],
                  [min(DC_Q[qi(q + uvdc)], 132), AC_Q[qi(q + uvac)]]], np.int64)
    zf = 84 if q < 48 else 80                             # qzbin_factors; qrounding_factors is 48 throughout
    out = {k: np.zeros((3, 2), np.int64) for k in FIELDS}
    for t in range(3):
        for k in range(2):
            v = int(d[t][k])
            sh = v.bit_length() - 1                       # invert_quant
            out["quant"][t][k] = int(fit(1 + (1 << (16 + sh)) // v - (1 << 16)))
            out["quant_shift"][t][k] = sh
            out["quant_fast"][t][k] = int(fit((1 << 16) // v))
            out["zbin"][t][k] = (zf * v + 64) >> 7
            out["round"][t][k] = (48 * v) >> 7
            out["dequant"][t][k] = v
    out["zrun_zbin_boost"] = np.array([[(int(d[t][0 if i == 0 else 1]) * ZBIN_BOOST[i]) >> 7 for i in range(16)] for t in range(3)], np.int64)
    return out


def factors_flat(q, deltas=(0, 0, 0, 0, 0)):
    """the table as vp8hip_quant_factors lays it out: int16 [84] -- the six fields [3][2] in FIELDS' order, then the boosts [3][16]"""
    f = quant_factors(q, deltas)
    return np.concatenate([f[k].ravel() for k in FIELDS] + [f["zrun_zbin_boost"].ravel()]).astype(np.int16)


def zbin_extra(f, over_quant=0, mode_boost=0, act_adj=0):
    """ZBIN_EXTRA_Y, _Y2, _UV -> int64 [3] in the tables' order, each through the reference's `(short)`"""
    o, m, a = int(over_quant), int(mode_boost), int(act_adj)
    assert all(abs(v) <= ZBIN_TERM_MAX for v in (o, m, a))
    half = -((-o) // 2) if o < 0 else o // 2              # C's zbin_over_quant / 2
    ac = f["dequant"][:, 1]
    return s16(np.array([(int(ac[Y1]) * (o + m + a)) >> 7, (int(ac[Y2]) * (half + m + a)) >> 7, (int(ac[UV]) * (o + m + a)) >> 7]))


def fdct(d):
    """vp8_short_fdct4x4_c on blocks [..., 4, 4] (row, col) of residual -> [..., 4, 4] (v, u): position 4 v + u"""
    d = np.asarray(d, np.int64)
    a, b, c, e = (d[..., 0] + d[..., 3]) << 3, (d[..., 1] + d[..., 2]) << 3, (d[..., 1] - d[..., 2]) << 3, (d[..., 0] - d[..., 3]) << 3
    t = fit(np.stack([a + b, (c * 2217 + e * 5352 + 14500) >> 12, a - b, (e * 2217 - c * 5352 + 7500) >> 12], -1))
    a, b, c, e = t[..., 0, :] + t[..., 3, :], t[..., 1, :] + t[..., 2, :], t[..., 1, :] - t[..., 2, :], t[..., 0, :] - t[..., 3, :]
    return fit(np.stack([(a + b + 7) >> 4, ((c * 2217 + e * 5352 + 12000) >> 16) + (e != 0), (a - b + 7) >> 4,
                         (e * 2217 - c * 5352 + 51000) >> 16], -2))


def walsh(d):
    """vp8_short_walsh4x4_c on the luma DCs [..., 4, 4] (block row, block column) -> [..., 4, 4] (v, u)"""
    d = np.asarray(d, np.int64)
    a, e, c, b = (d[..., 0] + d[..., 2]) << 2, (d[..., 1] + d[..., 3]) << 2, (d[..., 1] - d[..., 3]) << 2, (d[..., 0] - d[..., 2]) << 2
    t = fit(np.stack([a + e + (a != 0), b + c, b - c, a - e], -1))
    a, e, c, b = t[..., 0, :] + t[..., 2, :], t[..., 1, :] + t[..., 3, :], t[..., 1, :] - t[..., 3, :], t[..., 0, :] - t[..., 2, :]
    out = []
    for x in (a + e, b + c, b - c, a - e):
        x = x + (x < 0)
        out.append((x + 3) >> 3)
    return fit(np.stack(out, -2))


def quantise(coef, f, extra, quantizer):
    """coef: int64 [n, 25, 16] (position 4 v + u) -> (qcoeff, dqcoeff [n, 25, 16], eob [n, 25])"""
    assert quantizer in QUANTIZERS
    n = coef.shape[0]
    ac = (np.arange(16) != 0).astype(np.int64)
    tab = {k: f[k][BLOCK_TABLE][:, ac] for k in FIELDS}                # [25, 16]
    boost = f["zrun_zbin_boost"][BLOCK_TABLE]                            # [25, 16]
    ext = np.asarray(extra, np.int64)[BLOCK_TABLE]                       # [25]
    q, dq = np.zeros((n, 25, 16), np.int64), np.zeros((n, 25, 16), np.int64)
    eob, run = np.zeros((n, 25), np.int64), np.zeros((n, 25), np.int64)
    blk = np.arange(25)[None, :]
    for i, rc in enumerate(ZIGZAG):
        z = coef[:, :, rc]
        x = np.abs(z)
        if quantizer == "fast":
            y = ((x + tab["round"][:, rc]) * tab["quant_fast"][:, rc]) >> 16
        else:
            zbin = tab["zbin"][:, rc] + boost[blk, run] + ext
            xr = x + tab["round"][:, rc]
            y = np.where(x >= zbin, (((xr * tab["quant"][:, rc]) >> 16) + xr) >> tab["quant_shift"][:, rc], 0)
            run = np.where(y != 0, 0, run + 1)
        level = np.where(z < 0, -y, y)
        q[:, :, rc] = fit(level)
        dq[:, :, rc] = fit(level * tab["dequant"][:, rc])
        eob = np.where(y != 0, i + 1, eob)
    return q, dq, eob


def predict_mb(ref, my, mx, vx, vy, filt):
    """vp8_build_inter16x16_predictors_mb without the clamp: the three predictions of macroblock (my, mx) from the coded planes ref"""
    cx, cy = chroma_mv(vx), chroma_mv(vy)
    return [TR.predict(ref[0], 16 * my, 16 * mx, vy, vx, 16, filt), TR.predict(ref[1], 8 * my, 8 * mx, cy, cx, 8, filt),
            TR.predict(ref[2], 8 * my, 8 * mx, cy, cx, 8, filt)]


def _blocks(p, g):
    """a plane block [4 g, 4 g] -> its g * g 4x4 blocks [g * g, 4, 4] in raster order"""
    return p.reshape(g, 4, g, 4).transpose(0, 2, 1, 3).reshape(g * g, 4, 4)


def _unblocks(b, g):
    return b.reshape(g, g, 4, 4).transpose(0, 2, 1, 3).reshape(4 * g, 4 * g)


def quant_planes(src, ref, mv=None, qindex=40, deltas=(0, 0, 0, 0, 0), quantizer="regular", filt="sixtap", zbin=(0, 0, 0)):
    """src, ref: the coded planes (y, u, v) of the source and of the reference picture; mv: None or integers [2, rows, cols] (x, y)
    in 1/8 pel; zbin: (zbin_over_quant, zbin_mode_boost, act_zbin_adj) -> a dict: "levels", "dequant" int16 [rows, cols, 25, 16];
    "eob" uint8 [rows, cols, 32]; "stats" {name: uint32 [rows, cols]}; "pred", "rec": coded planes uint8"""
    assert filt in TR.FILTERS
    rows, cols = src[0].shape[0] // 16, src[0].shape[1] // 16
    n = rows * cols
    f = quant_factors(qindex, deltas)
    extra = zbin_extra(f, *zbin)
    pred = [np.zeros(p.shape, np.int64) for p in src]
    for my in range(rows):
        for mx in range(cols):
            vx, vy = (0, 0) if mv is None else (int(mv[0][my][mx]), int(mv[1][my][mx]))
            for pl, p in enumerate(predict_mb(ref, my, mx, vx, vy, filt)):
                s = 8 if pl else 16
                pred[pl][s * my:s * my + s, s * mx:s * mx + s] = p
    # the residual (vp8_subtract_mby_c, _mbuv_c) of every block: [n, 24, 4, 4]
    diff = [fit(s.astype(np.int64) - p) for s, p in zip(src, pred)]
    res = np.zeros((n, 24, 4, 4), np.int64)
    for my in range(rows):
        for mx in range(cols):
            m = my * cols + mx
            res[m, :16] = _blocks(diff[0][16 * my:16 * my + 16, 16 * mx:16 * mx + 16], 4)
            res[m, 16:20] = _blocks(diff[1][8 * my:8 * my + 8, 8 * mx:8 * mx + 8], 2)
            res[m, 20:24] = _blocks(diff[2][8 * my:8 * my + 8, 8 * mx:8 * mx + 8], 2)
    coef = np.zeros((n, 25, 4, 4), np.int64)
    coef[:, :24] = fdct(res)
    coef[:, 24] = walsh(coef[:, :16, 0, 0].reshape(n, 4, 4))            # build_dcblock: the luma blocks keep their own coefficient 0
    coef = coef.reshape(n, 25, 16)
    q, dq, eob = quantise(coef, f, extra, quantizer)
    err = (coef - dq) ** 2
    stats = {"erry": err[:, :16, 1:].sum(axis=(1, 2)), "erry2": err[:, 24].sum(axis=1), "erruv": err[:, 16:24].sum(axis=(1, 2)),
             "eobs": eob.sum(axis=1)}
    # the reconstruction: vp8_inverse_transform_mby, then vp8_dequant_idct_add_y_block / _uv_block on the prediction
    wht = inv_walsh(dq[:, 24].reshape(n, 4, 4), fit).reshape(n, 16)
    a1 = fit((dq[:, 24, 0] + 3) >> 3)
    y2dc = np.where((eob[:, 24] > 1)[:, None], wht, a1[:, None])        # position 0 of the sixteen luma blocks
    e = eob[:, :24].copy()
    e[:, :16] = np.where((e[:, :16] == 0) & (y2dc != 0), 1, e[:, :16])  # eob_adjust
    blk = q[:, :24].reshape(n, 24, 4, 4).copy()
    blk[:, :16, 0, 0] = y2dc
    fac = np.zeros((24, 4, 4), np.int64)
    fac[:16], fac[16:] = f["dequant"][Y1][1], f["dequant"][UV][1]
    fac[:16, 0, 0], fac[16:, 0, 0] = 1, f["dequant"][UV][0]
    full = idct(fit(blk * fac), fit)
    dc = fit((fit(blk[:, :, 0, 0] * fac[:, 0, 0]) + 4) >> 3)
    add = np.where((e > 1)[:, :, None, None], full, dc[:, :, None, None])
    rec = [np.zeros(p.shape, np.int64) for p in src]
    for my in range(rows):
        for mx in range(cols):
            m = my * cols + mx
            rec[0][16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = _unblocks(add[m, :16], 4)
            rec[1][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = _unblocks(add[m, 16:20], 2)
            rec[2][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = _unblocks(add[m, 20:24], 2)
    rec = [np.clip(r + p, 0, 255) for r, p in zip(rec, pred)]
    sse = np.zeros((rows, cols), np.int64)
    for pl in range(3):
        s = 8 if pl else 16
        d2 = (src[pl].astype(np.int64) - rec[pl]) ** 2
        sse += d2.reshape(rows, s, cols, s).sum(axis=(1, 3))
    stats["recsse"] = sse.ravel()
    eob32 = np.zeros((n, 32), np.uint8)
    eob32[:, :25] = eob
    return {"levels": q.astype(np.int16).reshape(rows, cols, 25, 16), "dequant": dq.astype(np.int16).reshape(rows, cols, 25, 16),
            "eob": eob32.reshape(rows, cols, 32), "stats": {k: v.astype(np.uint32).reshape(rows, cols) for k, v in stats.items()},
            "pred": [p.astype(np.uint8) for p in pred], "rec": [r.astype(np.uint8) for r in rec], "coef": coef.reshape(rows, cols, 25, 16)}


def stats_tensor(out, planes):
    """the stats of quant_planes' result as the call lays them out: uint32 [popcount, rows, cols] in bit order"""
    mask = planes if isinstance(planes, int) else sum({STATS[p] for p in planes})
    return np.stack([out["stats"][k] for k, bit in STATS.items() if mask & bit])


# ---- the pictures and vectors of the fixture ----------------------------------------------------------------------------------------
CONTENTS = ("decoded", "noise", "flat", "flatluma")


def pictures(kind, w, h, seed, k=1):
    """-> (source planes, reference planes) of the coded size w x h: "decoded": a smooth picture and a noisy, moved neighbour
    (tfilter_reference.sequence's source k); "noise": two unrelated noise pictures; "flat": flat 97 against flat 90; "flatluma": luma
    flat 98 against flat 90, chroma 90 in both"""
    if kind == "decoded":
        centre, sources = TR.sequence(w, h, seed, k + 1)
        return centre, sources[k]
    if kind == "noise":
        return TR.picture("noise", w, h, seed), TR.picture("noise", w, h, seed + 50)
    if kind == "flatluma":
        return [TR.picture("flat98", w, h, 0)[0]] + TR.picture("flat90", w, h, 0)[1:], TR.picture("flat90", w, h, 0)
    assert kind == "flat"
    return TR.picture("flat97", w, h, 0), TR.picture("flat90", w, h, 0)
