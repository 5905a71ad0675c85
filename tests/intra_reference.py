"""The definition of vp8hip_frames_intra_async, vp8hip_intra_costs and vp8hip_intra_rd (include/vp8hip.h) a second time, in Python:
the reference's vp8_pick_intra_mode followed by the body of vp8cx_encode_intra_macro_block, per macroblock of a key frame in raster
order, on a bordered reconstruction seeded as vp8_setup_intra_recon seeds it and extended to the right as vp8_extend_mb_row does.
Every `short` the reference stores goes through an assert that the value is an int16 already.  Nothing here knows how the kernel
goes about it.  The transforms and the quantiser of the 16x16 and chroma paths are quant_reference's; the sub-block chain has its
own one-block forms in plain integers (test_intra_cpu.py holds the two against each other)."""
import numpy as np

import quant_reference as QR
from residual_reference import DC_Q, idct, inv_walsh

INT_MAX = 0x7FFFFFFF
DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED = range(5)       # vp8_ir.h's numbering
B_DC, B_TM, B_VE, B_HE, B_LD, B_RD, B_VR, B_VL, B_HD, B_HU = range(10)
IMPLIED_BMODE = {DC_PRED: B_DC, V_PRED: B_VE, H_PRED: B_HE, TM_PRED: B_TM}
STATS = {"rd16": 1, "rd4": 2, "rate": 4, "eobs": 8, "recsse": 16}       # VP8HIP_INTRA_*: bit order = plane order
NO_BPRED = 1                                               # VP8HIP_INTRA_NO_BPRED
KF_YMODE_PROB = (145, 156, 163, 128)                       # vp8_kf_ymode_prob
# vp8_kf_ymode_tree and vp8_bmode_tree as (bit, index of its probability) paths to each leaf
YMODE_CODE = {B_PRED: ((0, 0),), DC_PRED: ((1, 0), (0, 1), (0, 2)), V_PRED: ((1, 0), (0, 1), (1, 2)), H_PRED: ((1, 0), (1, 1), (0, 3)),
              TM_PRED: ((1, 0), (1, 1), (1, 3))}
BMODE_CODE = {
    0: ((0, 0),), 1: ((1, 0), (0, 1)), 2: ((1, 0), (1, 1), (0, 2)),
    3: ((1, 0), (1, 1), (1, 2), (0, 3), (0, 4)),
    5: ((1, 0), (1, 1), (1, 2), (0, 3), (1, 4), (0, 5)), 6: ((1, 0), (1, 1), (1, 2), (0, 3), (1, 4), (1, 5)),
    4: ((1, 0), (1, 1), (1, 2), (1, 3), (0, 6)),
    7: ((1, 0), (1, 1), (1, 2), (1, 3), (1, 6), (0, 7)),
    8: ((1, 0), (1, 1), (1, 2), (1, 3), (1, 6), (1, 7), (0, 8)), 9: ((1, 0), (1, 1), (1, 2), (1, 3), (1, 6), (1, 7), (1, 8)),
}


def _path_cost(path, probs, cost):
    """vp8_cost_tokens for one leaf: vp8_cost_bit along its path (vp8_cost_one(p) = vp8_cost_zero(255 - p))"""
    return sum(cost[255 - probs[i]] if bit else cost[probs[i]] for bit, i in path)


def intra_costs(prob_cost, kf_bmode_probs):
    """vp8_init_mode_costs for a key frame: (mbmode_cost [5] in vp8_ir.h's order, bmode_cost [10][10][10]), from vp8_prob_cost [256]
    and vp8_kf_bmode_prob [900]"""
    mb = np.array([_path_cost(YMODE_CODE[m], KF_YMODE_PROB, prob_cost) for m in range(5)], np.int64)
    b = np.zeros((10, 10, 10), np.int64)
    for a in range(10):
        for left in range(10):
            p = kf_bmode_probs[(a * 10 + left) * 9:(a * 10 + left) * 9 + 9]
            for m in range(10):
                b[a, left, m] = _path_cost(BMODE_CODE[m], p, prob_cost)
    return mb, b


def intra_rd(qindex, y1dc_delta=0, zbin_over_quant=0):
    """vp8_initialize_rd_consts for one pass: (rdmult, rddiv)"""
    q = float(min(int(DC_Q[min(max(int(qindex) + int(y1dc_delta), 0), 127)]), 160))
    rdmult = int(2.70 * (q * q))
    if zbin_over_quant > 0:
        modq = float(int(q * (1.0 + 0.0015625 * zbin_over_quant)))
        rdmult = int(2.70 * (modq * modq))
    if rdmult > 1000:
        return rdmult // 100, 1
    return rdmult, 100


def rdcost(rdmult, rddiv, rate, dist):
    v = ((128 + rate * rdmult) >> 8) + rddiv * dist
    assert 0 <= v <= INT_MAX
    return v


def _s16(v):
    assert -32768 <= v <= 32767, v
    return v


# ---- one 4x4 block in plain integers ------------------------------------------------------------------------------------------------
def F(i): return ("F", i)
def G(i): return ("G", i)


# a pixel of a directional mode over the edge vector P = {L3 L3 L2 L1 L0 TL A0 .. A7 A7}: F[k] = (P[k-1] + 2 P[k] + P[k+1] + 2) >> 2,
# G[k] = (P[k] + P[k+1] + 1) >> 1 (vp8_intra4x4_predict; the table of tools/gen_pred_sel.py, which test_pred_table_cpu.py holds to the oracle)
BMODE_PIXELS = {
    B_VE: [[F(6 + c) for c in range(4)] for r in range(4)],
    B_HE: [[F(4 - r)] * 4 for r in range(4)],
    B_LD: [[F(7 + r + c) for c in range(4)] for r in range(4)],
    B_RD: [[F(5 - r + c) for c in range(4)] for r in range(4)],
    B_VR: [[G(5), G(6), G(7), G(8)], [F(5), F(6), F(7), F(8)], [F(4), G(5), G(6), G(7)], [F(3), F(5), F(6), F(7)]],
    B_VL: [[G(6), G(7), G(8), G(9)], [F(7), F(8), F(9), F(10)], [G(7), G(8), G(9), F(11)], [F(8), F(9), F(10), F(12)]],
    B_HD: [[G(4), F(5), F(6), F(7)], [G(3), F(4), G(4), F(5)], [G(2), F(3), G(3), F(4)], [G(1), F(2), G(2), F(3)]],
    B_HU: [[G(3), F(3), G(2), F(2)], [G(2), F(2), G(1), F(1)], [G(1), F(1), G(0), G(0)], [G(0)] * 4],
}


def predict4(mode, above, left, tl):
    """vp8_intra4x4_predict: above [8] (the last four the above-right), left [4] top first, tl -> sixteen pixels, 4 row + column"""
    if mode == B_DC:
        return [(sum(above[:4]) + sum(left) + 4) >> 3] * 16
    if mode == B_TM:
        return [min(max(left[r] + above[c] - tl, 0), 255) for r in range(4) for c in range(4)]
    P = [left[3], left[3], left[2], left[1], left[0], tl] + list(above) + [above[7]]
    out = []
    for r in range(4):
        for c in range(4):
            kind, k = BMODE_PIXELS[mode][r][c]
            out.append((P[k - 1] + 2 * P[k] + P[k + 1] + 2) >> 2 if kind == "F" else (P[k] + P[k + 1] + 1) >> 1)
    return out


def fdct4(d):
    """vp8_short_fdct4x4_c: d [16], 4 row + column -> [16], 4 v + u"""
    t, o = [0] * 16, [0] * 16
    for r in range(4):
        a1, b1 = (d[4 * r] + d[4 * r + 3]) * 8, (d[4 * r + 1] + d[4 * r + 2]) * 8
        c1, d1 = (d[4 * r + 1] - d[4 * r + 2]) * 8, (d[4 * r] - d[4 * r + 3]) * 8
        t[4 * r], t[4 * r + 2] = _s16(a1 + b1), _s16(a1 - b1)
        t[4 * r + 1], t[4 * r + 3] = _s16((c1 * 2217 + d1 * 5352 + 14500) >> 12), _s16((d1 * 2217 - c1 * 5352 + 7500) >> 12)
    for c in range(4):
        a1, b1, c1, d1 = t[c] + t[12 + c], t[4 + c] + t[8 + c], t[4 + c] - t[8 + c], t[c] - t[12 + c]
        o[c], o[8 + c] = _s16((a1 + b1 + 7) >> 4), _s16((a1 - b1 + 7) >> 4)
        o[4 + c] = _s16(((c1 * 2217 + d1 * 5352 + 12000) >> 16) + (d1 != 0))
        o[12 + c] = _s16((d1 * 2217 - c1 * 5352 + 51000) >> 16)
    return o


def quant4(c, f, extra, ty, quantizer):
    """the quantiser over table ty on one block c [16] (4 v + u) -> (qcoeff, dqcoeff, eob)"""
    q, dq, eob, run = [0] * 16, [0] * 16, 0, 0
    for i, rc in enumerate(QR.ZIGZAG):
        k = 1 if rc else 0
        z = c[rc]
        x = abs(z)
        rnd = int(f["round"][ty][k])
        if quantizer == "fast":
            y = ((x + rnd) * int(f["quant_fast"][ty][k])) >> 16
        else:
            zbin = int(f["zbin"][ty][k]) + int(f["zrun_zbin_boost"][ty][run]) + int(extra[ty])
            y = ((((x + rnd) * int(f["quant"][ty][k])) >> 16) + x + rnd) >> int(f["quant_shift"][ty][k]) if x >= zbin else 0
            run = 0 if y else run + 1
        q[rc] = _s16(-y if z < 0 else y)
        dq[rc] = _s16(q[rc] * int(f["dequant"][ty][k]))
        if y:
            eob = i + 1
    return q, dq, eob


def _idct1(i0, i1, i2, i3):
    a, b = i0 + i2, i0 - i2
    c = ((i1 * 35468) >> 16) - (i3 + ((i3 * 20091) >> 16))
    d = (i1 + ((i1 * 20091) >> 16)) + ((i3 * 35468) >> 16)
    return a + d, b + c, b - c, a - d


def idct4(dq):
    """vp8_short_idct4x4llm_c without the predictor: dq [16], 4 v + u -> what it adds [16], 4 row + column"""
    t, o = [0] * 16, [0] * 16
    for u in range(4):
        for v, x in enumerate(_idct1(dq[u], dq[4 + u], dq[8 + u], dq[12 + u])):
            t[4 * v + u] = _s16(x)
    for v in range(4):
        for u, x in enumerate(_idct1(t[4 * v], t[4 * v + 1], t[4 * v + 2], t[4 * v + 3])):
            o[4 * v + u] = _s16((x + 4) >> 3)
    return o


# ---- whole-block predictors (the decoder's vp8_build_intra_predictors_mby_s / _mbuv_s) ---------------------------------------------
def predict_block(mode, above, left, tl, up, lf, n):
    """above, left: int64 [n]; up / lf: the macroblock has one above / to its left (the DC rule only) -> int64 [n, n]"""
    if mode == DC_PRED:
        shift = (3 if n == 16 else 2) + up + lf
        dc = 128 if not (up or lf) else ((int(above.sum()) if up else 0) + (int(left.sum()) if lf else 0) + (1 << (shift - 1))) >> shift
        return np.full((n, n), dc, np.int64)
    if mode == V_PRED:
        return np.repeat(above[None, :], n, 0)
    if mode == H_PRED:
        return np.repeat(left[:, None], n, 1)
    return np.clip(left[:, None] + above[None, :] - tl, 0, 255)


def intra_planes(src, qindex=40, deltas=(0, 0, 0, 0, 0), quantizer="regular", zbin=(0, 0, 0), rdmult=300, rddiv=1, mbmode_cost=None,
                 bmode_cost=None, bmode_last=3, flags=0):
    """src: the coded planes (y, u, v), uint8 -> a dict: "levels", "dequant" int16 [rows, cols, 25, 16]; "eob" uint8 [rows, cols, 32];
    "modes" uint8 [rows, cols, 32]; "stats" {name: uint32 [rows, cols]}; "rec": coded planes uint8; "seen": what the cases met (the
    sub-block modes tried and chosen, break-outs, ...) for the tests that assert no path goes untested"""
    assert quantizer in QR.QUANTIZERS and 0 <= bmode_last <= 9 and 0 <= rdmult <= 1000 and 1 <= rddiv <= 100
    mbmode_cost = [int(v) for v in mbmode_cost]
    bmode_cost = np.asarray(bmode_cost, np.int64).reshape(10, 10, 10)
    assert all(0 <= v <= 65535 for v in mbmode_cost) and 0 <= bmode_cost.min() and bmode_cost.max() <= 65535
    B, A = src[0].shape
    rows, cols = B // 16, A // 16
    f = QR.quant_factors(qindex, deltas)
    extra = QR.zbin_extra(f, *zbin)
    # the bordered reconstruction: row 0 and column 0 are the border (127 above, 129 to the left), four more columns to the right
    Y = np.zeros((B + 1, A + 5), np.int64)
    U, V = np.zeros((B // 2 + 1, A // 2 + 1), np.int64), np.zeros((B // 2 + 1, A // 2 + 1), np.int64)
    for p in (Y, U, V):
        p[1:, 0] = 129
        p[0, :] = 127
    sy, su, sv = (np.asarray(p, np.int64) for p in src)
    levels, dequant = np.zeros((rows, cols, 25, 16), np.int64), np.zeros((rows, cols, 25, 16), np.int64)
    eobs, modes = np.zeros((rows, cols, 32), np.uint8), np.zeros((rows, cols, 32), np.uint8)
    stats = {k: np.zeros((rows, cols), np.int64) for k in STATS}
    seen = {"tried": set(), "bmodes": set(), "breakout": 0, "bpred_eob_le1": 0, "bpred_eob_gt1": 0, "y2_eob_le1": 0, "y2_eob_gt1": 0,
            "skippable": 0, "last_col_bpred": 0}

    def bmode_of(r, c, b):                       # the context a neighbour macroblock gives
        if r < 0 or c < 0:
            return B_DC
        return int(modes[r, c, 4 + b])

    for r in range(rows):
        for c in range(cols):
            y0, x0, cy0, cx0 = 16 * r + 1, 16 * c + 1, 8 * r + 1, 8 * c + 1
            up, lf = int(r > 0), int(c > 0)
            S = sy[16 * r:16 * r + 16, 16 * c:16 * c + 16]
            SU, SV = su[8 * r:8 * r + 8, 8 * c:8 * c + 8], sv[8 * r:8 * r + 8, 8 * c:8 * c + 8]
            # 1. the chroma mode
            cpred = {}
            err = []
            for m in range(4):
                cpred[m] = [predict_block(m, P[cy0 - 1, cx0:cx0 + 8], P[cy0:cy0 + 8, cx0 - 1], int(P[cy0 - 1, cx0 - 1]), up, lf, 8) for P in (U, V)]
                err.append(int(((SU - cpred[m][0]) ** 2).sum() + ((SV - cpred[m][1]) ** 2).sum()))
            uv_mode = err.index(min(err))        # (index: the first of equal minima)
            # 2. the 16x16 mode
            above, left, tl = Y[y0 - 1, x0:x0 + 16], Y[y0:y0 + 16, x0 - 1], int(Y[y0 - 1, x0 - 1])
            rd16, ymode, best_sse, best_rate = INT_MAX, DC_PRED, 0, 0
            for m in range(4):
                d = S - predict_block(m, above, left, tl, up, lf, 16)
                total, sse = int(d.sum()), int((d * d).sum())
                var = sse - (((total * total) & 0xFFFFFFFF) >> 8)
                rd = rdcost(rdmult, rddiv, mbmode_cost[m], var)
                if rd16 > rd:
                    rd16, ymode, best_sse, best_rate = rd, m, sse, mbmode_cost[m]
            # 3. B_PRED
            rd4 = INT_MAX
            bm, bq, bdq, beob = [0] * 16, [None] * 16, [None] * 16, [0] * 16
            if not flags & NO_BPRED:
                cost, dist, done = mbmode_cost[B_PRED], 0, True
                aright = [int(v) for v in Y[y0 - 1, x0 + 16:x0 + 20]]       # vp8_intra_prediction_down_copy
                for b in range(16):
                    by, bx = b >> 2, b & 3
                    ctxA = bmode_of(r - 1, c, 12 + bx) if by == 0 else bm[b - 4]
                    ctxL = bmode_of(r, c - 1, 4 * by + 3) if bx == 0 else bm[b - 1]
                    py, px = y0 + 4 * by, x0 + 4 * bx
                    ab = [int(v) for v in Y[py - 1, px:px + 4]] + (aright if bx == 3 else [int(v) for v in Y[py - 1, px + 4:px + 8]])
                    lt, btl = [int(v) for v in Y[py:py + 4, px - 1]], int(Y[py - 1, px - 1])
                    s = [int(v) for v in S[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].ravel()]
                    best = (INT_MAX, 0, 0, 0, None)
                    for m in range(bmode_last + 1):
                        p = predict4(m, ab, lt, btl)
                        d = sum((a - e) ** 2 for a, e in zip(s, p))
                        rate = int(bmode_cost[ctxA, ctxL, m])
                        rd = rdcost(rdmult, rddiv, rate, d)
                        seen["tried"].add(m)
                        if rd < best[0]:
                            best = (rd, m, rate, d, p)
                    _, bm[b], rate, d, p = best
                    # vp8_encode_intra4x4block
                    q, dq, e = quant4(fdct4([_s16(a - e) for a, e in zip(s, p)]), f, extra, QR.Y1, quantizer)
                    add = idct4(dq) if e > 1 else [_s16((dq[0] + 4) >> 3)] * 16
                    Y[py:py + 4, px:px + 4] = np.clip(np.array(p) + np.array(add), 0, 255).reshape(4, 4)
                    bq[b], bdq[b], beob[b] = q, dq, e
                    cost += rate
                    dist += d
                    if dist > best_sse:
                        done = False
                        break
                if done:
                    rd4 = rdcost(rdmult, rddiv, cost, dist)
                else:
                    seen["breakout"] += 1
            # 4, 5. the decision and the encode
            lv, dqv, eob = np.zeros((25, 16), np.int64), np.zeros((25, 16), np.int64), np.zeros(25, np.int64)
            if rd4 < rd16:
                ymode, best_rate = B_PRED, cost
                lv[:16], dqv[:16], eob[:16] = np.array(bq), np.array(bdq), beob
                seen["bmodes"].update(bm)
                seen["bpred_eob_le1"] += sum(e <= 1 for e in beob)
                seen["bpred_eob_gt1"] += sum(e > 1 for e in beob)
                seen["last_col_bpred"] += int(c == cols - 1 and r > 0)
            else:
                bm = [IMPLIED_BMODE[ymode]] * 16
                pred = predict_block(ymode, above, left, tl, up, lf, 16)
                coef = np.zeros((1, 25, 4, 4), np.int64)
                coef[0, :16] = QR.fdct(QR._blocks(QR.fit(S - pred), 4))
                coef[0, 24] = QR.walsh(coef[0, :16, 0, 0].reshape(4, 4))
                coef = coef.reshape(1, 25, 16)
                take = np.array(list(range(16)) + [24])
                q, dq, e = QR.quantise(coef, f, extra, quantizer)
                lv[take], dqv[take], eob[take] = q[0, take], dq[0, take], e[0, take]
                # vp8_inverse_transform_mby
                wht = inv_walsh(dq[0, 24].reshape(4, 4), QR.fit).reshape(16) if e[0, 24] > 1 else np.full(16, int(QR.fit((dq[0, 24, 0] + 3) >> 3)))
                ea = np.where((e[0, :16] == 0) & (wht != 0), 1, e[0, :16])
                blk = q[0, :16].reshape(16, 4, 4).copy()
                blk[:, 0, 0] = wht
                fac = np.full((4, 4), int(f["dequant"][QR.Y1][1]), np.int64)
                fac[0, 0] = 1
                full = idct(QR.fit(blk * fac), QR.fit)
                dc = QR.fit((wht + 4) >> 3)
                add = np.where((ea > 1)[:, None, None], full, dc[:, None, None])
                Y[y0:y0 + 16, x0:x0 + 16] = np.clip(pred + QR._unblocks(add, 4), 0, 255)
                seen["y2_eob_le1" if e[0, 24] <= 1 else "y2_eob_gt1"] += 1
            # chroma: vp8_encode_intra16x16mbuv, vp8_dequant_idct_add_uv_block
            coef = np.zeros((1, 25, 16), np.int64)
            for k, (SP, P) in enumerate(((SU, cpred[uv_mode][0]), (SV, cpred[uv_mode][1]))):
                coef[0, 16 + 4 * k:20 + 4 * k] = QR.fdct(QR._blocks(QR.fit(SP - P), 2)).reshape(4, 16)
            q, dq, e = QR.quantise(coef, f, extra, quantizer)
            lv[16:24], dqv[16:24], eob[16:24] = q[0, 16:24], dq[0, 16:24], e[0, 16:24]
            full = idct(dq[0, 16:24].reshape(8, 4, 4), QR.fit)
            dc = QR.fit((dq[0, 16:24, 0] + 4) >> 3)
            add = np.where((e[0, 16:24] > 1)[:, None, None], full, dc[:, None, None])
            U[cy0:cy0 + 8, cx0:cx0 + 8] = np.clip(cpred[uv_mode][0] + QR._unblocks(add[:4], 2), 0, 255)
            V[cy0:cy0 + 8, cx0:cx0 + 8] = np.clip(cpred[uv_mode][1] + QR._unblocks(add[4:], 2), 0, 255)
            # what is kept
            skip = bool((eob[:16] < 2).all() and (eob[16:] == 0).all()) if ymode != B_PRED else bool((eob[:24] == 0).all())
            seen["skippable"] += skip
            levels[r, c], dequant[r, c] = lv, dqv
            eobs[r, c, :25] = eob
            modes[r, c, 0], modes[r, c, 1], modes[r, c, 2] = ymode, uv_mode, skip
            modes[r, c, 4:20] = bm
            stats["rd16"][r, c], stats["rd4"][r, c], stats["rate"][r, c], stats["eobs"][r, c] = rd16, rd4, best_rate, int(eob.sum())
            stats["recsse"][r, c] = int(((S - Y[y0:y0 + 16, x0:x0 + 16]) ** 2).sum() + ((SU - U[cy0:cy0 + 8, cx0:cx0 + 8]) ** 2).sum() +
                                        ((SV - V[cy0:cy0 + 8, cx0:cx0 + 8]) ** 2).sum())
        # vp8_extend_mb_row: the row's lines go on to the right with their last pixel
        Y[16 * r + 1:16 * r + 17, A + 1:] = Y[16 * r + 1:16 * r + 17, A:A + 1]
    return {"levels": QR.fit(levels).astype(np.int16), "dequant": QR.fit(dequant).astype(np.int16), "eob": eobs, "modes": modes,
            "stats": {k: v.astype(np.uint32) for k, v in stats.items()},
            "rec": [Y[1:, 1:A + 1].astype(np.uint8), U[1:, 1:].astype(np.uint8), V[1:, 1:].astype(np.uint8)], "seen": seen}


def stats_tensor(out, planes):
    """the stats of intra_planes' result as the call lays them out: uint32 [popcount, rows, cols] in bit order"""
    mask = planes if isinstance(planes, int) else sum({STATS[p] for p in planes})
    return np.stack([out["stats"][k] for k, bit in STATS.items() if mask & bit])


def rec_i420(out, w, h):
    """the reconstruction at the display size w x h in the packed I420 layout of the call's rec"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return np.concatenate([out["rec"][0][:h, :w].ravel(), out["rec"][1][:ch, :cw].ravel(), out["rec"][2][:ch, :cw].ravel()])


def to_ir(out):
    """-> (mbs uint8 [n, 64], coef int16 [n, 400]) as vp8_writer.write_key_frame takes them: the modes, the skip flag, and the levels
    transposed (the IR keeps a block column-major)"""
    rows, cols = out["modes"].shape[:2]
    n = rows * cols
    m = out["modes"].reshape(n, 32)
    mbs = np.zeros((n, 64), np.uint8)
    mbs[:, 0], mbs[:, 1], mbs[:, 3] = m[:, 0], m[:, 1], m[:, 2]
    mbs[:, 40:56] = m[:, 4:20]
    lv = out["levels"].reshape(n, 25, 4, 4).transpose(0, 1, 3, 2).reshape(n, 400).copy()
    return mbs, lv


# ---- the pictures of the cases --------------------------------------------------------------------------------------------------------
CONTENTS = ("decoded", "noise", "flat", "gradient", "vstripes", "hstripes")


def picture(kind, w, h, seed):
    """the coded planes (y, u, v) of size w x h (multiples of 16)"""
    import tfilter_reference as TR
    if kind == "decoded":
        return TR.sequence(w, h, seed, 1)[0]
    if kind == "noise":
        return TR.picture("noise", w, h, seed)
    if kind == "flat":
        return TR.picture("flat97", w, h, 0)
    rng = np.random.default_rng(seed)
    if kind in ("vstripes", "hstripes"):                   # every line (every column) the same: the pictures V_PRED and H_PRED win on
        def plane(n, m):
            line = rng.integers(40, 216, m if kind == "vstripes" else n)
            return np.ascontiguousarray(np.broadcast_to(line[None, :] if kind == "vstripes" else line[:, None], (n, m)).astype(np.uint8))
        return [plane(h, w), plane(h // 2, w // 2), plane(h // 2, w // 2)]
    assert kind == "gradient"
    yy, xx = np.mgrid[0:h, 0:w]
    a, b, c, d = rng.integers(-3, 4, 4)
    y = np.clip(128 + a * (xx - w // 2) + b * (yy - h // 2) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h // 2, 0:w // 2]
    u = np.clip(120 + c * xx + d * yy, 0, 255).astype(np.uint8)
    v = np.clip(140 - d * xx + c * yy, 0, 255).astype(np.uint8)
    return [y, u, v]
