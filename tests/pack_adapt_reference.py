"""TEST INFRASTRUCTURE: the restatement of vp8hip_frames_pack_adapt_async (include/vp8hip.h).  The content is pack_reference's: the
same modes, skips and coded levels (pack_reference.restate is run first and its no-update frame is the anchor: with no flags and
the default baseline this module must write the same bytes).  From there: the frame as a list of EVENTS -- per macroblock the skip
flag, the mode tree's puts and the coded vector difference; per macroblock row the tokens with their (type, band, context) --, the
reference encoder's counts over those events, its choice of updates in integers (vp8_tree_probs_from_distribution,
prob_update_savings / update_coef_probs without error resilience, write_component_probs / calc_prob / update,
vp8_convert_rfct_to_prob: restated here from the reference's text; tests/golden/pack_adapt_ref.json holds what its exported
functions answer), and the frame through vp8_writer.BoolEncoder with token and vector writers that take the effective tables."""
import ctypes

import numpy as np

import pack_reference as PR
import vp8_writer as W
from vp8_testlib import load_package

COEF, MV, SKIP, REF = 1, 2, 4, 8
ALL = 15
PROBS_BYTES, COUNTS = 1104, 1216
UPDATE_BYTES = 8624                                 # the bound's share of the probability section: 9843 puts of 7 bits, rounded up
MV_PROB_UPDATE_CORRECTION = -1

_cost = None


def prob_cost():
    """the library's copy of vp8_prob_cost (csrc/host/vp8_enc_tables.c)"""
    global _cost
    if _cost is None:
        _cost = list((ctypes.c_uint16 * 256).in_dll(load_package().load_host(), "vp8t_prob_cost"))
    return _cost


def default_probs():
    T = W.tables()
    return np.array(list(T["coef"]) + list(T["mvc"]) + [0] * 10, np.uint8)


# ---- the choice -------------------------------------------------------------------------------------------------------------------
U32 = 0xffffffff


def cost_branch(c0, c1, p):
    """vp8_cost_branch, in the reference's unsigned 32-bit arithmetic"""
    C = prob_cost()
    return ((c0 * C[p] + c1 * C[255 - p]) & U32) >> 8


def coef_branches(c):
    """branch_counts over vp8_coef_tree of a context's 12 token counts (0 ZERO, 1..4, 5..10 DCT_CAT1..6, 11 the end of block)"""
    s = lambda a, b: sum(int(x) for x in c[a:b + 1]) & U32
    return [(int(c[11]), s(0, 10)), (int(c[0]), s(1, 10)), (int(c[1]), s(2, 10)), (s(2, 4), s(5, 10)), (int(c[2]), s(3, 4)), (int(c[3]), int(c[4])),
            (s(5, 6), s(7, 10)), (int(c[5]), int(c[6])), (s(7, 8), s(9, 10)), (int(c[7]), int(c[8])), (int(c[9]), int(c[10]))]


def tree_probs(branches):
    """vp8_tree_probs_from_distribution(..., Pfac 256, rd 1) of branch counts"""
    out = []
    for c0, c1 in branches:
        tot = (c0 + c1) & U32
        if tot:
            p = (((c0 * 256) & U32) + (tot >> 1) & U32) // tot
            out.append(255 if p >= 256 else p if p else 1)
        else:
            out.append(128)
    return out


def coef_saving(c0, c1, oldp, newp, upd):
    """prob_update_savings"""
    C = prob_cost()
    return cost_branch(c0, c1, oldp) - cost_branch(c0, c1, newp) - (8 + ((C[255 - upd] - C[upd]) >> 8))


def choose_coef(counts, base, on=True):
    """counts: the 1152 token counts; base: the 1056 baseline probabilities.  -> (effective [1056], update flags [1056], the sum
    of the positive savings)"""
    upd = W.tables()["coef_update"]
    eff, flag, saved = [int(b) for b in base], [0] * 1056, 0
    for row in range(96):
        br = coef_branches(counts[row * 12:row * 12 + 12])
        for t, newp in enumerate(tree_probs(br)):
            i = row * 11 + t
            s = coef_saving(br[t][0], br[t][1], eff[i], newp, upd[i])
            if on and s > 0:
                eff[i], flag[i] = newp, 1
                saved += s
    return eff, flag, saved & U32                               # (the call's info is uint32; the reference's int wraps alike)


def reduce_events(events):
    """write_component_probs' reduction of a component's histogram events[2047] (index 1023 + d) to the 32 branch counts:
    is_short_ct[2], sign_ct[2], short_ct[8], bit_ct[10][2]"""
    out = [0] * 32
    for d in range(-1023, 1024):
        n = int(events[1023 + d])
        if n:
            for k in component_bins(d):
                out[k] += n
    return out


def component_bins(d):
    """the counters a coded difference d adds 1 to"""
    x = abs(d)
    bins = [2 + (d < 0)] if x else []
    if x < 8:
        return bins + [0, 4 + x]
    return bins + [1] + [12 + 2 * k + ((x >> k) & 1) for k in range(10)]


def mv_branches(m):
    """the (c0, c1) of a component's 19 probabilities from its 32 branch counts"""
    sh = [int(v) for v in m[4:12]]
    s = lambda *ix: sum(sh[i] for i in ix)
    return [(int(m[0]), int(m[1])), (int(m[2]), int(m[3])), (s(0, 1, 2, 3), s(4, 5, 6, 7)), (s(0, 1), s(2, 3)), (sh[0], sh[1]), (sh[2], sh[3]),
            (s(4, 5), s(6, 7)), (sh[4], sh[5]), (sh[6], sh[7])] + [(int(m[12 + 2 * k]), int(m[13 + 2 * k])) for k in range(10)]


def choose_mv(m, base, comp, on=True):
    """m: a component's 32 branch counts; base: its 19 baseline probabilities.  -> (effective [19], update flags [19])"""
    T, C = W.tables(), prob_cost()
    dflt, upd = T["mvc"][19 * comp:19 * comp + 19], T["mv_update"][19 * comp:19 * comp + 19]
    eff, flag = [int(b) for b in base], [0] * 19
    for k, (c0, c1) in enumerate(mv_branches(m)):
        tot = (c0 + c1) & U32
        newp = dflt[k]                                          # calc_prob starts from the DEFAULT context
        if tot:
            x = ((((c0 * 255) & U32) // tot) & 0xff) & -2       # (a vp8_prob: the low byte)
            newp = x if x else 1
        cost = 7 + MV_PROB_UPDATE_CORRECTION + ((C[255 - upd[k]] - C[upd[k]] + 128) >> 8)
        if on and cost_branch(c0, c1, eff[k]) - cost_branch(c0, c1, newp) > cost:
            eff[k], flag[k] = newp, 1
    return eff, flag


def ref_probs(ref_frame):
    """vp8_convert_rfct_to_prob of a frame whose macroblocks are all inter on ref_frame: (prob_intra, prob_last, prob_gf)"""
    return (1, 255, 128) if ref_frame == 1 else (1, 1, 255) if ref_frame == 2 else (1, 1, 1)


# ---- the events -------------------------------------------------------------------------------------------------------------------
def mb_events(vec, rows, cols):
    """vec: int [rows, cols, 2] of (row, column).  -> per macroblock (the mode tree's puts [(bit, probability)], the coded
    difference (row, column) of a NEWMV macroblock or None), by the call's rule (pack_reference.choose_modes)"""
    MC = W.tables()["mode_contexts"]
    out = []

    def nb(r, c):
        return None if r < 0 or c < 0 else (int(vec[r, c, 0]), int(vec[r, c, 1]))
    for r in range(rows):
        for c in range(cols):
            v = nb(r, c)
            near, cnt, k = [(0, 0)] * 4, [0, 0, 0, 0], 0
            for t, weight in ((nb(r - 1, c), 2), (nb(r, c - 1), 2), (nb(r - 1, c - 1), 1)):
                if t is None:
                    continue
                if t != (0, 0):
                    if k == 0 or t != near[k]:
                        k += 1
                        near[k] = t
                    cnt[k] += weight
                else:
                    cnt[0] += weight
            e = (-((c * 16) << 3) - 128, (((cols - 1 - c) * 16) << 3) + 128, -((r * 16) << 3) - 128, (((rows - 1 - r) * 16) << 3) + 128)
            if v == (0, 0):
                out.append(([(0, MC[cnt[0] * 4])], None))
                continue
            puts = [(1, MC[cnt[0] * 4])]
            if cnt[3] and near[k] == near[1]:
                cnt[1] += 1
            if cnt[2] > cnt[1]:
                cnt[1], cnt[2] = cnt[2], cnt[1]
                near[1], near[2] = near[2], near[1]
            d = None
            if v == W._clamp_mv(near[1], e):
                puts.append((0, MC[cnt[1] * 4 + 1]))
            else:
                puts.append((1, MC[cnt[1] * 4 + 1]))
                if v == W._clamp_mv(near[2], e):
                    puts.append((0, MC[cnt[2] * 4 + 2]))
                else:
                    puts += [(1, MC[cnt[2] * 4 + 2]), (0, MC[3])]      # (NEWMV against SPLITMV: the split count is always 0)
                    best = W._clamp_mv(near[1] if cnt[1] >= cnt[0] else near[0], e)
                    d = ((v[0] - best[0]) >> 1, (v[1] - best[1]) >> 1)
            out.append((puts, d))
    return out


def token_events(coded, rows, cols):
    """coded: int [rows * cols, 25, 16], position 4 v + u, luma position 0 cleared.  -> per macroblock row the list of (type,
    band, context, level or None for the end of block, "follows a zero")"""
    has = np.zeros((rows * cols, 25), np.int64)
    none = np.zeros(25, np.int64)
    zz = list(PR.ZIGZAG)
    order = [(24, 1, 0)] + [(b, 0, 1) for b in range(16)] + [(b, 2, 0) for b in range(16, 24)]
    ev = [[] for _ in range(rows)]
    for mb in range(rows * cols):
        if not coded[mb].any():
            continue                                            # skipped: nothing is coded and its contexts are 0
        r, c = divmod(mb, cols)
        up, left = has[mb - cols] if r else none, has[mb - 1] if c else none
        for blk, btype, first in order:
            if blk == 24:
                ctx = up[24] + left[24]
            elif blk < 16:
                ctx = (has[mb, blk - 4] if blk >= 4 else up[blk + 12]) + (has[mb, blk - 1] if blk & 3 else left[blk + 3])
            else:
                q = (blk - 16) & 3
                ctx = (has[mb, blk - 2] if q >> 1 else up[blk + 2]) + (has[mb, blk - 1] if q & 1 else left[blk + 1])
            ctx = int(ctx)
            z = [int(coded[mb, blk, p]) for p in zz]
            end = max([i + 1 for i in range(first, 16) if z[i]], default=0)
            after_zero = False
            for i in range(first, 16):
                if i >= end:
                    ev[r].append((btype, W.COEF_BANDS[i], ctx, None, False))
                    break
                ev[r].append((btype, W.COEF_BANDS[i], ctx, z[i], after_zero))
                after_zero = z[i] == 0
                ctx = 0 if z[i] == 0 else 1 if abs(z[i]) == 1 else 2
            has[mb, blk] = int(end > first)
    return ev


def token_of(v):
    a = abs(v)
    return a if a < 5 else 5 if a < 7 else 6 if a < 11 else 7 if a < 19 else 8 if a < 35 else 9 if a < 67 else 10


def count_events(mbs, tokens):
    """-> the call's counts: int64 [1216]"""
    counts = np.zeros(COUNTS, np.int64)
    for row in tokens:
        for btype, band, ctx, v, _ in row:
            counts[((btype * 8 + band) * 3 + ctx) * 12 + (11 if v is None else token_of(v))] += 1
    for _, d in mbs:
        if d is not None:
            for comp in range(2):
                for k in component_bins(d[comp]):
                    counts[1152 + 32 * comp + k] += 1
    return counts


# ---- the frame --------------------------------------------------------------------------------------------------------------------
def prefix_encoder(qindex=40, deltas=(0, 0, 0, 0, 0), refresh_entropy_probs=1, **fields):
    """a BoolEncoder driven through the header fields in write_inter_frame's order, through refresh_last"""
    f = {**PR.DEFAULTS, **fields}
    e = W.BoolEncoder()
    e.literal(0, 1)
    e.literal(f["filter_type"], 1)
    e.literal(f["filter_level"], 6)
    e.literal(f["sharpness"], 3)
    e.literal(0, 1)
    e.literal(f["log2_parts"], 2)
    e.literal(qindex, 7)
    for d in deltas:
        if d:
            e.flag_value(d, 4)
        else:
            e.put(0, 128)
    e.literal(f["refresh_golden"], 1)
    e.literal(f["refresh_alt"], 1)
    if not f["refresh_golden"]:
        e.literal(f["copy_buffer_to_gf"], 2)
    if not f["refresh_alt"]:
        e.literal(f["copy_buffer_to_arf"], 2)
    e.literal(f["sign_bias_golden"], 1)
    e.literal(f["sign_bias_alt"], 1)
    e.literal(refresh_entropy_probs, 1)
    e.literal(f["refresh_last"], 1)
    return e


def write_frame(f, qindex, deltas, refresh, mbs, skipped, tokens, eff, flag, four):
    """the frame from its events, the effective set eff with its update flags, and four = (prob_skip_false, prob_intra,
    prob_last, prob_gf).  -> (frame, [the first partition's bytes, the token partitions'])"""
    T = W.tables()
    e = prefix_encoder(qindex, deltas, refresh, **f)
    for i in range(1056):
        e.put(flag[i], T["coef_update"][i])
        if flag[i]:
            e.literal(eff[i], 8)
    e.literal(1, 1)
    for p in four:
        e.literal(p, 8)
    e.literal(0, 2)
    for k in range(38):
        e.put(flag[1056 + k], T["mv_update"][k])
        if flag[1056 + k]:
            e.literal(eff[1056 + k] >> 1, 7)
    ref = f["ref_frame"]
    for (puts, d), skip in zip(mbs, skipped):
        e.put(int(skip), four[0])
        e.put(1, four[1])
        e.put(0 if ref == 1 else 1, four[2])
        if ref != 1:
            e.put(ref - 2, four[3])
        for bit, prob in puts:
            e.put(bit, prob)
        if d is not None:
            W._put_mv_component(e, d[0], eff[1056:1075])
            W._put_mv_component(e, d[1], eff[1075:1094])
    first = e.finish()
    nparts = 1 << f["log2_parts"]
    encs = [W.BoolEncoder() for _ in range(nparts)]
    for r, row in enumerate(tokens):
        te = encs[r % nparts]
        for btype, band, ctx, v, after_zero in row:
            p0 = ((btype * 8 + band) * 3 + ctx) * 11
            if v is None:
                te.put(0, eff[p0])
            else:
                W._put_token(te, v, eff[p0:p0 + 11], after_zero)
    parts = [x.finish() for x in encs]
    tag = 1 | (f["version"] << 1) | (f["show_frame"] << 4) | (len(first) << 5)
    out = bytearray([tag & 255, (tag >> 8) & 255, (tag >> 16) & 255]) + first
    for p in parts[:-1]:
        out += bytes([len(p) & 255, (len(p) >> 8) & 255, (len(p) >> 16) & 255])
    for p in parts:
        out += p
    return bytes(out), [len(first)] + [len(p) for p in parts]


def restate(mv, levels, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, flags=ALL, refresh_entropy_probs=1, probs_in=None, **fields):
    """mv, levels, qindex, deltas, cap, fields: as pack_reference.restate; probs_in: the baseline set, uint8 [1104], or None.
    -> a dict: "status", "data" (None where the status forbids), "info" (the call's 32 entries), "counts" [1216], "probs_out"
    [1104], "flag" (the update flags), "default" (pack_reference's frame of the same content), "plain" (all pack_reference.restate
    returns: the IR among it)"""
    f = {**PR.DEFAULTS, **fields}
    base = default_probs() if probs_in is None else np.asarray(probs_in, np.uint8).copy()
    base[1094:] = 0
    plain = PR.restate(mv, levels, qindex, deltas, **fields)
    info = np.zeros(32, np.int64)
    info[:16] = plain["info"]
    out = {"status": plain["status"], "data": None, "info": info, "counts": np.zeros(COUNTS, np.int64), "probs_out": base, "flag": None,
           "default": plain["data"], "plain": plain}
    if plain["status"] & (PR.BAD_VECTOR | PR.BAD_LEVEL):
        return out
    levels = np.asarray(levels)
    rows, cols = levels.shape[:2]
    n = rows * cols
    vec = np.zeros((rows, cols, 2), np.int64)
    if mv is not None:
        vec[..., 0], vec[..., 1] = np.asarray(mv)[1], np.asarray(mv)[0]
    coded = levels.reshape(n, 25, 16).astype(np.int64).copy()
    coded[:, :16, 0] = 0
    skipped = ~coded.any(axis=(1, 2))
    mbs, tokens = mb_events(vec, rows, cols), token_events(coded, rows, cols)
    counts = count_events(mbs, tokens)
    eff, flag, saved = choose_coef(counts[:1152], base[:1056], bool(flags & COEF))
    for comp in range(2):
        e2, f2 = choose_mv(counts[1152 + 32 * comp:1184 + 32 * comp], base[1056 + 19 * comp:1075 + 19 * comp], comp, bool(flags & MV))
        eff, flag = eff + e2, flag + f2
    skip = f["prob_skip_false"]
    if flags & SKIP:
        skip = min(max((n - int(skipped.sum())) * 256 // n, 1), 255)
    three = ref_probs(f["ref_frame"]) if flags & REF else (f["prob_intra"], f["prob_last"], f["prob_gf"])
    data, sizes = write_frame(f, qindex, deltas, refresh_entropy_probs, mbs, skipped, tokens, eff, flag, (skip,) + tuple(three))
    status = plain["status"] & PR.CLAMPS
    info[1], info[2] = len(data), sizes[0]
    info[3:11] = 0
    info[3:3 + len(sizes) - 1] = sizes[1:]
    if sizes[0] >= 1 << 19 or (cap is not None and len(data) > cap):
        status |= PR.OVERFLOW
        info[1] = 0
    info[0] = status
    info[16], info[17], info[18], info[19] = sum(flag[:1056]), sum(flag[1056:]), skip, saved
    out.update(status=status, data=None if status & PR.OVERFLOW else data, counts=counts, probs_out=np.array(eff + [0] * 10, np.uint8), flag=flag)
    return out
