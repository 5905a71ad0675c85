"""TEST INFRASTRUCTURE: the restatement of vp8hip_frames_pack_async (include/vp8hip.h).  From frames_quant's levels and vectors it
builds the IR tests/vp8_writer.py writes from -- every macroblock inter, its mode chosen by the call's rule among ZEROMV, NEARESTMV,
NEARMV and NEWMV, the blocks transposed to the IR's column-major order with luma position 0 cleared -- and lets
vp8_writer.write_inter_frame, which the real reference decoder arbitrates (tests/test_writer_cpu.py), write the frame.  It asserts
that the writer carried every vector and every mode as given, so the rule cannot drift from what a decoder derives."""
import types

import numpy as np

import vp8_writer as W

OVERFLOW, BAD_VECTOR, BAD_LEVEL, CLAMPS = 1, 2, 4, 8
MAX_LEVEL = 2114                                   # DCT_CAT6: 67 + 2047
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)
DEFAULTS = dict(version=0, show_frame=1, filter_type=0, filter_level=0, sharpness=0, ref_frame=1, refresh_last=1, refresh_golden=0, refresh_alt=0,
                copy_buffer_to_gf=0, copy_buffer_to_arf=0, sign_bias_golden=0, sign_bias_alt=0, log2_parts=0, prob_skip_false=200, prob_intra=150,
                prob_last=140, prob_gf=100)
YMODE = {"zero": 7, "nearest": 5, "near": 6, "new": 8}


class CountingEncoder(W.BoolEncoder):
    """BoolEncoder that counts its carries -- all, and those that run through a 0xFF byte -- and, where asked, its puts"""
    made = []
    count_puts = False

    def __init__(self):
        super().__init__()
        self.carries = self.ff_carries = self.puts = 0
        CountingEncoder.made.append(self)
        if CountingEncoder.count_puts:
            self.put = self._counted_put

    def _counted_put(self, bit, prob):
        self.puts += 1
        W.BoolEncoder.put(self, bit, prob)

    def _carry(self):
        self.carries += 1
        self.ff_carries += self.out[-1] == 255
        super()._carry()


def header(rows, cols, qindex, deltas, f):
    """what write_inter_frame reads of a frame header, for the call's parameters f"""
    return types.SimpleNamespace(
        frame_type=1, mb_cols=cols, mb_rows=rows, segmentation_enabled=0, filter_type=f["filter_type"], filter_level=f["filter_level"],
        sharpness_level=f["sharpness"], mode_ref_lf_delta_enabled=0, base_qindex=qindex, y1dc_delta_q=deltas[0], y2dc_delta_q=deltas[1],
        y2ac_delta_q=deltas[2], uvdc_delta_q=deltas[3], uvac_delta_q=deltas[4], refresh_golden=f["refresh_golden"], refresh_alt=f["refresh_alt"],
        copy_buffer_to_gf=f["copy_buffer_to_gf"], copy_buffer_to_arf=f["copy_buffer_to_arf"], sign_bias_golden=f["sign_bias_golden"],
        sign_bias_alt=f["sign_bias_alt"], refresh_last=f["refresh_last"], version=f["version"], show_frame=f["show_frame"])


def header_encoder(qindex=40, deltas=(0, 0, 0, 0, 0), **fields):
    """a BoolEncoder driven through the header fields in write_inter_frame's order, up to where the per-macroblock data begin"""
    f = {**DEFAULTS, **fields}
    T = W.tables()
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
    e.literal(1, 1)
    e.literal(f["refresh_last"], 1)
    for p in T["coef_update"]:
        e.put(0, p)
    e.literal(1, 1)
    for name in ("prob_skip_false", "prob_intra", "prob_last", "prob_gf"):
        e.literal(f[name], 8)
    e.literal(0, 2)
    for p in T["mv_update"]:
        e.put(0, p)
    return e


def choose_modes(mv, rows, cols):
    """mv: int [rows, cols, 2] of (row, column).  -> (mode names [rows][cols], BAD_VECTOR / CLAMPS bits) by the call's rule"""
    modes, status = [[None] * cols for _ in range(rows)], 0
    if (mv & 1).any():
        status |= BAD_VECTOR

    def nb(r, c):
        return None if r < 0 or c < 0 else (int(mv[r, c, 0]), int(mv[r, c, 1]))
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
            if cnt[3] and near[k] == near[1]:
                cnt[1] += 1
            if cnt[2] > cnt[1]:
                cnt[1], cnt[2] = cnt[2], cnt[1]
                near[1], near[2] = near[2], near[1]
            left, right, top, bottom = -((c * 16) << 3), ((cols - 1 - c) * 16) << 3, -((r * 16) << 3), ((rows - 1 - r) * 16) << 3
            e = (left - 128, right + 128, top - 128, bottom + 128)
            if v == (0, 0):
                modes[r][c] = "zero"
            elif v == W._clamp_mv(near[1], e):
                modes[r][c] = "nearest"
            elif v == W._clamp_mv(near[2], e):
                modes[r][c] = "near"
            else:
                modes[r][c] = "new"
                best = W._clamp_mv(near[1] if cnt[1] >= cnt[0] else near[0], e)
                if any(abs((v[i] - best[i]) >> 1) > 1023 for i in range(2)):
                    status |= BAD_VECTOR
                if v[1] < left - (19 << 3) or v[1] > right + (18 << 3) or v[0] < top - (19 << 3) or v[0] > bottom + (18 << 3):
                    status |= CLAMPS
    return modes, status


def restate(mv, levels, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, count_puts=False, **fields):
    """mv: int [2, rows, cols], channel 0 = x, 1 = y, in 1/8 pel, or None; levels: int16 [rows, cols, 25, 16], position 4 v + u
    (frames_quant's layout).  -> a dict: "status"; "data" (the frame; None where the status forbids); "info", the call's sixteen
    entries; "carries" = [(carries, those through a 0xFF byte)] of the first partition and of each token partition; "puts"
    likewise where count_puts; "mbs", "coef", "mvs", "hdr": the IR the frame was written from"""
    f = {**DEFAULTS, **fields}
    levels = np.asarray(levels)
    rows, cols = levels.shape[:2]
    n = rows * cols
    vec = np.zeros((rows, cols, 2), np.int64)
    if mv is not None:
        vec[..., 0], vec[..., 1] = np.asarray(mv)[1], np.asarray(mv)[0]
    modes, status = choose_modes(vec, rows, cols)
    coded = levels.reshape(n, 25, 16).astype(np.int64).copy()
    coded[:, :16, 0] = 0
    if (np.abs(coded) > MAX_LEVEL).any():
        status |= BAD_LEVEL
    skipped = ~coded.any(axis=(1, 2))
    names = [m for row in modes for m in row]
    info = np.zeros(16, np.int64)
    info[11] = int(skipped.sum())
    for i, name in enumerate(("zero", "nearest", "near", "new")):
        info[12 + i] = names.count(name)
    out = {"status": status, "data": None, "info": info, "carries": None, "puts": None}
    if status & (BAD_VECTOR | BAD_LEVEL):
        info[0] = status
        return out
    hdr = header(rows, cols, qindex, deltas, f)
    mbs = np.zeros((n, 64), np.uint8)
    mbs[:, 0], mbs[:, 2], mbs[:, 3] = [YMODE[m] for m in names], f["ref_frame"], skipped
    coef = coded.reshape(n, 25, 4, 4).transpose(0, 1, 3, 2).reshape(n, 400).astype(np.int16)
    mvs = np.zeros((n, 16, 2), np.int64)
    mvs[:] = vec.reshape(n, 1, 2)
    CountingEncoder.made, CountingEncoder.count_puts = [], count_puts
    plain, W.BoolEncoder = W.BoolEncoder, CountingEncoder
    try:
        data, mbs2, mvs2 = W.write_inter_frame(hdr, mbs, coef, mvs, log2_parts=f["log2_parts"], prob_skip_false=f["prob_skip_false"],
                                               prob_intra=f["prob_intra"], prob_last=f["prob_last"], prob_gf=f["prob_gf"])
    finally:
        W.BoolEncoder = plain
    assert np.array_equal(mvs2, mvs), "the writer did not carry the vectors as given"
    assert np.array_equal(mbs2[:, 0], mbs[:, 0]) and np.array_equal(mbs2[:, 2], mbs[:, 2]), "a mode did not come back as chosen"
    parts = 1 << f["log2_parts"]
    encs = CountingEncoder.made
    assert len(encs) == 1 + parts
    first = (data[0] | data[1] << 8 | data[2] << 16) >> 5
    assert first == len(encs[0].out) and len(data) == 3 + first + 3 * (parts - 1) + sum(len(e.out) for e in encs[1:])
    info[1], info[2] = len(data), first
    info[3:3 + parts] = [len(e.out) for e in encs[1:]]
    if first >= 1 << 19 or (cap is not None and len(data) > cap):
        status |= OVERFLOW
        info[1] = 0
    info[0] = status
    out.update(status=status, data=None if status & OVERFLOW else data, carries=[(e.carries, e.ff_carries) for e in encs],
               puts=[e.puts for e in encs] if count_puts else None, mbs=mbs, coef=coef, mvs=mvs, hdr=hdr)
    return out


# ---- the content the tests share -----------------------------------------------------------------------------------------------
ALPHABET = np.array([[0, 0], [0, 0], [2, -4], [2, -4], [-6, 8], [300, -200], [-900, 1000], [16, 16]])     # (x, y), all even


def make_field(kind, rows, cols, seed):
    """a vector field int16 [2, rows, cols]: "zero", "equal" (NEARESTMV everywhere but the first), "alphabet" (few distinct vectors,
    so that all four modes occur), "far" (far outside the picture)"""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((2, rows, cols), np.int16)
    if kind == "equal":
        return np.broadcast_to(np.array([-12, 6], np.int16).reshape(2, 1, 1), (2, rows, cols)).copy()
    if kind == "alphabet":
        v = ALPHABET[rng.integers(0, len(ALPHABET), size=(rows, cols))]
        v = v + 2 * rng.integers(-1, 2, size=v.shape) * (rng.random(v.shape) < 0.2)
        return np.ascontiguousarray(v.transpose(2, 0, 1)).astype(np.int16)
    assert kind == "far"                    # (all up and to the left: beyond the border at the first row and column, differences in range)
    return (-2 * rng.integers(80, 451, size=(2, rows, cols))).astype(np.int16)


CAT_EDGES = (1, 2, 3, 4, 5, 6, 7, 10, 11, 18, 19, 34, 35, 66, 67, 2114)


def make_levels(kind, rows, cols, seed):
    """levels int16 [rows, cols, 25, 16]: "zero", "sparse", "dense", "edges" (both signs of every magnitude at which the token tree or
    a DCT category changes)"""
    rng = np.random.default_rng(seed)
    shape = (rows, cols, 25, 16)
    if kind == "zero":
        return np.zeros(shape, np.int16)
    if kind == "sparse":
        lv = (rng.random(shape) < 0.05) * rng.integers(-70, 71, size=shape)
        lv[rng.random((rows, cols)) < 0.3] = 0                                  # some macroblocks are skipped
        return lv.astype(np.int16)
    if kind == "dense":
        return ((rng.random(shape) < 0.7) * rng.integers(-40, 41, size=shape)).astype(np.int16)
    assert kind == "edges"
    mags = np.array(CAT_EDGES)[rng.integers(0, len(CAT_EDGES), size=shape)]
    return ((rng.random(shape) < 0.3) * mags * rng.choice([-1, 1], size=shape)).astype(np.int16)


# ---- a carry that runs through 0xFF bytes, made on purpose ---------------------------------------------------------------------
# The bool coder keeps three bytes of `bottom` behind the byte it writes, so a carry into a written byte needs some 23 one bits in
# a row and one into a written 0xFF byte some 31: no seed of random content is found to have one.  But the tokens of a block
# partition the coder's interval, so for any boundary B inside it there is a sequence of tokens whose intervals all contain B: the
# low end then creeps up to B from below -- 0x..7F 0xFF 0xFF ... -- and one step to the upper side crosses it.
def _interval(e):
    """the coder's absolute interval: (low, bits) with the interval [low, low + e.range) in units of 2^-bits"""
    c, n = e.bit_count, len(e.out)
    return ((int.from_bytes(e.out, "big") << (32 - c)) if n else 0) + e.bottom, 8 + 8 * n + 24 - c


def carry_levels(rows=2, cols=3, straddle_bits=44):
    """levels int16 [rows, cols, 25, 16] of a frame (vectors zero, one token partition) whose token partition has a carry that
    runs through 0xFF bytes: the first boundary (2 j + 1) / 1024 for which the tokens whose intervals contain it make a frame"""
    for j in range(512):
        try:
            lv = _levels_around((2 * j + 1, 10), rows, cols, straddle_bits)
        except _NoFrame:
            continue
        if lv is not None:
            return lv
    raise AssertionError("no boundary makes a frame")


class _NoFrame(Exception):
    pass


def _levels_around(boundary, rows, cols, straddle_bits):
    """tokens chosen so that `boundary` = (num, k), num / 2^k, stays inside the coder's interval for straddle_bits bits, then the
    step across it, then nothing more; None where that is no frame: a macroblock without a level would have been skipped, and the
    macroblocks may run out"""
    T = W.tables()["coef"]
    lv = np.zeros((rows * cols, 25, 16), np.int64)
    has = np.zeros((rows * cols, 25), np.int64)
    e = W.BoolEncoder()
    state = {"mode": "straddle", "B": boundary}

    def decide(prob, allowed=(0, 1)):
        """the bit of the next put: by the mode, among `allowed`"""
        if len(allowed) == 1:
            bit = allowed[0]
        elif state["mode"] == "free":
            bit = allowed[0]
        else:
            low, bits = _interval(e)
            cut = low + 1 + (((e.range - 1) * prob) >> 8)
            num, k = state["B"]                                  # B = num / 2^k
            b, cut = num << max(bits - k, 0), cut << max(k - bits, 0)
            if b == cut:                                         # on the cut: the boundary would become the low end itself
                raise _NoFrame
            below = b < cut
            if state["mode"] == "cross" and below:
                bit, state["mode"] = 1, "free"
            else:
                bit = 0 if below else 1
        e.put(bit, prob)
        return bit

    def token(p, after_zero, last_step):
        """one token by decisions; returns the level, or None for the end of the block"""
        if not after_zero and not decide(p[0]):
            return None
        if not decide(p[1], (1,) if last_step else (0, 1)):
            return 0
        if not decide(p[2]):
            a = 1
        elif not decide(p[3]):
            a = 2 if not decide(p[4]) else 3 + decide(p[5])
        else:
            if not decide(p[6]):
                cat = decide(p[7])
            else:
                hi = decide(p[8])
                cat = 2 + 2 * hi + decide(p[10] if hi else p[9])
            extra = 0
            for pb in W.CAT_PROBS[cat]:
                extra = extra * 2 + decide(pb)
            a = W.CAT_BASE[cat] + extra
        return -a if decide(128) else a

    order = [(24, 1, 0)] + [(b, 0, 1) for b in range(16)] + [(b, 2, 0) for b in range(16, 24)]
    none = np.zeros(25, np.int64)
    for mb in range(rows * cols):
        up, left = has[mb - cols] if mb >= cols else none, has[mb - 1] if mb % cols else none
        if state["mode"] == "free":
            break                                                # the rest of the frame is skipped
        for blk, btype, first in order:
            if blk == 24:
                ctx = up[24] + left[24]
            elif blk < 16:
                ctx = (has[mb, blk - 4] if blk >= 4 else up[blk + 12]) + (has[mb, blk - 1] if blk & 3 else left[blk + 3])
            else:
                q = (blk - 16) & 3
                ctx = (has[mb, blk - 2] if q >> 1 else up[blk + 2]) + (has[mb, blk - 1] if q & 1 else left[blk + 1])
            after_zero = False
            for i in range(first, 16):
                if state["mode"] == "straddle" and _interval(e)[1] - 8 >= straddle_bits:
                    state["mode"] = "cross"
                p0 = ((btype * 8 + W.COEF_BANDS[i]) * 3 + ctx) * 11
                v = token(T[p0:p0 + 11], after_zero, i == 15)         # (a block cannot end on zeros: its last step refuses one)
                if v is None:
                    break
                lv[mb, blk, ZIGZAG[i]] = v
                after_zero = v == 0
                ctx = 0 if v == 0 else 1 if abs(v) == 1 else 2
            has[mb, blk] = int(lv[mb, blk].any())
        if not has[mb].any():
            return None
    if state["mode"] != "free" or np.abs(lv).max() > MAX_LEVEL:
        return None
    return lv.reshape(rows, cols, 25, 16).astype(np.int16)
