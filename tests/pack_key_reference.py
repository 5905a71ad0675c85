"""TEST INFRASTRUCTURE: the restatement of vp8hip_frames_pack_key_async (include/vp8hip.h).  From frames_intra's modes and levels it
builds the IR tests/vp8_writer.py writes from as intra_reference.to_ir does -- the blocks transposed to the IR's column-major
order, what is not coded cleared (luma position 0 beside a Y2 block, block 24 of a B_PRED macroblock), the skip flag derived from
the coded levels -- and lets vp8_writer.write_key_frame, which the real reference decoder arbitrates (tests/test_pack_key_cpu.py),
write the frame.  It asserts that the product's host parser reads every mode and every skip flag back as given."""
import types

import numpy as np

import pack_reference as R
import vp8_writer as W
from vp8_testlib import load_package

OVERFLOW, BAD_LEVEL, BAD_MODE = 1, 4, 16
MAX_LEVEL = R.MAX_LEVEL
B_PRED = 4
IMPLIED = (0, 2, 3, 1)                             # DC -> B_DC, V -> B_VE, H -> B_HE, TM -> B_TM
DEFAULTS = dict(version=0, show_frame=1, color_space=0, clamping_type=0, filter_type=0, filter_level=0, sharpness=0, log2_parts=0, prob_skip_false=200)


def header(rows, cols, display, qindex, deltas, f):
    """what write_key_frame reads of a frame header, for the call's parameters f"""
    return types.SimpleNamespace(
        frame_type=0, mb_cols=cols, mb_rows=rows, width=display[0], height=display[1], color_space=f["color_space"], clamping_type=f["clamping_type"],
        segmentation_enabled=0, filter_type=f["filter_type"], filter_level=f["filter_level"], sharpness_level=f["sharpness"],
        mode_ref_lf_delta_enabled=0, base_qindex=qindex, y1dc_delta_q=deltas[0], y2dc_delta_q=deltas[1], y2ac_delta_q=deltas[2],
        uvdc_delta_q=deltas[3], uvac_delta_q=deltas[4], version=f["version"])


def header_encoder(qindex=40, deltas=(0, 0, 0, 0, 0), **fields):
    """a BoolEncoder driven through the header fields in write_key_frame's order, up to where the per-macroblock data begin"""
    f = {**DEFAULTS, **fields}
    e = W.BoolEncoder()
    e.literal(f["color_space"], 1)
    e.literal(f["clamping_type"], 1)
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
    e.literal(1, 1)
    for p in W.tables()["coef_update"]:
        e.put(0, p)
    e.literal(1, 1)
    e.literal(f["prob_skip_false"], 8)
    return e


def restate(modes, levels, qindex=40, deltas=(0, 0, 0, 0, 0), cap=None, display=None, check_parser=True, count_puts=False, **fields):
    """modes: uint8 [rows, cols, 32], levels: int16 [rows, cols, 25, 16], frames_intra's layouts; display: (w, h), default the coded
    size.  -> a dict: "status"; "data" (the frame; None where the status forbids); "info", the call's sixteen entries -- with
    BAD_LEVEL or BAD_MODE only [0], [1], [11] and [12] are defined, a y mode above 4 counting as one with a Y2 block --; "mbs",
    "coef", "hdr": the IR the frame was written from; "puts": where count_puts, the decisions of the first partition (the header's
    included) and of each token partition"""
    f = {**DEFAULTS, **fields}
    modes, levels = np.asarray(modes), np.asarray(levels)
    rows, cols = levels.shape[:2]
    n = rows * cols
    display = display or (16 * cols, 16 * rows)
    m = modes.reshape(n, 32)
    ym, uv, bm = m[:, 0].astype(np.int64), m[:, 1].astype(np.int64), m[:, 4:20].astype(np.int64)
    bpred = ym == B_PRED
    status = 0
    if (ym > 4).any() or (uv > 3).any() or (bm[bpred] > 9).any():
        status |= BAD_MODE
    coded = levels.reshape(n, 25, 16).astype(np.int64).copy()
    coded[~bpred, :16, 0] = 0
    coded[bpred, 24, :] = 0
    if (np.abs(coded) > MAX_LEVEL).any():
        status |= BAD_LEVEL
    skipped = ~coded.any(axis=(1, 2))
    info = np.zeros(16, np.int64)
    info[11], info[12] = int(skipped.sum()), int(bpred.sum())
    out = {"status": status, "data": None, "info": info}
    if status:
        info[0] = status
        return out
    hdr = header(rows, cols, display, qindex, deltas, f)
    mbs = np.zeros((n, 64), np.uint8)
    mbs[:, 0], mbs[:, 1], mbs[:, 3] = ym, uv, skipped
    mbs[:, 40:56] = np.where(bpred[:, None], bm, 0)
    coef = coded.reshape(n, 25, 4, 4).transpose(0, 1, 3, 2).reshape(n, 400).astype(np.int16)
    R.CountingEncoder.made, R.CountingEncoder.count_puts = [], count_puts
    plain, W.BoolEncoder = W.BoolEncoder, R.CountingEncoder
    try:
        data = W.write_key_frame(hdr, mbs, coef, log2_parts=f["log2_parts"], prob_skip_false=f["prob_skip_false"])
    finally:
        W.BoolEncoder = plain
    if not f["show_frame"]:
        data = bytes([data[0] & 0xef]) + data[1:]   # (the writer fixes the bit to 1)
    parts = 1 << f["log2_parts"]
    encs = R.CountingEncoder.made
    assert len(encs) == 1 + parts
    first = (data[0] | data[1] << 8 | data[2] << 16) >> 5
    assert first == len(encs[0].out) and len(data) == 10 + first + 3 * (parts - 1) + sum(len(e.out) for e in encs[1:])
    if check_parser:
        _check_parser(data, hdr, mbs, bpred, display, f)
    info[1], info[2] = len(data), first
    info[3:3 + parts] = [len(e.out) for e in encs[1:]]
    if first >= 1 << 19 or (cap is not None and len(data) > cap):
        status |= OVERFLOW
        info[1] = 0
    info[0] = status
    out.update(status=status, data=None if status & OVERFLOW else data, mbs=mbs, coef=coef, hdr=hdr,
               puts=[e.puts for e in encs] if count_puts else None)
    return out


def _check_parser(data, hdr, mbs, bpred, display, f):
    """the product's host parser reads the frame's size, modes and skip flags back as given"""
    P = load_package()
    parser = P.Parser()
    try:
        got, _, mbs2, _, _ = P.parse_to_numpy(parser, data)
    finally:
        parser.close()
    assert (got.width, got.height, got.frame_type, got.base_qindex) == (display[0], display[1], 0, hdr.base_qindex)
    assert got.num_token_partitions == 1 << f["log2_parts"] and got.filter_level == f["filter_level"]
    assert np.array_equal(mbs2[:, 0], mbs[:, 0]) and np.array_equal(mbs2[:, 1], mbs[:, 1]), "a mode did not come back as given"
    assert np.array_equal(mbs2[:, 3] & 1, mbs[:, 3] & 1), "a skip flag did not come back as derived"
    assert np.array_equal(mbs2[bpred, 40:56], mbs[bpred, 40:56]), "a sub-block mode did not come back as given"


# ---- the content the tests share -----------------------------------------------------------------------------------------------
def make_modes(kind, rows, cols, seed):
    """modes uint8 [rows, cols, 32]: "bpred" (every macroblock B_PRED), "16x16" (none), "mixed".  Bytes 2, 3 and 20..31 hold other
    values, and bytes 4..19 of a 16x16 macroblock modes that are NOT the implied ones: none of them is read"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 256, size=(rows, cols, 32)).astype(np.uint8)
    if kind == "bpred":
        ym = np.full((rows, cols), B_PRED)
    elif kind == "16x16":
        ym = rng.integers(0, 4, size=(rows, cols))
    else:
        assert kind == "mixed"
        ym = rng.integers(0, 5, size=(rows, cols))
        ym[rng.random((rows, cols)) < 0.3] = B_PRED
    m[..., 0], m[..., 1] = ym, rng.integers(0, 4, size=(rows, cols))
    m[..., 4:20] = rng.integers(0, 10, size=(rows, cols, 16))
    return m


def make_cover_modes(rows, cols, seed):
    """modes uint8 [rows, cols, 32] drawn so that (A, L) pairs are many: one macroblock of each 16x16 mode at a random place, the
    rest B_PRED, whose sub-block modes are chosen in raster order of the picture's sub-blocks -- each, where it can, so that the
    block to its right (whose A is known by then) meets a pair no block has met yet, else at random"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 256, size=(rows, cols, 32)).astype(np.uint8)
    ym = np.full(rows * cols, B_PRED)
    ym[rng.permutation(rows * cols)[:4]] = np.arange(4)
    ym = ym.reshape(rows, cols)
    m[..., 0], m[..., 1] = ym, (np.arange(rows * cols).reshape(rows, cols) + rng.integers(0, 4)) % 4
    grid = np.zeros((4 * rows + 1, 4 * cols + 2), np.int64)         # sub-block modes with B_DC above, to the left and to the right
    fixed = np.repeat(np.repeat(ym != B_PRED, 4, 0), 4, 1)
    grid[1:, 1:-1] = np.repeat(np.repeat(np.array(IMPLIED + (0,))[ym], 4, 0), 4, 1)
    met = set()
    for i in range(1, 4 * rows + 1):
        for j in range(1, 4 * cols + 1):
            if not fixed[i - 1, j - 1]:
                met.add((int(grid[i - 1, j]), int(grid[i, j - 1])))
                right_open = j < 4 * cols and not fixed[i - 1, j]
                fresh = [v for v in range(10) if (int(grid[i - 1, j + 1]), v) not in met] if right_open else []
                grid[i, j] = rng.choice(fresh) if fresh else rng.integers(0, 10)
    sub = grid[1:, 1:-1].reshape(rows, 4, cols, 4).transpose(0, 2, 1, 3).reshape(rows, cols, 16)
    m[..., 4:20] = np.where((ym == B_PRED)[..., None], sub, m[..., 4:20])
    return m


def make_levels(kind, rows, cols, seed):
    """pack_reference.make_levels: "zero", "sparse", "dense", "edges" -- position 0 of luma blocks and block 24 included, which a
    macroblock codes or does not by its y mode"""
    return R.make_levels(kind, rows, cols, seed)


def coverage(modes):
    """(y modes, uv modes, sub-block modes, (A, L) pairs) that occur in a frame of these modes, as sets"""
    rows, cols = modes.shape[:2]
    ym = modes[..., 0].astype(int)

    def sub(r, c, b):
        if r < 0 or c < 0:
            return 0
        return int(modes[r, c, 4 + b]) if ym[r, c] == B_PRED else IMPLIED[ym[r, c]]
    pairs, subs = set(), set()
    for r in range(rows):
        for c in range(cols):
            if ym[r, c] != B_PRED:
                continue
            for b in range(16):
                A = sub(r - 1, c, b + 12) if b < 4 else sub(r, c, b - 4)
                Lm = sub(r, c - 1, b + 3) if b % 4 == 0 else sub(r, c, b - 1)
                pairs.add((A, Lm))
                subs.add(sub(r, c, b))
    return set(ym.ravel().tolist()), set(modes[..., 1].ravel().tolist()), subs, pairs


def y2_context_case(first_has_level, column):
    """(modes, levels) of 64x64: along column 1 (column=True) or row 1 a macroblock with a Y2 block -- with a coded Y2 level or,
    first_has_level False, an empty Y2 block --, two B_PRED macroblocks of which the second is skipped, then a macroblock with a Y2
    block whose Y2 context therefore depends on the first one alone.  Everything else is skipped 16x16 macroblocks."""
    modes = np.zeros((4, 4, 32), np.uint8)
    levels = np.zeros((4, 4, 25, 16), np.int16)
    at = [(k, 1) if column else (1, k) for k in range(4)]
    for k, (r, c) in enumerate(at):
        modes[r, c, 0] = B_PRED if k in (1, 2) else 1 + k // 3        # V_PRED, B_PRED, B_PRED, H_PRED
        modes[r, c, 4:20] = (np.arange(16) * 3 + k) % 10
    (r, c) = at[0]
    levels[r, c, 24, 0] = 5 if first_has_level else 0
    levels[r, c, 2, 1], levels[r, c, 17, 0] = -1, 2                  # (not skipped either way)
    (r, c) = at[1]
    levels[r, c, 0, 0], levels[r, c, 5, 3], levels[r, c, 20, 0] = 3, -2, 1
    levels[r, c, 24, 0] = 9                                          # block 24 of a B_PRED macroblock: not read
    (r, c) = at[3]
    levels[r, c, 24, 0], levels[r, c, 24, 5], levels[r, c, 7, 2] = -4, 1, 1
    return modes, levels
