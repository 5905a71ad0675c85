"""Fixture of the transform-and-quantise call: what the REFERENCE's inter 16x16 encode (vp8_encode_inter16x16, then
vp8_inverse_transform_mby and vp8_dequant_idct_add_uv_block) makes of the pictures and vectors of tests/quant_reference.py, and what
vp8cx_init_quantizer computes for every qindex.

    python tests/golden/make_quant_fixtures.py <reference tree> [<scratch directory>]

Needs oracle/_ref/libvpxref.so (make -C oracle ref), which exports the functions.  quant_ref_driver.c, beside this file, is compiled
against the reference's headers and that library into the scratch directory (default: a temporary one) and called through ctypes.
The reference picture is bordered here by edge replication, wide enough for the case's largest vector plus the taps.  No case has a
vector component of 32767 or -32768, where the reference's `short` wraps and the definition does not: asserted here.

Writes, next to this file:
    quant_ref.json  "cases": per case the coded size, the display size, the seed, the content, the kind of vectors, the qindex, the five
                    deltas, the quantiser, the filter and the three zero-bin terms (case_inputs below makes the inputs from them),
                    then the reference's answers: levels and dequant (int16 LE [rows][cols][25][16]), eob (uint8 [rows][cols][32],
                    entries 25..31 zero), stats (uint32 LE [5][rows][cols]: mbblock_error(1), block_error of block 24, mbuverror, the
                    sum of the eobs, and the squared error of the reconstruction, the last two summed here from the reference's eobs
                    and pixels) and rec (packed I420 at the display size): in full -- base64 of their zlib stream -- for coded sizes
                    up to 48x32, their SHA-256 above that.  "factors": for three delta sets, the SHA-256 of all 128 tables of
                    vp8hip_quant_factors' layout (int16 LE [128][84]) and the tables of qindex 0, 40 and 127 in full
"""
import base64
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import motion_reference as MR  # noqa: E402
import quant_reference as QR  # noqa: E402
import subpel_reference as SR  # noqa: E402
import tfilter_reference as TR  # noqa: E402

FULL_UP_TO = 48 * 32
TENSORS = (("levels", "<i2"), ("dequant", "<i2"), ("eob", "u1"), ("stats", "<u4"), ("rec", "u1"))
DELTA_SETS = ((0, 0, 0, 0, 0), (3, -2, 5, -7, 4), (-15, 15, -15, 15, -15))
FACTOR_ROWS = (0, 40, 127)                                # the qindex values whose table is recorded in full
D0, D1, Z0 = DELTA_SETS[0], DELTA_SETS[1], (0, 0, 0)


def cases():
    out = []

    def add(w, h, content, vectors, q, deltas=D0, quantizer="regular", filt="sixtap", zbin=Z0, display=None, group=None):
        out.append({"w": w, "h": h, "display": list(display or (w, h)), "seed": w * 17 + h * 5 + len(out) * 9, "content": content, "vectors": vectors,
                    "qindex": q, "deltas": list(deltas), "quantizer": quantizer, "filter": filt, "zbin": list(zbin), "group": group})
    add(32, 32, "decoded", "zero", 40)
    add(32, 32, "decoded", "phases", 40, D1, "regular", "sixtap", (0, 12, 0))
    add(32, 32, "noise", "negodd", 3, (0, 1, 0, 0, 0), "fast")
    add(32, 32, "decoded", "search", 127, D1, "fast", "bilinear")
    add(32, 32, "decoded", "outside", 40, D0, "regular", "bilinear", (24, 0, 0))
    add(32, 32, "flat", "zero", 40)
    add(32, 32, "flatluma", "zero", 112)                                # only the Y2 DC survives: eob_adjust and the _1 inverse Walsh
    add(48, 32, "decoded", "phases", 40, D0, "regular", "sixtap", (0, 0, -3))
    add(48, 32, "noise", "search", 127, D1, "fast", "bilinear", (7, 9, 11))
    for q in (0, 40, 127, 3):                                           # one call's jobs: the same deltas, a qindex each
        add(32, 32, "decoded", "phases", q, D1, group="jobq")
    for q, deltas in ((0, D0), (3, (0, 1, 0, 0, 0)), (40, D1), (127, D0)):
        for quantizer in QR.QUANTIZERS:
            add(176, 144, "decoded", "search" if q == 40 else "phases", q, deltas, quantizer, "sixtap" if quantizer == "regular" else "bilinear")
    add(176, 144, "noise", "negodd", 40, D1, "regular", "bilinear")
    add(176, 144, "noise", "outside", 127, D0, "fast", "sixtap", (5, 0, 0))
    add(176, 144, "flat", "zero", 40)
    add(176, 144, "decoded", "zero", 40, D0, "regular", "sixtap", (0, 30, 0))
    add(176, 144, "decoded", "phases", 40, D0, "regular", "sixtap", (0, 0, 8))
    add(80, 48, "decoded", "phases", 40, D1, "regular", "sixtap", Z0, (67, 45))
    add(80, 48, "noise", "search", 3, (0, 1, 0, 0, 0), "fast", "bilinear", Z0, (67, 45))
    return out


def case_inputs(c):
    """-> (source planes, reference planes, the vectors [2, rows, cols] or None)"""
    rows, cols = c["h"] // 16, c["w"] // 16
    src, ref = QR.pictures(c["content"], c["w"], c["h"], c["seed"])
    if c["vectors"] == "search":
        mv = SR.refine(src[0], ref[0], MR.search(src[0], ref[0], 4)[0].astype(np.int64))[0].astype(np.int64)
    else:
        mv = TR.fixture_mv(c["vectors"], rows, cols, c["seed"])
    return src, ref, mv


def answers(c, levels, dequant, eob, stats, rec):
    """the five tensors of a case in the layouts the call writes, as little-endian arrays"""
    w, h = c["display"]
    return {"levels": levels.astype("<i2"), "dequant": dequant.astype("<i2"), "eob": eob.astype("u1"), "stats": stats.astype("<u4"),
            "rec": TR.pack(rec, w, h).astype("u1")}


def packed(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a).tobytes(), 9)).decode()


def unpacked(s, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), dtype)


def main():
    ref_tree = sys.argv[1]
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    oref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(scratch, "libquantref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(oref, "gen"), "-I" + os.path.join(oref, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-I" + os.path.join(ref_tree, "vpx_mem", "include"), "-o", lib,
                           os.path.join(HERE, "quant_ref_driver.c"), "-L" + oref, "-lvpxref", "-lm", "-Wl,-rpath," + oref])
    L = ctypes.CDLL(lib)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.quant_ref_run.argtypes = [vp, vp, ci, ci, ci, vp, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    L.quant_ref_factors.argtypes = [ci, vp, vp]
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ptrs = lambda arrs: (vp * len(arrs))(*[a.ctypes.data for a in arrs])
    done = []
    for c in cases():
        w, h = c["w"], c["h"]
        rows, cols = h // 16, w // 16
        src, ref, mv = case_inputs(c)
        assert mv is None or (int(mv.min()) > -32768 and int(mv.max()) < 32767), c
        reach = 0 if mv is None else int(np.abs(mv).max())
        pad = 2 * ((reach // 8 + 24) // 2 + 1)
        rb = [np.ascontiguousarray(np.pad(p, pad if i == 0 else pad // 2, mode="edge")) for i, p in enumerate(ref)]
        sp = [np.ascontiguousarray(p) for p in src]
        mvi = None if mv is None else ints(mv)
        deltas, zb = ints(c["deltas"]), ints(c["zbin"])
        n = rows * cols
        qc, dq = np.zeros((n, 400), np.int16), np.zeros((n, 400), np.int16)
        eobs, err = np.zeros((n, 25), np.uint8), np.zeros((n, 3), np.int32)
        rec = [np.zeros(p.shape, np.uint8) for p in src]
        rc = L.quant_ref_run(ptrs(sp), ptrs(rb), w, h, pad, None if mvi is None else mvi.ctypes.data, c["qindex"], deltas.ctypes.data,
                             QR.QUANTIZERS.index(c["quantizer"]), TR.FILTERS.index(c["filter"]), zb.ctypes.data, qc.ctypes.data, dq.ctypes.data,
                             eobs.ctypes.data, err.ctypes.data, ptrs(rec))
        assert rc == 0, c
        eob32 = np.zeros((n, 32), np.uint8)
        eob32[:, :25] = eobs
        sse = np.zeros((rows, cols), np.int64)
        for pl in range(3):
            s = 8 if pl else 16
            sse += ((src[pl].astype(np.int64) - rec[pl].astype(np.int64)) ** 2).reshape(rows, s, cols, s).sum(axis=(1, 3))
        stats = np.stack([err[:, 0].astype(np.int64), err[:, 1], err[:, 2], eobs.astype(np.int64).sum(axis=1), sse.ravel()]).reshape(5, rows, cols)
        got = answers(c, qc.reshape(rows, cols, 25, 16), dq.reshape(rows, cols, 25, 16), eob32.reshape(rows, cols, 32), stats, rec)
        if w * h <= FULL_UP_TO:
            done.append(dict(c, **{k: packed(v) for k, v in got.items()}))
        else:
            done.append(dict(c, **{k + "_sha256": hashlib.sha256(v.tobytes()).hexdigest() for k, v in got.items()}))
    tables = []
    for deltas in DELTA_SETS:
        t = np.zeros((128, 84), np.int16)
        d = ints(deltas)
        for q in range(128):
            assert L.quant_ref_factors(q, d.ctypes.data, t[q].ctypes.data) == 0
        tables.append({"deltas": list(deltas), "sha256": hashlib.sha256(t.astype("<i2").tobytes()).hexdigest(),
                       "rows": {str(q): t[q].tolist() for q in FACTOR_ROWS}})
    with open(os.path.join(HERE, "quant_ref.json"), "w") as f:
        f.write('{"what": "the reference\'s inter 16x16 encode and reconstruction of quant_reference.pictures(content, w, h, seed) at the vectors of '
                'make_quant_fixtures.case_inputs: levels, dequant (int16 LE), eob (uint8, 32 a macroblock), stats (uint32 LE, five planes), rec '
                '(packed I420), base64 of zlib up to 48x32, SHA-256 above; factors: vp8cx_init_quantizer\'s tables, int16 LE [128][84], as SHA-256 and three rows",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in done))
        f.write("\n ],\n \"factors\": [\n")
        f.write(",\n".join("  " + json.dumps(t, separators=(",", ":")) for t in tables))
        f.write("\n ]}\n")


if __name__ == "__main__":
    main()
