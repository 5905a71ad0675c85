#!/usr/bin/env python3
"""Records the fixtures of the intra tests:

  intra_ref.json           what the reference itself computes for the cases below: tests/golden/intra_ref_driver.c, a driver of our
                           own over what oracle/_ref/libvpxref.so exports, run on the pictures of intra_reference.picture()
  intra_ref_md5.json       the reference decoder's MD5 of the key frames the closure test writes
  intra_1080p_sha256.json  SHA-256 of the restatement's five outputs at 1920x1080 (tests/test_gpu_intra.py compares the device's)

    python3 tests/golden/make_intra_fixtures.py [ref <reference tree>] [md5] [1080p]

`ref` and `md5` need the reference build (make -C oracle ref); `ref` compiles the driver against the reference's headers."""
import base64
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intra_reference as IR  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
FULL_LIMIT = 48 * 32                                       # tensors of pictures up to this size are kept in full, larger ones as SHA-256

# display, content, seed, qindex, deltas (y1dc, y2dc, y2ac, uvdc, uvac), quantizer, zbin (over_quant, mode_boost, act_adj)
CASES = [
    ((16, 16), "decoded", 1, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((16, 16), "flat", 0, 127, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((32, 32), "noise", 2, 0, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((32, 32), "gradient", 3, 3, (0, 1, 0, 0, 0), "regular", (0, 0, 0)),
    ((32, 32), "gradient", 13, 112, (0, 0, 0, 0, 0), "fast", (0, 0, 0)),
    ((48, 32), "decoded", 4, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "decoded", 5, 40, (0, 0, 0, 0, 0), "fast", (0, 0, 0)),
    ((48, 32), "noise", 6, 112, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "gradient", 7, 40, (5, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "gradient", 8, 40, (0, -7, 0, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "decoded", 9, 40, (0, 0, 9, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "decoded", 10, 40, (0, 0, 0, -11, 0), "regular", (0, 0, 0)),
    ((48, 32), "decoded", 11, 40, (0, 0, 0, 0, 15), "regular", (0, 0, 0)),
    ((48, 32), "decoded", 12, 40, (0, 0, 0, 0, 0), "regular", (40, 0, 0)),
    ((48, 32), "decoded", 14, 40, (0, 0, 0, 0, 0), "regular", (0, 12, 0)),
    ((48, 32), "decoded", 15, 40, (0, 0, 0, 0, 0), "regular", (0, 0, -6)),
    ((48, 32), "vstripes", 22, 10, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((48, 32), "hstripes", 23, 10, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((67, 45), "decoded", 16, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((67, 45), "noise", 17, 127, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((67, 45), "gradient", 18, 60, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((176, 144), "decoded", 19, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0)),
    ((176, 144), "gradient", 20, 112, (3, -2, 5, -4, 7), "regular", (10, 3, 2)),
    ((176, 144), "noise", 21, 20, (0, 0, 0, 0, 0), "fast", (0, 0, 0)),
]
SHA_1080P = {"content": "decoded", "seed": 7, "qindex": 40, "bmode_last": 9}
CLOSURE = [((48, 32), "decoded", 4, 40), ((176, 144), "decoded", 19, 40)]          # x bmode_last 3 and 9


def aligned(display):
    return (display[0] + 15) // 16 * 16, (display[1] + 15) // 16 * 16


def case_key(c):
    return f"{c[0][0]}x{c[0][1]}_{c[1]}{c[2]}_q{c[3]}_{c[5]}_d" + ".".join(str(d) for d in c[4]) + "_z" + ".".join(str(z) for z in c[6])


def keep(a, full):
    """a tensor as the fixture keeps it: its bytes, deflated, in full, or their SHA-256"""
    raw = np.ascontiguousarray(a).tobytes()
    return {"zlib": base64.b64encode(zlib.compress(raw, 9)).decode()} if full else {"sha256": hashlib.sha256(raw).hexdigest()}


def same(kept, a):
    """a recorded tensor (keep) against an array of the type it was recorded with"""
    raw = np.ascontiguousarray(a).tobytes()
    if "sha256" in kept:
        return kept["sha256"] == hashlib.sha256(raw).hexdigest()
    return zlib.decompress(base64.b64decode(kept["zlib"])) == raw


def load_driver(ref_tree, scratch=None):
    """quant-fixture style: intra_ref_driver.c against the reference's headers and oracle/_ref/libvpxref.so, into a scratch directory"""
    import ctypes
    scratch = scratch or tempfile.mkdtemp()
    lib = os.path.join(scratch, "libintraref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(REF_DIR, "gen"), "-I" + os.path.join(REF_DIR, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-I" + os.path.join(ref_tree, "vpx_mem", "include"), "-o", lib,
                           os.path.join(HERE, "intra_ref_driver.c"), "-L" + REF_DIR, "-lvpxref", "-lm", "-Wl,-rpath," + REF_DIR])
    L = ctypes.CDLL(lib)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.intra_ref_run.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.intra_ref_helpers.argtypes = [vp, vp, vp]
    return L


def run_driver(L, src, q, deltas, quantizer, zbin):
    """-> the reference's record of one picture: a dict of arrays"""
    import ctypes
    h, w = src[0].shape
    n = (w // 16) * (h // 16)
    ints = lambda v: np.ascontiguousarray(v, np.int32)
    ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    sp = [np.ascontiguousarray(p) for p in src]
    d, z, rd = ints(deltas), ints(zbin), np.zeros(2, np.int32)
    modes, lv, eob = np.zeros((n, 18), np.uint8), np.zeros((n, 25, 16), np.int16), np.zeros((n, 25), np.uint8)
    rate, skip, rd16, rd4 = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rec = [np.zeros(p.shape, np.uint8) for p in sp]
    rc = L.intra_ref_run(ptrs(sp), w, h, q, d.ctypes.data, int(quantizer == "fast"), z.ctypes.data, rd.ctypes.data, modes.ctypes.data, lv.ctypes.data,
                         eob.ctypes.data, rate.ctypes.data, skip.ctypes.data, rd16.ctypes.data, rd4.ctypes.data, ptrs(rec))
    assert rc == 0
    return {"rdmult": int(rd[0]), "rddiv": int(rd[1]), "modes": modes, "levels": lv, "eob": eob, "rate": rate, "skip": skip, "rd16": rd16, "rd4": rd4,
            "rec": np.concatenate([p.ravel() for p in rec])}


def record_ref(ref_tree):
    import ctypes
    L = load_driver(ref_tree)
    cases = {}
    for c in CASES:
        display, kind, seed, q, deltas, quantizer, zbin = c
        w, h = aligned(display)
        o = run_driver(L, IR.picture(kind, w, h, seed), q, deltas, quantizer, zbin)
        full = w * h <= FULL_LIMIT
        cases[case_key(c)] = {"rdmult": o["rdmult"], "rddiv": o["rddiv"], **{k: keep(o[k], full) for k in ("modes", "levels", "eob", "rate", "skip", "rd16", "rd4", "rec")}}
    mb, b, rd = np.zeros(5, np.int32), np.zeros(1000, np.int32), np.zeros((128, 2), np.int32)
    assert L.intra_ref_helpers(mb.ctypes.data, b.ctypes.data, rd.ctypes.data) == 0
    helpers = {"mbmode_cost": mb.tolist(), "bmode_cost": b.tolist(), "rd": rd.tolist()}
    with open(os.path.join(HERE, "intra_ref.json"), "w") as f:
        json.dump({"what": "the reference's key-frame macroblock loop (vp8_pick_intra_mode, then the body of vp8cx_encode_intra_macro_block) on "
                           "intra_reference.picture(content, w, h, seed), recorded by make_intra_fixtures.py through intra_ref_driver.c; helpers: "
                           "vp8_init_mode_costs and vp8_initialize_rd_consts (RDMULT, RDDIV of every qindex)",
                   "cases": cases, "helpers": helpers}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


def closure_stream(display, kind, seed, q, last, costs):
    """the key frame of the closure test: -> (the restatement's result, the compressed frame)"""
    from vp8_testlib import synth_ir
    from vp8_writer import write_key_frame
    w, h = aligned(display)
    rdm, rdd = IR.intra_rd(q)
    o = IR.intra_planes(IR.picture(kind, w, h, seed), q, rdmult=rdm, rddiv=rdd, mbmode_cost=costs[0], bmode_cost=costs[1], bmode_last=last)
    hdr, _, _, _ = synth_ir(display[0], display[1], 1, inter=False, segmented=False)
    hdr.filter_level, hdr.base_qindex, hdr.mode_ref_lf_delta_enabled = 0, q, 0
    for f in ("y1dc_delta_q", "y2dc_delta_q", "y2ac_delta_q", "uvdc_delta_q", "uvac_delta_q"):
        setattr(hdr, f, 0)
    mbs, coef = IR.to_ir(o)
    return o, write_key_frame(hdr, mbs, coef)


def host_costs():
    import ctypes
    from vp8_testlib import load_package
    H = load_package().load_host()
    return IR.intra_costs(list((ctypes.c_uint16 * 256).in_dll(H, "vp8t_prob_cost")), list((ctypes.c_uint8 * 900).in_dll(H, "vp8t_kf_bmode_probs")))


def record_md5():
    from vp8_writer import write_ivf
    costs = host_costs()
    table = {}
    for display, kind, seed, q in CLOSURE:
        for last in (3, 9):
            _, data = closure_stream(display, kind, seed, q, last, costs)
            with tempfile.TemporaryDirectory() as d:
                ivf, out = os.path.join(d, "s.ivf"), os.path.join(d, "s.md5")
                write_ivf(ivf, display[0], display[1], [data])
                subprocess.run([os.path.join(REF_DIR, "ref_md5"), ivf, out], check=True)
                table[f"{display[0]}x{display[1]}_last{last}"] = {"stream_sha256": hashlib.sha256(data).hexdigest(), "md5": open(out).read().split()[0]}
    with open(os.path.join(HERE, "intra_ref_md5.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


def record_1080p():
    costs = host_costs()
    p = SHA_1080P
    rdm, rdd = IR.intra_rd(p["qindex"])
    o = IR.intra_planes(IR.picture(p["content"], 1920, 1088, p["seed"]), p["qindex"], rdmult=rdm, rddiv=rdd, mbmode_cost=costs[0], bmode_cost=costs[1],
                        bmode_last=p["bmode_last"])
    outs = {"coef": o["levels"], "eob": o["eob"], "stats": IR.stats_tensor(o, 31), "rec": IR.rec_i420(o, 1920, 1080), "modes": o["modes"]}
    rec = dict(p, sha256={k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in outs.items()})
    with open(os.path.join(HERE, "intra_1080p_sha256.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    what = sys.argv[1:]
    if "ref" in what:
        record_ref(what[what.index("ref") + 1])
    if "md5" in what:
        record_md5()
    if "1080p" in what:
        record_1080p()
