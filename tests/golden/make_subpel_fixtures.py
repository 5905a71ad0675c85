"""Fixture of the sub-pixel refinement: what the REFERENCE's vp8_find_best_sub_pixel_step and vp8_find_best_half_pixel_step
(vp8/encoder/mcomp.c) return for the picture pairs of tests/subpel_reference.py.

    python tests/golden/make_subpel_fixtures.py <reference tree> [<scratch directory>]

Needs oracle/_ref/libvpxref.so (make -C oracle ref), which exports both and the variance functions they call.  subpel_ref_driver.c,
beside this file, is compiled against the reference's headers and that library into the scratch directory (default: a temporary
one) and called through ctypes.  The pictures are bordered here by 32 replicated pixels, as the reference's border extension leaves
them.  Every case keeps |sum| <= 46340 at every candidate evaluated (the reference's int product does not overflow) and every cost
index inside +-R (the reference reads inside its table): asserted here, on the restatement's log of its evaluations.

Writes, next to this file:
    subpel_ref.json   per case: the kind of pair, its size and seed (subpel_reference.pair makes the pictures from them), the kind of
                      start ("search": motion_reference.search at distance 4; else subpel_reference.fixture_start), the kind of
                      reference vectors, the cost table's range R (0: no table; subpel_reference.fixture_cost) with its
                      error_per_bit, the precision, then per macroblock in raster order [x, y, the return value, *distortion,
                      *sse1, the variance at the start] as the reference computed them (vector in 1/8 pel)
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import motion_reference as MR  # noqa: E402
import subpel_reference as SR  # noqa: E402


def cases():
    out = []

    def add(kind, w, h, start="zero", ref="zero", R=0, epb=0, precision=4):
        out.append({"kind": kind, "w": w, "h": h, "seed": w * 131 + h * 7 + len(out) * 3, "start": start, "ref": ref, "R": R, "error_per_bit": epb,
                    "precision": precision})
    kinds = [k for k in SR.KINDS if k != "extremes"]
    for w, h in ((32, 32), (48, 32)):
        for kind in kinds:
            for precision in (4, 2):
                add(kind, w, h, precision=precision)
        for kind in ("noise", "smooth", "half", "quarter", "shifted"):
            add(kind, w, h, "search")
            add(kind, w, h, "near", precision=2)
            add(kind, w, h, "far")
            add(kind, w, h, "bounds")
    for kind in ("noise", "smooth", "half", "quarter", "stripes"):
        add(kind, 48, 32, "zero", "zero", 40, 1)
        add(kind, 48, 32, "near", "given", 40, 300)
        add(kind, 48, 32, "search", "given", 255, 5000, 2)
        add(kind, 48, 32, "far", "given", 255, 16383)
        add(kind, 32, 32, "bounds", "zero", 255, 16383)
    add("flat", 48, 32, "zero", "given", 40, 16383)
    add("smooth", 64, 48, "search", "given", 255, 70)
    for kind in ("noise", "smooth", "half", "quarter"):
        add(kind, 176, 144)
        add(kind, 176, 144, "search", precision=2)
    add("noise", 176, 144, "far", "given", 1023, 900)
    add("noise", 176, 144, "bounds", "given", 1023, 16383)
    add("smooth", 176, 144, "near", "given", 1023, 16383)
    add("quarter", 176, 144, "search", "given", 1023, 40)
    return out


def case_inputs(c):
    """-> (s, ref, start or None, reference vectors or None, cost or None) of a fixture case"""
    s, r = SR.pair(c["kind"], c["w"], c["h"], c["seed"])
    rows, cols = c["h"] // 16, c["w"] // 16
    if c["start"] == "search":
        start = MR.search(s, r, 4)[0].astype(np.int32)
    else:
        start = SR.fixture_start(c["start"], rows, cols, c["seed"] + 1)
    rvec = SR.fixture_ref(c["ref"], rows, cols, c["seed"] + 3)
    return s, r, start, rvec, SR.fixture_cost(c["R"], c["seed"] + 2) if c["R"] else None


def main():
    ref_tree = sys.argv[1]
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    oref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(scratch, "libsubpelref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(oref, "gen"), "-I" + os.path.join(oref, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-I" + os.path.join(ref_tree, "vpx_mem", "include"),
                           "-o", lib, os.path.join(HERE, "subpel_ref_driver.c"), "-L" + oref, "-lvpxref", "-lm", "-Wl,-rpath," + oref])
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.subpel_ref_run.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    done = []
    for c in cases():
        w, h = c["w"], c["h"]
        rows, cols = h // 16, w // 16
        s, r, start, rvec, cost = case_inputs(c)
        # the reference's int product and its table: inside their ranges at every evaluation
        log = []
        SR.refine(s, r, start, rvec, cost, c["error_per_bit"], c["precision"], log)
        assert all(abs(e[2]) <= 46340 for e in log), c
        assert cost is None or all(abs(e[3]) <= c["R"] and abs(e[4]) <= c["R"] for e in log), c
        whole = np.zeros((2, rows, cols), np.int32)
        for my in range(rows):
            for mx in range(cols):
                whole[:, my, mx] = SR.clamp_start(s.shape, my, mx, *((0, 0) if start is None else start[:, my, mx]))
        rv = np.zeros((2, rows, cols), np.int32) if rvec is None or cost is None else np.ascontiguousarray(rvec, np.int32)
        sb, rb = (np.ascontiguousarray(np.pad(p, 32, mode="edge")) for p in (s, r))
        out = np.zeros((rows * cols, 6), np.int32)
        rc = L.subpel_ref_run(sb.ctypes.data, rb.ctypes.data, w, h, whole.ctypes.data, rv.ctypes.data, None if cost is None else cost.ctypes.data,
                              c["R"], c["error_per_bit"], c["precision"], out.ctypes.data)
        assert rc == 0, c
        done.append(dict(c, mbs=out.tolist()))
    with open(os.path.join(HERE, "subpel_ref.json"), "w") as f:
        f.write('{"what": "vp8_find_best_sub_pixel_step / _half_pixel_step over subpel_reference.pair(kind, w, h, seed): per macroblock [x, y, value, distortion, sse, var0]",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in done))
        f.write("\n ]}\n")


if __name__ == "__main__":
    main()
