"""Fixture of the block motion search: what the REFERENCE's vp8_full_search_sad_c (vp8/encoder/mcomp.c), vp8_sad16x16_c and
vp8_variance16x16_c return for the picture pairs of tests/motion_reference.py.

    python tests/golden/make_motion_fixtures.py <reference tree> [<scratch directory>]

Needs oracle/_ref/libvpxref.so (make -C oracle ref), which exports all three.  motion_ref_driver.c, beside this file, is compiled
against the reference's headers and that library into the scratch directory (default: a temporary one) and called through ctypes.
The pictures are bordered here by 32 replicated pixels, as the reference's border extension leaves them.

Writes, next to this file:
    motion_ref.json   per case: the kind of pair, its size and seed (motion_reference.pair makes the pictures from them), the
                      distance, the kind of centre tensor and of cost table with its sad_per_bit (motion_reference.fixture_centre /
                      fixture_cost make them), then per macroblock in raster order [col, row, plain SAD at that vector, SAD at
                      (0, 0), SSE, VAR, SRCVAR] as the reference computed them (vector in whole pixels)
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


def cases():
    out = []

    def add(kind, w, h, d, centre="zero", cost=0):
        out.append({"kind": kind, "w": w, "h": h, "seed": w * 131 + h * 7 + d * 3 + len(out), "d": d, "centre": centre, "sad_per_bit": cost})
    for w, h in ((32, 32), (48, 32)):
        for d in (1, 4, 16):
            for kind in MR.KINDS:
                add(kind, w, h, d)
            for kind in ("noise", "smooth"):
                add(kind, w, h, d, "near")
                add(kind, w, h, d, "far")
    for kind in ("noise", "shifted", "stripes", "smooth"):
        add(kind, 48, 32, 64)
    add("noise", 32, 32, 64)
    add("noise", 48, 32, 64, "far")
    for kind in ("noise", "smooth", "shifted", "stripes"):
        for d in (4, 16):
            add(kind, 48, 32, d, "zero", 3)
            add(kind, 48, 32, d, "near", 40)
    add("smooth", 48, 32, 16, "zero", 255)
    add("stripes", 32, 32, 4, "far", 255)
    for kind in ("noise", "smooth", "shifted"):
        for d in (4, 16):
            add(kind, 176, 144, d)
    add("noise", 176, 144, 16, "far", 12)
    add("smooth", 176, 144, 16, "near", 12)
    return out


def main():
    ref_tree = sys.argv[1]
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    oref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(scratch, "libmotionref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(oref, "gen"), "-I" + os.path.join(oref, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-I" + os.path.join(ref_tree, "vpx_mem", "include"),
                           "-o", lib, os.path.join(HERE, "motion_ref_driver.c"), "-L" + oref, "-lvpxref", "-lm", "-Wl,-rpath," + oref])
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.motion_ref_run.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp]
    done = []
    for c in cases():
        w, h, d = c["w"], c["h"], c["d"]
        rows, cols = h // 16, w // 16
        s, r = (np.ascontiguousarray(np.pad(p, 32, mode="edge")) for p in MR.pair(c["kind"], w, h, c["seed"]))
        centre = MR.fixture_centre(c["centre"], rows, cols, c["seed"] + 1)
        centre = None if centre is None else np.ascontiguousarray(centre, np.int32)
        cost = MR.fixture_cost(d, c["seed"] + 2) if c["sad_per_bit"] else None
        out = np.zeros((rows * cols, 7), np.int32)
        rc = L.motion_ref_run(s.ctypes.data, r.ctypes.data, w, h, d, None if centre is None else centre.ctypes.data,
                              None if cost is None else cost.ctypes.data, c["sad_per_bit"], out.ctypes.data)
        assert rc == 0, c
        done.append(dict(c, mbs=out.tolist()))
    with open(os.path.join(HERE, "motion_ref.json"), "w") as f:
        f.write('{"what": "vp8_full_search_sad_c over motion_reference.pair(kind, w, h, seed): per macroblock [col, row, sad, sad0, sse, var, srcvar]",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in done))
        f.write("\n ]}\n")


if __name__ == "__main__":
    main()
