"""Fixture of the structural-similarity call: what the REFERENCE's vp8_ssim2 (vp8/encoder/ssim.c) returns for a few dozen plane
pairs.

    python tests/golden/make_ssim_fixtures.py <shared object that exports vp8_ssim2>

ssim.c is compiled under CONFIG_INTERNAL_STATS only and is not part of oracle/_ref, which the rest of the suite pins.  The one file
compiles alone against the headers oracle/Makefile generates, into a shared object outside the repository (from oracle/, after
`make ref`; <reference> is the reference tree):
    cc -O2 -fPIC -shared -I_ref/gen -I_ref/gen/up -I<reference> -I<reference>/vp8/common -I<reference>/vp8/encoder \\
       -Dvp8_ssim_parms_8x8=vp8_ssim_parms_8x8_c -Dvp8_ssim_parms_16x16=vp8_ssim_parms_16x16_c \\
       -o <somewhere>/libssimref.so <reference>/vp8/encoder/ssim.c -lm
vp8_ssim2(img1, img2, stride1, stride2, width, height) is then callable through ctypes on numpy planes.

Writes, next to this file:
    ssim_ref.json    per case: the kind of pair, its size and seed (tests/ssim_reference.py's pair() makes the planes from them) and
                     vp8_ssim2's double as a hex float ("nan" where the plane has no windows: the reference's 0 / 0)
"""
import ctypes
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim_reference as SR  # noqa: E402

SIZES = [(16, 16), (17, 33), (9, 9), (25, 9), (12, 12), (13, 13), (67, 45), (130, 98), (8208, 16), (8, 8)]


def main():
    L = ctypes.CDLL(sys.argv[1])
    L.vp8_ssim2.restype = ctypes.c_double
    L.vp8_ssim2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    cases = []
    for w, h in SIZES:
        for k, kind in enumerate(SR.KINDS):
            seed = w * 131 + h * 7 + k
            s, r = (np.ascontiguousarray(p) for p in SR.pair(kind, w, h, seed))
            v = L.vp8_ssim2(s.ctypes.data, r.ctypes.data, w, w, w, h)
            cases.append({"kind": kind, "w": w, "h": h, "seed": seed, "ssim2": "nan" if math.isnan(v) else float(v).hex()})
    with open(os.path.join(HERE, "ssim_ref.json"), "w") as f:
        json.dump({"what": "vp8_ssim2(s, r) of ssim_reference.pair(kind, w, h, seed), as float.hex()", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
