"""Fixture of the temporal filter: what the REFERENCE's vp8_temporal_filter_apply_c (vp8/encoder/temporal_filter.c) accumulates over
the predictions of its six-tap, bilinear and copy functions, normalised as the reference normalises, for the pictures, vectors and
errors of tests/tfilter_reference.py.

    python tests/golden/make_tfilter_fixtures.py <reference tree> [<scratch directory>]

Needs oracle/_ref/libvpxref.so (make -C oracle ref), which exports those functions.  tfilter_ref_driver.c, beside this file, is
compiled against the reference's generated headers and that library into the scratch directory (default: a temporary one) and
called through ctypes.  The pictures are bordered here by edge replication, wide enough for the case's largest vector plus the taps.
Every case keeps strength in 1..6 (the reference's shift by strength - 1 is undefined at 0) and every error below 2^31 (the
reference compares an int): asserted here.

Writes, next to this file:
    tfilter_ref.json  per case: the size, the seed, how many sources, the filter, the strength, the kind of vectors and of weights
                      (tfilter_reference.sequence, fixture_mv, fixture_err make the inputs from them; case_inputs below), then the
                      picture (packed I420, uint8) and the count (the same geometry, uint16, little-endian) as the reference
                      computed them: in full -- base64 of their zlib stream -- for sizes up to 48x32, their SHA-256 above that
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
import subpel_reference as SR  # noqa: E402
import tfilter_reference as TR  # noqa: E402

FULL_UP_TO = 48 * 32


def cases():
    out = []

    def add(w, h, count, filt, strength, vectors, weights):
        out.append({"w": w, "h": h, "seed": w * 17 + h * 5 + len(out) * 9, "count": count, "filter": filt, "strength": strength, "vectors": vectors,
                    "weights": weights})
    add(32, 32, 1, "sixtap", 3, "zero", "two")
    add(32, 32, 2, "sixtap", 3, "phases", "two")
    add(32, 32, 3, "bilinear", 1, "phases", "mixed")
    add(32, 32, 15, "sixtap", 6, "search", "val")
    add(32, 32, 3, "sixtap", 3, "outside", "two")
    add(32, 32, 2, "bilinear", 6, "negodd", "mixed")
    add(32, 32, 3, "sixtap", 1, "zero", "none")
    add(48, 32, 1, "bilinear", 3, "phases", "two")
    add(48, 32, 2, "sixtap", 1, "negodd", "two")
    add(48, 32, 3, "sixtap", 6, "phases", "mixed")
    add(48, 32, 15, "bilinear", 3, "search", "val")
    add(48, 32, 3, "bilinear", 3, "outside", "mixed")
    add(48, 32, 15, "sixtap", 3, "zero", "two")
    for filt in TR.FILTERS:
        for strength in (1, 3, 6):
            add(176, 144, 3, filt, strength, "phases", "mixed")
    for count in (1, 2, 15):
        add(176, 144, count, "sixtap", 3, "search", "val")
    add(176, 144, 15, "bilinear", 6, "search", "two")
    add(176, 144, 2, "sixtap", 3, "negodd", "mixed")
    add(176, 144, 2, "bilinear", 1, "negodd", "two")
    add(176, 144, 3, "sixtap", 6, "outside", "two")
    add(176, 144, 2, "bilinear", 3, "outside", "mixed")
    add(176, 144, 3, "sixtap", 3, "zero", "mixed")
    add(176, 144, 2, "sixtap", 3, "phases", "none")
    return out


def case_inputs(c):
    """-> (centre planes, the list of the sources' planes, the vectors per source or None, the errors per source or None)"""
    rows, cols = c["h"] // 16, c["w"] // 16
    centre, sources = TR.sequence(c["w"], c["h"], c["seed"], c["count"])
    mvs = errs = None
    if c["vectors"] == "search":
        found = [SR.refine(centre[0], s[0], MR.search(centre[0], s[0], 4)[0].astype(np.int64)) for s in sources]
        mvs = [f[0].astype(np.int64) for f in found]
        if c["weights"] == "val":
            errs = [f[1][0] for f in found]
    elif c["vectors"] != "zero":
        mvs = [TR.fixture_mv(c["vectors"], rows, cols, c["seed"], k) for k in range(c["count"])]
    if c["weights"] not in ("two", "val"):
        errs = [TR.fixture_err(c["weights"], rows, cols, c["seed"], k) for k in range(c["count"])]
    assert c["weights"] != "val" or errs is not None
    return centre, sources, mvs, errs


def packed(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a).tobytes(), 9)).decode()


def unpacked(s, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), dtype)


def main():
    ref_tree = sys.argv[1]
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    oref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(scratch, "libtfilterref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(oref, "gen"), "-I" + os.path.join(oref, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-o", lib, os.path.join(HERE, "tfilter_ref_driver.c"), "-L" + oref,
                           "-lvpxref", "-lm", "-Wl,-rpath," + oref])
    L = ctypes.CDLL(lib)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.tfilter_ref_run.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp]
    done = []
    for c in cases():
        w, h, n = c["w"], c["h"], c["count"]
        assert 1 <= c["strength"] <= 6, c
        centre, sources, mvs, errs = case_inputs(c)
        assert errs is None or all(int(np.asarray(e).max()) < 1 << 31 for e in errs), c
        reach = 0 if mvs is None else max(int(np.abs(m).max()) for m in mvs)
        pad = 2 * ((reach // 8 + 24) // 2 + 1)

        def bordered(planes):
            return [np.ascontiguousarray(np.pad(p, pad if i == 0 else pad // 2, mode="edge")) for i, p in enumerate(planes)]
        cb = bordered(centre)
        sb = [p for s in sources for p in bordered(s)]
        ptrs = lambda arrs: (vp * len(arrs))(*[a.ctypes.data for a in arrs])
        mv = None if mvs is None else np.ascontiguousarray(np.stack(mvs), np.int32)
        er = None if errs is None else np.ascontiguousarray(np.stack(errs).astype(np.int64), np.int32)
        size = w * h + 2 * (w // 2) * (h // 2)
        out, cnt = np.zeros(size, np.uint8), np.zeros(size, np.uint16)
        rc = L.tfilter_ref_run(ptrs(cb), ptrs(sb), w, h, pad, n, None if mv is None else mv.ctypes.data, None if er is None else er.ctypes.data,
                               c["strength"], TR.FILTERS.index(c["filter"]), TR.THRESH[0], TR.THRESH[1], out.ctypes.data, cnt.ctypes.data)
        assert rc == 0, c
        cnt = cnt.astype("<u2")
        if w * h <= FULL_UP_TO:
            done.append(dict(c, picture=packed(out), counts=packed(cnt)))
        else:
            done.append(dict(c, picture_sha256=hashlib.sha256(out.tobytes()).hexdigest(), counts_sha256=hashlib.sha256(cnt.tobytes()).hexdigest()))
    with open(os.path.join(HERE, "tfilter_ref.json"), "w") as f:
        f.write('{"what": "vp8_temporal_filter_apply_c over the reference\'s predictions, normalised, for tfilter_reference.sequence(w, h, seed, count): '
                'packed I420 picture (uint8) and count (uint16 LE), base64 of zlib up to 48x32, SHA-256 above",\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in done))
        f.write("\n ]}\n")


if __name__ == "__main__":
    main()
