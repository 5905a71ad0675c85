"""Fixture of the frame packer's probability adaptation: what the REFERENCE's exported functions answer for seeded count sets.

    python tests/golden/make_pack_adapt_fixtures.py <reference tree> [<scratch directory>]

Needs oracle/_ref/libvpxref.so (make -C oracle ref) and the built product (the restatement reads its tables).
pack_adapt_ref_driver.c, beside this file, is compiled against the reference's headers and that library into the scratch directory
(default: a temporary one) and called through ctypes.  Recorded in pack_adapt_ref.json, next to this file:
    "cost"     vp8_prob_cost, 256 entries
    "tree"     vp8_tree_probs_from_distribution(12, vp8_coef_encodings, vp8_coef_tree, ..., 256, 1): per case the 12 counts, the 11
               probabilities and the 11 x 2 branch counts
    "savings"  vp8_estimate_entropy_savings on a zeroed VP8_COMP (key frame, no error resilience: default_coef_context_savings):
               per case the non-zero token counts {index: count} of [4][8][3][12], the baseline ("default" or its 1056 values), the
               1056 probabilities it leaves in frame_coef_probs and the saving it returns
    "mv"       vp8_write_mvprobs on a zeroed VP8_COMP: per case the non-zero events {component: {d: count}}, the context before, the
               context after and the bytes of the bool coder (vp8_stop_encode's 32 padding bits included)
Cases: empty, one event, saturated (counts near 2^24, where the reference's 32-bit products wrap), seeded random ones, and counts at
a saving of exactly 0 and exactly 1 (coefficients) or exactly at and one above the threshold (vectors), found here by search with
the restatement.  The reference's STATIC functions -- prob_update_savings, update_coef_probs' flag, calc_prob, update,
write_component_probs -- cannot be called: they are restated in tests/pack_adapt_reference.py, and what is recorded here pins them
through the exported functions around them (the returned saving is the sum of the positive prob_update_savings; the bytes and the
context after vp8_write_mvprobs are update's decisions)."""
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
import pack_adapt_reference as A  # noqa: E402


def coef_cases():
    """-> [(name, counts int64 [1152], baseline uint8 [1056])]"""
    rng = np.random.default_rng(2906)
    dflt = A.default_probs()[:1056]
    other = np.clip(dflt.astype(np.int64) + rng.integers(-60, 61, size=1056), 1, 255).astype(np.uint8)
    z = lambda: np.zeros(1152, np.int64)
    out = [("empty", z(), dflt)]
    one = z(); one[(0 * 8 + 1) * 3 * 12 + 3] = 1
    out.append(("one event", one, dflt))
    sat = z(); sat[:] = rng.integers((1 << 24) - 5000, 1 << 24, size=1152)
    out.append(("saturated", sat, dflt))
    wrap = z(); wrap[:] = rng.integers(0, 1 << 20, size=1152); wrap[5::12] = (1 << 24) - 1
    out.append(("saturated zeros", wrap, other))
    sparse = (rng.random(1152) < 0.2) * rng.integers(1, 40, size=1152)
    out.append(("random sparse", sparse.astype(np.int64), dflt))
    dense = rng.integers(0, 3000, size=1152) * (rng.random(1152) < 0.8)
    out.append(("random dense", dense.astype(np.int64), other))
    # one context with counts, the largest saving of its nodes exactly `target`: the flag is 0 at 0 and 1 at 1
    upd = A.W.tables()["coef_update"]
    for target in (0, 1):
        while True:
            row = int(rng.integers(0, 96))
            c = rng.integers(0, 12, size=12) * (rng.random(12) < 0.6)
            br = A.coef_branches(c)
            s = [A.coef_saving(br[t][0], br[t][1], int(dflt[row * 11 + t]), p, upd[row * 11 + t]) for t, p in enumerate(A.tree_probs(br))]
            if max(s) == target and s.count(target) == 1:
                break
        one = z(); one[row * 12:row * 12 + 12] = c
        out.append((f"saving of exactly {target}", one, dflt))
    return out


def mv_cases():
    """-> [(name, events int64 [2][2047], context before uint8 [38])]"""
    rng = np.random.default_rng(1706)
    dflt = A.default_probs()[1056:1094]
    other = np.clip(dflt.astype(np.int64) + rng.integers(-50, 51, size=38), 1, 255).astype(np.uint8)
    z = lambda: np.zeros((2, 2047), np.int64)
    out = [("empty", z(), dflt)]
    one = z(); one[0, 1023 + 5] = 1
    out.append(("one short event", one, dflt))
    one = z(); one[1, 1023 - 700] = 1
    out.append(("one long event", one, other))
    sat = z(); sat[:] = rng.integers(0, 9000, size=(2, 2047))
    out.append(("saturated", sat, dflt))
    short = z(); short[:, 1023 - 7:1023 + 8] = rng.integers(0, 50, size=(2, 15))
    out.append(("short", short, dflt))
    mixed = z(); mixed[:] = (rng.random((2, 2047)) < 0.03) * rng.integers(1, 6, size=(2, 2047)); mixed[:, 1023] = 40
    out.append(("mixed", mixed, other))
    # is_short of the row component exactly at the threshold (no update) and one above it (update): a zeros, b events of 8
    T, C = A.W.tables(), A.prob_cost()
    cost = 7 + A.MV_PROB_UPDATE_CORRECTION + ((C[255 - T["mv_update"][0]] - C[T["mv_update"][0]] + 128) >> 8)
    found = {}
    for a in range(0, 60):
        for b in range(0, 60):
            if a + b == 0:
                continue
            x = ((a * 255) // (a + b)) & 0xfe
            newp = x if x else 1
            d = A.cost_branch(a, b, int(dflt[0])) - A.cost_branch(a, b, newp) - cost
            if d in (0, 1) and d not in found:
                found[d] = (a, b)
    for d, name in ((0, "exactly at the threshold"), (1, "one above the threshold")):
        ev = z(); ev[0, 1023], ev[0, 1023 + 8] = found[d]
        out.append((f"is_short {name}", ev, dflt))
    return out


def main():
    ref_tree = sys.argv[1]
    scratch = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    os.makedirs(scratch, exist_ok=True)
    oref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(scratch, "libpackadaptref.so")
    subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-w", "-I" + os.path.join(oref, "gen"), "-I" + os.path.join(oref, "gen", "up"),
                           "-I" + ref_tree, "-I" + os.path.join(ref_tree, "vp8"), "-I" + os.path.join(ref_tree, "vpx_mem", "include"), "-o", lib,
                           os.path.join(HERE, "pack_adapt_ref_driver.c"), "-L" + oref, "-lvpxref", "-lm", "-Wl,-rpath," + oref])
    L = ctypes.CDLL(lib)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.adapt_ref_cost.argtypes = [vp]
    L.adapt_ref_tree.argtypes = [vp, vp, vp]
    L.adapt_ref_savings.argtypes = [vp, vp, vp, vp]
    L.adapt_ref_mvprobs.argtypes = [vp, vp, vp, ci]
    cost = np.zeros(256, np.uint32)
    L.adapt_ref_cost(cost.ctypes.data)
    tree, savings, mv = [], [], []
    for name, counts, base in coef_cases():
        c32 = np.ascontiguousarray(counts, np.uint32)
        newp, branch = np.zeros(1056, np.uint8), np.zeros((1056, 2), np.uint32)
        s = L.adapt_ref_savings(c32.ctypes.data, np.ascontiguousarray(base).ctypes.data, newp.ctypes.data, branch.ctypes.data)
        savings.append({"name": name, "counts": {str(i): int(c32[i]) for i in np.flatnonzero(c32)},
                        "base": "default" if np.array_equal(base, A.default_probs()[:1056]) else base.tolist(), "newp": newp.tolist(), "saving": int(s)})
        for row in (0, 37, 95):                              # three contexts of every case through the tree function itself
            probs, br = np.zeros(11, np.uint8), np.zeros((11, 2), np.uint32)
            c12 = np.ascontiguousarray(c32[row * 12:row * 12 + 12])
            L.adapt_ref_tree(c12.ctypes.data, probs.ctypes.data, br.ctypes.data)
            assert np.array_equal(probs, newp[row * 11:row * 11 + 11]) and np.array_equal(br, branch[row * 11:row * 11 + 11])
            tree.append({"counts": c12.tolist(), "probs": probs.tolist(), "branch": br.tolist()})
    for name, events, before in mv_cases():
        e32 = np.ascontiguousarray(events, np.uint32)
        ctx, buf = np.ascontiguousarray(before).copy(), np.zeros(256, np.uint8)
        n = L.adapt_ref_mvprobs(e32.ctypes.data, ctx.ctypes.data, buf.ctypes.data, buf.size)
        assert 0 < n <= buf.size
        mv.append({"name": name, "events": {str(k): {str(int(i) - 1023): int(e32[k, i]) for i in np.flatnonzero(e32[k])} for k in range(2)},
                   "before": before.tolist(), "after": ctx.tolist(), "bytes": buf[:n].tobytes().hex()})
    with open(os.path.join(HERE, "pack_adapt_ref.json"), "w") as f:
        f.write('{"what": "the reference\'s vp8_prob_cost, vp8_tree_probs_from_distribution over vp8_coef_tree, vp8_estimate_entropy_savings '
                '(key frame, no error resilience) and vp8_write_mvprobs on the count sets of make_pack_adapt_fixtures.py",\n "cost": ')
        f.write(json.dumps(cost.tolist(), separators=(",", ":")))
        for key, rows in (("tree", tree), ("savings", savings), ("mv", mv)):
            f.write(f',\n "{key}": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ]")
        f.write("}\n")


if __name__ == "__main__":
    main()
