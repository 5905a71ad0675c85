"""Fixtures of the decoder's debug overlays (vp8/common/postproc.c:1007-1362, CONFIG_POSTPROC_VISUALIZER): what the REFERENCE
decoder shows with `vpxdec --pp-debug-info / --pp-dbg-*`, and the numbers its overlays are drawn with.

    python tests/golden/make_vis_fixtures.py <dir with a visualizer build's libvpxref.so and vpxdec_ref>

The build the argument names is made like oracle/_ref's, with two changes to a scratch copy of oracle/Makefile:
    --enable-postproc-visualizer   on the configure line, and
    textblit                       added to COMMON
then `make _ref/vpxdec_ref` (the visualizer is not part of oracle/_ref, which the rest of the suite pins).

Writes, next to this file:
    <stream>.vis_<tag>.md5   one line per shown frame ("<md5>  f-NNNN.i420": vpxdec -o 'f-%4.i420' --md5 --i420)
    vis.vpxdec_md5           "<stream> <md5> <options...>": one digest over the whole output of vpxdec --md5 --i420
    vis_tables.json          the glyph of every character (vp8_blit_text on blank buffers) and the colour triples the
                             overlays blend with (the static arrays of postproc.o, read from the library's symbol table)
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

# tag -> vpxdec options.  The --pp-dbg-* tags alone leave VP8_SET_POSTPROC unset, so the decoder runs its default
# configuration (deblock + demacroblock + MFQE, vp8_dx_iface.c:421-431) under the overlays; on sizes that are not multiples
# of 16 the reference dies in that configuration (make_fixtures.py), so those streams get --deblock with them (EXTRA).
TAGS = {
    "info8": ["--pp-debug-info=8"],
    "info16": ["--pp-debug-info=16"],
    "info32": ["--pp-debug-info=32"],
    "info64": ["--pp-debug-info=64"],
    "info120": ["--pp-debug-info=120"],
    "mvs1023": ["--pp-dbg-mvs=1023"],
    "mbmodes1023": ["--pp-dbg-mb-modes=1023"],
    "mbmodes4": ["--pp-dbg-mb-modes=4"],
    "bmodes1023": ["--pp-dbg-b-modes=1023"],
    "ref15": ["--pp-dbg-ref-frame=15"],
    "all_mfqe": ["--mfqe", "--pp-debug-info=120", "--pp-dbg-mvs=1023", "--pp-dbg-mb-modes=1023", "--pp-dbg-b-modes=1023",
                 "--pp-dbg-ref-frame=15"],
}
STREAMS = ("p_arf_176x144", "p_split_352x288", "p_odd_130x98", "kf_odd_67x45", "kf_640x360", "p_1920x1080")
EXTRA = ["--deblock"]
# whole-stream digests of vpxdec with the options as a user types them
CLI = (("p_split_352x288", ["--pp-dbg-mvs=1023"]), ("p_split_352x288", ["--pp-dbg-mb-modes=1023"]),
       ("p_split_352x288", ["--pp-dbg-ref-frame=15"]), ("p_split_352x288", ["--pp-dbg-b-modes=1023", "--pp-dbg-mvs=0"]),
       ("kf_odd_67x45", ["--pp-debug-info=120"]), ("kf_640x360", ["--deblock", "--pp-dbg-b-modes=1023", "--pp-debug-info=16"]),
       ("p_arf_176x144", ["--mfqe", "--pp-debug-info=121", "--pp-dbg-mvs=1023", "--pp-dbg-ref-frame=15"]),
       ("p_odd_130x98", ["--pp-debug-info=9", "--pp-dbg-mvs=992", "--pp-dbg-mb-modes=1023"]))


def aligned16(name):
    w, h = (int(v) for v in name.rsplit("_", 1)[1].split("x"))
    return w % 16 == 0 and h % 16 == 0


def tag_args(name, tag):
    a = TAGS[tag]
    if not aligned16(name) and not any(x.startswith("--pp-debug-info") for x in a):
        a = a + EXTRA
    return a


def tables(build):
    lib = os.path.join(build, "libvpxref.so")
    L = ctypes.CDLL(lib)
    glyphs = [0] * 256
    pitch = 16
    for code in range(1, 256):
        buf = (ctypes.c_ubyte * (pitch * 5))(*([0x55] * (pitch * 5)))
        L.vp8_blit_text(bytes([code]), buf, pitch)
        bits = 0
        for r in range(5):
            for c in range(pitch):
                v = buf[r * pitch + c]
                assert (c < 7 and v in (0, 255)) or (c >= 7 and v == 0x55), (code, r, c, v)
                if c < 7 and v == 255:
                    bits |= 1 << (r * 7 + c)
        glyphs[code] = bits
    # the colour arrays are static: their addresses in the symbol table, read out of the loaded library
    syms = {}
    for line in subprocess.run(["nm", "-S", lib], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 4:
            syms[f[3]] = (int(f[0], 16), int(f[1], 16))
    base = ctypes.cast(L.vp8_blit_text, ctypes.c_void_p).value - syms["vp8_blit_text"][0]
    colours = {}
    for name in ("MB_PREDICTION_MODE_colors", "B_PREDICTION_MODE_colors", "MV_REFERENCE_FRAME_colors"):
        addr, size = syms[name]
        raw = ctypes.string_at(base + addr, size)
        colours[name] = [list(raw[i:i + 3]) for i in range(0, size, 3)]
    return {"glyph_bits": "bit r*7+c set: row r (0..4), column c (0..6) of the character's cell is 255, else 0",
            "glyphs": glyphs, "mb_mode_colours": colours["MB_PREDICTION_MODE_colors"],
            "b_mode_colours": colours["B_PREDICTION_MODE_colors"], "ref_frame_colours": colours["MV_REFERENCE_FRAME_colors"]}


def main():
    build = sys.argv[1]
    vpxdec = os.path.join(build, "vpxdec_ref")
    with open(os.path.join(HERE, "vis_tables.json"), "w") as f:
        json.dump(tables(build), f, indent=1)
        f.write("\n")
    for name in STREAMS:
        ivf = os.path.join(HERE, name + ".ivf")
        for tag in TAGS:
            r = subprocess.run([vpxdec, "--md5", "--i420", "-o", "f-%4.i420", *tag_args(name, tag), ivf],
                               capture_output=True, text=True, check=True, cwd="/tmp")
            with open(os.path.join(HERE, f"{name}.vis_{tag}.md5"), "w") as f:
                f.write(r.stdout)
    with open(os.path.join(HERE, "vis.vpxdec_md5"), "w") as f:
        for name, args in CLI:
            r = subprocess.run([vpxdec, *args, "--md5", "--i420", os.path.join(HERE, name + ".ivf")], capture_output=True, text=True,
                               check=True)
            f.write(f"{name} {r.stdout.split()[0]} {' '.join(args)}\n")


if __name__ == "__main__":
    main()
