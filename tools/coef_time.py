"""Dev aid (GPU): vp8hip_frames_coef_async on a batch of IR slots holding p_dense_1920x1080's frames -- tools/residual_time.py's slots --
and, in the same process over the same slots, its yardstick: frames_residual on the native grid, I420, int16, which reads the same
bytes as the int16 Y|U|V call, writes the same number and does the inverse DCT on top.  Device events around each call after
warm-up; the three that are compared run in A B C C B A order and both passes are printed.  TB/s by the byte model: records (128
bytes a macroblock) and 32 bytes for every block the slots really hold, plus the destination bytes.  One destination is held at a
time.
   python3 tools/coef_time.py [slots (2048, or as many as fit beside the largest destination)] [timed calls (20)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

TORCH = {"i16": torch.int16, "f16": torch.float16, "f32": torch.float32}
PLANES = ("y", "u", "v")
# layout, type, nfreq, order: after the compared pair, the same as floats and the first six of the scan
MORE = (("channels", "f32", 16, "raster"), ("inplace", "f32", 16, "raster"), ("channels", "f16", 16, "raster"), ("channels", "i16", 6, "zigzag"),
        ("channels", "f32", 6, "zigzag"))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    reps = int(args[1]) if len(args) > 1 else 20
    P = load_package()
    w, h, frames = P.read_ivf(ivf_path("p_dense_1920x1080"))
    cols, rows = (w + 15) // 16, (h + 15) // 16
    nmb = cols * rows
    per_frame = nmb * 960 + nmb * 384 * 4          # a slot, and the largest destination held (floats)
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(2048, int(free * 0.9) // per_frame)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, 1, n)
    parser = P.Parser()
    kinds, nblocks = [], []
    for i, data in enumerate(frames[:n]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
        kinds.append("key" if hdr.frame_type == 0 else "inter")
        ctx.sync()
        mbs, _ = ctx.ir_fetch(i)
        nblocks.append(int((P.block_kinds(mbs)[:, :24] == 2).sum()))       # blocks of 32 bytes in the slot's stream
    parser.close()
    for i in range(len(frames), n):
        ctx.ir_copy(i, i % len(frames))
    ctx.sync()
    before = ctx.memory_usage()
    blocks = sum(nblocks[i % len(nblocks)] for i in range(n))
    say(f"p_dense_1920x1080 ({', '.join(kinds)}; blocks per frame {nblocks}) x {n} slots; {reps} timed calls after 3; memory {before}")
    slots = list(range(n))
    src = nmb * 128 * n + blocks * 32
    elems = 384 * nmb

    def report(what, ms, dst):
        gb = (src + dst) / 1e9
        say(f"{what:52s} {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")

    def coef(layout, dtype, nfreq, order, out):
        return lambda: ctx.frames_coef(slots, "dequant", layout, PLANES, nfreq, order, TORCH[dtype], 1.0 / 255, out=out)

    # the compared three, int16 into one destination of the same size: A B C C B A
    out = torch.empty((n, elems), dtype=torch.int16, device="cuda:0")
    calls = {"yardstick": lambda: ctx.frames_residual(slots, layout="i420", out=out), "channels": coef("channels", "i16", 16, "raster", out),
             "inplace": coef("inplace", "i16", 16, "raster", out)}
    names = {"yardstick": "frames_residual native i420 i16 (the yardstick)", "channels": "frames_coef dequant channels i16 y|u|v nfreq 16",
             "inplace": "frames_coef dequant inplace i16 y|u|v"}
    ms = {k: [] for k in calls}
    for k in ("yardstick", "channels", "inplace", "inplace", "channels", "yardstick"):
        ms[k].append(timed(calls[k], 3, reps))
        report(names[k], ms[k][-1], elems * 2 * n)
    del out
    torch.cuda.empty_cache()
    for layout, dtype, nfreq, order in MORE:
        e = elems * nfreq // 16
        out = torch.empty((n, e), dtype=TORCH[dtype], device="cuda:0")
        t = timed(coef(layout, dtype, nfreq, order, out), 3, reps)
        report(f"frames_coef dequant {layout} {dtype} y|u|v nfreq {nfreq} {order}", t, e * out.element_size() * n)
        del out
        torch.cuda.empty_cache()
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    for k in ("channels", "inplace"):
        say(f"{k} against the yardstick in the same run, means of the two passes: {mean[k]:.3f} / {mean['yardstick']:.3f} = "
            f"{mean[k] / mean['yardstick']:.3f} (expected: at most 1.15)")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
