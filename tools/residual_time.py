"""Dev aid (GPU): vp8hip_frames_residual_async on a batch of IR slots holding p_dense_1920x1080's frames -- and, in the same run, the
yardsticks it is held against, neither of them the code under test: frames_rgb for the same number of frames at 1920x1080 with
planar floats, which writes exactly the bytes the planar float residual writes (from kf_1920x1080 frames left as tiles by one
launch), and frames_side's display-size float flow over the same slots.  Device events around each call after warm-up; TB/s by
the byte model: records (128 bytes a macroblock) and 32 bytes for every block the slots really hold, plus the destination bytes.
One destination is held at a time.
   python3 tools/residual_time.py [slots (8192, or as many as fit beside the largest destination)] [timed calls (20)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import scale_reference as S  # noqa: E402
from rgb_time import timed  # noqa: E402
from scale_time import byte_model  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

TORCH = {"i16": torch.int16, "f16": torch.float16, "f32": torch.float32}
# (width, height; 0: the native grid), type, layout
CALLS = ((1920, 1080, "f32", "planar"), (1920, 1080, "f16", "planar"), (1920, 1080, "i16", "planar"), (0, 0, "i16", "i420"), (1920, 1080, "i16", "i420"),
         (224, 224, "f32", "planar"))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    reps = int(args[1]) if len(args) > 1 else 20
    P = load_package()
    os.environ["VP8HIP_RECON"] = "simt"
    w, h, key_frames = P.read_ivf(ivf_path("kf_1920x1080"))
    w2, h2, frames = P.read_ivf(ivf_path("p_dense_1920x1080"))
    assert (w, h) == (w2, h2)
    cols, rows = (w + 15) // 16, (h + 15) // 16
    nmb = cols * rows
    # a slot (960 bytes a macroblock), a frame as tiles, and the largest destination held (planar floats): what a frame costs
    per_frame = nmb * 960 + nmb * 420 + 3 * w * h * 4
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(8192, int(free * 0.9) // per_frame)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, n, n)
    parser = P.Parser()
    for i, data in enumerate(key_frames[:n]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
    parser.close()
    for i in range(len(key_frames), n):
        ctx.ir_copy(i, i % len(key_frames))
    ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)       # the yardstick's frames: left as tiles
    ctx.sync()
    parser = P.Parser()
    kinds, nblocks = [], []
    for i, data in enumerate(frames[:n]):                           # the slots: the inter stream's frames, over and over
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
    say(f"p_dense_1920x1080 ({', '.join(kinds)}; blocks per frame {nblocks}) x {n} slots; kf_1920x1080 x {n} frame buffers as tiles; "
        f"{reps} timed calls after 3; memory {before}")
    slots = fbs = list(range(n))
    src = nmb * 128 * n + blocks * 32
    per_byte, model = {}, {}

    out = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda:0")
    ms = timed(lambda: ctx.frames_rgb(fbs, w, h, 1, dtype=torch.float32, out=out), 3, reps)
    dst = out[0].numel() * 4 * n
    gb = ((byte_model(w, h, w, h, 1) - S.i420_size(w, h)) * n + dst) / 1e9
    per_byte["rgb"], model["rgb"] = ms / dst, gb
    say(f"yardstick  {w}x{h} nchw f32 (frames_rgb):                 {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, "
        f"{ms * 1e9 / dst:7.4f} ps per destination byte")
    del out
    torch.cuda.empty_cache()
    mv = torch.empty((n, 2, h, w), dtype=torch.float32, device="cuda:0")
    ms = timed(lambda: ctx.frames_side(slots, width=w, height=h, mv_dtype=torch.float32, planes=(), scale="pixels", out_mv=mv, out_info=False), 3, reps)
    dst = mv[0].numel() * 4 * n
    gb = (nmb * (128 + 64) * n + dst) / 1e9
    say(f"yardstick  {w}x{h} float flow (frames_side):              {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, "
        f"{ms * 1e9 / dst:7.4f} ps per destination byte")
    del mv
    torch.cuda.empty_cache()

    for dw, dh, dtype, layout in CALLS:
        gw, gh = (dw, dh) if dw else (16 * cols, 16 * rows)
        size = dict(width=dw, height=dh) if dw else {}
        elems = 3 * gh * gw if layout == "planar" else gh * gw + 2 * ((gh + 1) // 2) * ((gw + 1) // 2)
        out = torch.empty((n, 3, gh, gw) if layout == "planar" else (n, elems), dtype=TORCH[dtype], device="cuda:0")
        ms = timed(lambda: ctx.frames_residual(slots, dtype=TORCH[dtype], layout=layout, scale=(1.0 / 255, 1.0 / 255, 1.0 / 255), out=out, **size), 3, reps)
        dst = elems * out.element_size() * n
        gb = (src + dst) / 1e9
        what = f"{gw}x{gh}{'' if dw else ' (native)'} {layout} {dtype}"
        say(f"frames_residual {what:36s} {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")
        if (dw, dh, dtype, layout) == CALLS[0]:
            per_byte["res"], model["res"] = ms / dst, gb
        del out
        torch.cuda.empty_cache()
    ratio, models = per_byte["res"] / per_byte["rgb"], model["res"] / model["rgb"]
    say(f"planar float residual against frames_rgb, time per destination byte: {ratio:.3f}; byte-model ratio {models:.3f}; "
        f"against the limit (frames_rgb's time per byte x the byte-model ratio): {ratio / models:.3f} (expected: at most 1.15)")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
