"""Dev aid (GPU): vp8hip_frames_side_async on a batch of IR slots holding p_dense_1920x1080's frames -- and, in the same run, the
yardsticks it is held against: frames_rgb for the same number of frames at the same size with planar floats (three planes of
floats where the flow writes two) and the scaler's display-size copy, both from kf_1920x1080 frames left as tiles by one launch.
Device events around each call after warm-up; TB/s by the byte model: records (128 bytes a macroblock: the line the 64 bytes read
lie in) and vectors (64) read, plus the destination bytes.  One destination is held at a time.
   python3 tools/side_time.py [slots (8192, or as many as fit beside the largest destination)] [timed calls (20)] [--out FILE]"""
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
# (width, height; 0: the native grid), type of the vectors, planes
CALLS = ((1920, 1080, "f32", ()), (1920, 1080, "f16", ()), (1920, 1080, "i16", ()), (1920, 1080, "f32", ("ref", "mode", "skip")),
         (1920, 1080, None, ("ref", "mode", "skip", "segment", "qindex", "coded")), (0, 0, "i16", ("ref", "mode", "skip")), (224, 224, "f32", ("ref", "mode", "skip")))


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
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
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
    ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)       # the yardsticks' frames: left as tiles
    ctx.sync()
    parser = P.Parser()
    kinds = []
    for i, data in enumerate(frames[:n]):                           # the slots: the inter stream's frames, over and over
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
        kinds.append("key" if hdr.frame_type == 0 else "inter")
    parser.close()
    for i in range(len(frames), n):
        ctx.ir_copy(i, i % len(frames))
    ctx.sync()
    before = ctx.memory_usage()
    say(f"p_dense_1920x1080 ({', '.join(kinds)}) x {n} slots; kf_1920x1080 x {n} frame buffers as tiles; {reps} timed calls after 3; memory {before}")
    slots = fbs = list(range(n))
    src_side = nmb * (128 + 64)
    per_byte = {}

    out = torch.empty((n, S.i420_size(w, h)), dtype=torch.uint8, device="cuda:0")
    ms = timed(lambda: ctx.frames_scaled(fbs, w, h, 1, out=out), 3, reps)
    gb = byte_model(w, h, w, h, 1) * n / 1e9
    dst = out[0].numel() * n
    say(f"yardstick  {w}x{h} I420 copy (frames_scaled):       {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, "
        f"{ms * 1e9 / dst:7.4f} ps per destination byte")
    del out
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda:0")
    ms = timed(lambda: ctx.frames_rgb(fbs, w, h, 1, dtype=torch.float32, out=out), 3, reps)
    dst = out[0].numel() * 4 * n
    gb = ((byte_model(w, h, w, h, 1) - S.i420_size(w, h)) * n + dst) / 1e9
    per_byte["rgb"] = ms / dst
    say(f"yardstick  {w}x{h} nchw f32 (frames_rgb):            {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, "
        f"{ms * 1e9 / dst:7.4f} ps per destination byte")
    del out
    torch.cuda.empty_cache()

    for dw, dh, dtype, planes in CALLS:
        gw, gh = (dw, dh) if dw else (4 * ((w + 15) // 16), 4 * ((h + 15) // 16))
        size = dict(width=dw, height=dh) if dw else {}
        mv = torch.empty((n, 2, gh, gw), dtype=TORCH[dtype], device="cuda:0") if dtype else False
        info = torch.empty((n, len(planes), gh, gw), dtype=torch.uint8, device="cuda:0") if planes else False
        ms = timed(lambda: ctx.frames_side(slots, mv_dtype=TORCH[dtype or "i16"], planes=planes, scale="pixels" if dtype != "i16" else None,
                                           out_mv=mv, out_info=info, **size), 3, reps)
        dst = ((mv[0].numel() * mv.element_size() if dtype else 0) + (info[0].numel() if planes else 0)) * n
        gb = (src_side * n + dst) / 1e9
        what = f"{gw}x{gh}{'' if dw else ' (native)'} mv {dtype or '-'} + {len(planes)} planes"
        say(f"frames_side {what:42s} {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")
        if (dw, dh, dtype, planes) == CALLS[0]:
            per_byte["flow"] = ms / dst
        del mv, info
        torch.cuda.empty_cache()
    ratio = per_byte["flow"] / per_byte["rgb"]
    say(f"display-size float flow against frames_rgb, time per destination byte: {ratio:.3f} (expected: at most 1.15)")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
