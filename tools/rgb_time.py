"""Dev aid (GPU): vp8hip_frames_rgb_async on a batch of kf_1920x1080 frames left as tiles by one launch, then the same calls from
the raster form -- and, in the same run, the route a caller had before the call existed: frames_scaled to the same size followed by
the torch operations that make the same tensor (plane split, repeat_interleave of the chroma, the matrix in integers, clamp,
type conversion, normalisation), a chunk of frames at a time so that its temporaries fit beside the batch.  Device events around
each call; TB/s by the byte model (the source rows the scaler's plan reads, tools/scale_time.py, plus the destination bytes).
One destination is held at a time: the two full-size ones are 51 and 68 GB beside the slots and the frames.
   python3 tools/rgb_time.py [frames (8192)] [timed calls (20)] [timed calls of the torch route (as the former)] [--check]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import rgb_reference as R  # noqa: E402
import scale_reference as S  # noqa: E402
from scale_time import byte_model  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

# (width, height, filter, layout, dtype)
CALLS = ((1920, 1080, 1, "nchw", "u8"), (1920, 1080, 1, "nhwc4", "u8"), (960, 540, 1, "nchw", "u8"), (224, 224, 1, "nchw", "f32"),
         (224, 224, 1, "nchw", "f16"))
TORCH = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
CHUNK = 256             # frames per step of the torch route


def torch_route(P, ctx, fbs, dw, dh, f, layout, dtype, out):
    """frames_scaled + torch: the same tensor as frames_rgb(matrix="bt601", order="rgb", ImageNet mean / std for the float types)"""
    yoff, cy, crv, cgu, cgv, cbu = R.MATRICES["bt601"]
    scale, bias = R.scale_bias(R.IMAGENET_MEAN, R.IMAGENET_STD)
    for i0 in range(0, len(fbs), CHUNK):
        t = ctx.frames_scaled(fbs[i0:i0 + CHUNK], dw, dh, f)
        y, u, v = P.split_i420(t, dw, dh)
        up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :dh, :dw].to(torch.int32) - 128
        u, v = up(u), up(v)
        l = cy * (y.to(torch.int32) - yoff) + 128
        chans = (((l + crv * v) >> 8).clamp_(0, 255), ((l + cgu * u + cgv * v) >> 8).clamp_(0, 255), ((l + cbu * u) >> 8).clamp_(0, 255))
        o = out[i0:i0 + CHUNK]
        for c in range(3):
            val = chans[c] if dtype == "u8" else chans[c].to(torch.float32) * float(scale[c]) + float(bias[c])
            if layout == "nchw":
                o[:, c] = val
            else:
                o[..., c] = val
        if layout == "nhwc4":
            o[..., 3] = 255


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    reps = int(args[1]) if len(args) > 1 else 20
    reps_torch = int(args[2]) if len(args) > 2 else reps
    check = "--check" in sys.argv
    P = load_package()
    os.environ["VP8HIP_RECON"] = "simt"
    name = "kf_1920x1080"
    w, h, frames = P.read_ivf(ivf_path(name))
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, n, n)
    parser = P.Parser()
    for i, data in enumerate(frames[:n]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
    parser.close()
    for i in range(len(frames), n):
        ctx.ir_copy(i, i % len(frames))
    ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)
    ctx.sync()
    st = ctx.stats()
    print(f"{name} x {n}: one launch, recon {st.recon_ms:.2f} ms; memory {ctx.memory_usage()}")
    print(f"timed calls: {reps} after 3 (frames_rgb, frames_scaled), {reps_torch} after 1 (frames_scaled + torch, {CHUNK} frames a step)")
    fbs = list(range(n))
    norm = dict(mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    for form in ("tiles", "raster"):
        if form == "raster":
            ctx.frames_to_raster(0, n)
            ctx.sync()
        # the scaler's copy at the display size: the same read side, half the destination bytes per byte read
        out = torch.empty((n, S.i420_size(w, h)), dtype=torch.uint8, device="cuda:0")
        ms = timed(lambda: ctx.frames_scaled(fbs, w, h, 1, out=out), 3, reps)
        gb = byte_model(w, h, w, h, 1) * n / 1e9
        print(f"from {form:6s} {w}x{h} I420 copy (frames_scaled): {ms:8.3f} ms per call of {n} frames, {gb:6.2f} GB, {gb / ms:6.3f} TB/s")
        del out
        for dw, dh, f, layout, dtype in CALLS:
            shape = (n, 3, dh, dw) if layout == "nchw" else (n, dh, dw, 4 if layout == "nhwc4" else 3)
            out = torch.empty(shape, dtype=TORCH[dtype], device="cuda:0")
            kw = norm if dtype != "u8" else {}
            ms = timed(lambda: ctx.frames_rgb(fbs, dw, dh, f, dtype=TORCH[dtype], layout=layout, out=out, **kw), 3, reps)
            src = byte_model(w, h, dw, dh, f) - S.i420_size(dw, dh)
            gb = (src + out[0].numel() * out.element_size()) * n / 1e9
            if check:
                got = out[:CHUNK].clone()
            ms_t = timed(lambda: torch_route(P, ctx, fbs, dw, dh, f, layout, dtype, out), 1, reps_torch)
            note = ""
            if check:
                same = torch.equal(got, out[:CHUNK]) if dtype == "u8" else bool(((got.float() - out[:CHUNK].float()).abs() <= (2e-3 if dtype == "f16" else 1e-6)).all())
                note = f"; first {CHUNK} frames {'equal' if same else 'DIFFER'}"
            print(f"from {form:6s} {dw}x{dh} f{f} {layout} {dtype}: {ms:8.3f} ms per call of {n} frames, {gb:6.2f} GB by the byte model, "
                  f"{gb / ms:6.3f} TB/s; frames_scaled + torch: {ms_t:9.3f} ms, {gb / ms_t:6.3f} TB/s, {ms_t / ms:6.1f} x{note}")
            del out
            torch.cuda.empty_cache()
    print(f"scratch {ctx.rgb_scratch_bytes()} bytes; memory {ctx.memory_usage()}")
    ctx.close()


if __name__ == "__main__":
    main()
