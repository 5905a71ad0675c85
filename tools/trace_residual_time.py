"""Dev aid (GPU): vp8hip_trace_residual_async on a batch of p_dense_1920x1080 frames left as tiles by large launches -- the key frame
into one half of the frame buffers (the anchors), the first inter frame into the other half, every job with an anchor and a one-hop
trace of its own, so that what it reads comes from HBM as it would for streams in lock step -- at the display size and at 224x224,
as halves.  In the same run the two yardsticks it is held against, neither of which is the code under test:
  (1) the torch formulation a caller had before the call existed: frames_rgb halves at the display size, int64 coordinates from the
      trace, a flat gather from the anchor's RGB halves (made once, outside the timing: the caller keeps them for the group) and a
      subtraction -- then F.interpolate(mode="nearest") for 224x224 --, a chunk of frames at a time so that its temporaries fit;
  (2) frames_rgb alone, planar halves at the display size: the same tensor written, the current frame only read.
Device events around each side after warm-up; GB by the byte model: trace 4 bytes a pixel, frame and anchor 1.5 each, destination 6.
   python3 tools/trace_residual_time.py [jobs (512, or as many as fit)] [timed calls (20)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

CHUNK = 16              # frames per step of the torch route (an int64 index of 17 MB a frame, the gathered anchor beside it)


def torch_route(ctx, pool, fbs, entries, anchors, out, small=None):
    """yardstick (1): out[i] = rgb(fbs[i]) - anchors[i] gathered at pool[entries[i]]; small: the same, nearest-sampled to its size"""
    w = ctx.width
    for i0 in range(0, len(fbs), CHUNK):
        cur = ctx.frames_rgb(fbs[i0:i0 + CHUNK], dtype=torch.float16, out=out[i0:i0 + CHUNK])          # [c, 3, d_h, d_w]
        t = pool[entries[i0]:entries[i0] + cur.shape[0]].to(torch.int64)                                # [c, d_h, d_w, 2]
        idx = (t[..., 1] * w + t[..., 0]).flatten(1)[:, None, :].expand(-1, 3, -1)
        cur -= anchors[i0:i0 + CHUNK].flatten(2).gather(2, idx).view_as(cur)
        if small is not None:
            small[i0:i0 + CHUNK] = F.interpolate(cur, size=small.shape[2:], mode="nearest")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    reps = int(args[1]) if len(args) > 1 else 20
    P = load_package()
    os.environ["VP8HIP_RECON"] = "simt"
    name = "p_dense_1920x1080"
    w, h, frames = P.read_ivf(ivf_path(name))
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    px = w * h
    # a job: a slot, two frame buffers as tiles, a trace, the anchor's RGB halves (yardstick 1) and a destination
    per_job = nmb * 960 + 2 * nmb * 420 + 4 * px + 6 * px + 6 * px
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(512, int(free * 0.8) // per_job)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, 2 * n, n + 2)
    parser = P.Parser()
    for k in range(2):                                  # the key frame in slot n, the first inter frame in slot n + 1
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, frames[k], n + k)
        parser.swap(hdr)
        assert hdr.frame_type == k
    parser.close()
    pool = ctx.trace_pool(n + 1)
    ctx.frames_trace([(n, n, None)], pool)              # entry n: the identity
    for k in range(2):                                  # anchors in frame buffers 0 .. n - 1, the frames in n .. 2n - 1: one launch each
        for i in range(n):
            ctx.ir_copy(i, n + k)
        jobs = [(i, i, None) for i in range(n)] if k == 0 else [(i, n + i, (i, i, i)) for i in range(n)]
        ctx.decode(jobs, P.STAGE_ALL)
    ctx.frames_trace([(i, i, (n, n, n)) for i in range(n)], pool)       # entries 0 .. n - 1: job i's own one-hop trace
    ctx.sync()
    before = ctx.memory_usage()
    moved = float((pool[0] != pool[n]).any(-1).float().mean())
    say(f"{name} (key, inter) x {n} jobs, frames left as tiles (raster pool {before['raster_pool']} bytes); {reps} timed calls after 3; "
        f"{100 * moved:.1f}% of a trace's pixels moved; memory {before}")
    jobs = [(n + i, i, i) for i in range(n)]
    cur_fbs, entries = [n + i for i in range(n)], list(range(n))

    def row(what, ms, gb):
        say(f"{what:64s} {ms:9.3f} ms per call of {n} jobs, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s")
        return ms

    out = torch.empty((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    small = torch.empty((n, 3, 224, 224), dtype=torch.float16, device="cuda:0")
    gb_full = (4 + 1.5 + 1.5 + 6) * px * n / 1e9
    gb_small = (4 + 1.5 + 1.5 + 6) * 224 * 224 * n / 1e9        # (what it asks for; whole sectors come)
    ms = {}
    ms["rgb"] = row(f"yardstick (2)  frames_rgb {w}x{h} nchw float16", timed(lambda: ctx.frames_rgb(cur_fbs, dtype=torch.float16, out=out), 3, reps),
                    (1.5 + 6) * px * n / 1e9)
    ms["full"] = row(f"trace_residual {w}x{h} float16",
                     timed(lambda: ctx.trace_residual(pool, jobs, dtype=torch.float16, scale=1 / 255, out=out), 3, reps), gb_full)
    ms["small"] = row("trace_residual 224x224 float16",
                      timed(lambda: ctx.trace_residual(pool, jobs, 224, 224, dtype=torch.float16, scale=1 / 255, out=small), 3, reps), gb_small)
    assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0
    anchors = torch.empty((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    ctx.frames_rgb(list(range(n)), dtype=torch.float16, out=anchors)
    ms["torch_full"] = row(f"yardstick (1)  frames_rgb + torch gather, subtract {w}x{h}, {CHUNK} frames a step",
                           timed(lambda: torch_route(ctx, pool, cur_fbs, entries, anchors, out), 1, reps), gb_full)
    ms["torch_small"] = row("yardstick (1)  ... + F.interpolate nearest to 224x224",
                            timed(lambda: torch_route(ctx, pool, cur_fbs, entries, anchors, out, small), 1, reps), gb_small)
    say(f"yardstick (1) against trace_residual: {ms['torch_full'] / ms['full']:.2f} x at {w}x{h}, {ms['torch_small'] / ms['small']:.1f} x at 224x224")
    say(f"trace_residual against yardstick (2) at {w}x{h}: {ms['full'] / ms['rgb']:.2f} x the time (byte model: 1.73 x the bytes)")
    say(f"memory {ctx.memory_usage()}")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
