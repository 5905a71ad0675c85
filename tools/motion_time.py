"""Dev aid (GPU): the block motion search between pictures at 1920x1080 (8160 macroblocks a pair), d = 16, over 1 job and over a batch
(1024), and, in the same process, what it is held against, which is not the code under test:
  frames_motion, vectors only          -- the search and the reduction;
  frames_motion, vectors and 5 planes  -- plus the second pass over the winner;
  frames_ssim scores                   -- over the same jobs: the nearest neighbour in bytes read;
  the torch formulation the call replaces, for scale: frames_scaled of both pictures, the reference picture padded by
      replication, and per candidate a shifted |s - r| pooled over the macroblocks (avg_pool2d 16x16), kept where strictly smaller
      -- the centre first, then raster order; over 1 and 8 jobs (a candidate is half a dozen launches over the whole picture).
Then d = 8, 32 and 64 on the decoded content (64: over 64 jobs).  The pictures come in three contents: kf_1920x1080's decoded key
frames -- as the tiles a large launch leaves and, after vp8hip_frames_to_raster, as raster --, uniform noise and identical pictures
(uploaded: raster).  The sides of a comparison alternate over two rounds, and both rounds are printed: their difference is the
spread.  Device events around each call after warm-up.  The last lines put the call's rate beside the model: candidates * 64
dword-SADs / 4 a v_qsad_pk_u16_u8, per wave of 64 lanes.
   python3 tools/motion_time.py [frames (1024)] [timed calls (5)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_motion(P, ctx, pairs, w, h, d):
    """the formulation frames_motion replaces: -> (mv int16 [n, 2, rows, cols] in 1/8 pel, sad int32 [n, rows, cols]) over the
    macroblock rows and columns the display size covers whole, zero centre, no cost, no UMV bound (none bites for d <= 16)"""
    pool = torch.nn.functional.avg_pool2d
    rows, cols = h // 16, w // 16
    s = P.split_i420(ctx.frames_scaled([p[0] for p in pairs]), w, h)[0][:, :16 * rows, :16 * cols].float()[:, None]
    r = P.split_i420(ctx.frames_scaled([p[1] for p in pairs]), w, h)[0].float()[:, None]
    r = torch.nn.functional.pad(r, (d, d + 16, d, d + 16), mode="replicate")

    def sad(dy, dx):
        win = r[:, :, d + dy:d + dy + 16 * rows, d + dx:d + dx + 16 * cols]
        return (pool((s - win).abs(), 16) * 256)[:, 0].round().int()
    best = sad(0, 0)
    by, bx = torch.zeros_like(best), torch.zeros_like(best)
    for dy in range(-d, d):
        for dx in range(-d, d):
            v = sad(dy, dx)
            less = v < best
            best = torch.where(less, v, best)
            by = torch.where(less, torch.full_like(by, dy), by)
            bx = torch.where(less, torch.full_like(bx, dx), bx)
    return (torch.stack((bx, by), 1) << 3).short(), best


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 1024
    reps = int(args[1]) if len(args) > 1 else 5
    P = load_package()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    times = {}

    def row(key, what, fn, r=None):
        ms = timed(fn, 1, reps if r is None else r)
        times.setdefault(key, []).append(ms)
        say(f"{what:86s} {ms:10.4f} ms per call")
        return ms

    def mean(key):
        return sum(times[key]) / len(times[key])

    os.environ["VP8HIP_RECON"] = "simt"                 # the large launch's kernels: frames left as tiles
    w, h, frames = P.read_ivf(ivf_path("kf_1920x1080"))
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
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    nmb = rows * cols
    say(f"kf_1920x1080 x {n} frame buffers, {nmb} macroblocks a pair; {reps} timed calls after 1 (the torch formulation: 1 after 1); "
        f"memory {ctx.memory_usage()}")
    rng = np.random.default_rng(7)
    g = ctx.g

    def motion(pairs, d, planes, mv, st):
        return lambda: ctx.frames_motion(pairs, d, planes=planes, out_mv=mv, out_stats=st if planes else None)

    def measure(content, form, with_torch):
        for m in (1, n):
            pairs = [(i, (i + 1) % n) for i in range(m)]
            mv = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
            st = torch.empty((m, 5, rows, cols), dtype=torch.int32, device="cuda:0")
            sc = torch.empty((m, 3, 2), dtype=torch.int64, device="cuda:0")
            for rnd in range(2):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                row(("ssim", content, form, m), f"yardstick  frames_ssim scores          {tag}", lambda: ctx.frames_ssim(pairs, out_scores=sc))
                row(("mv", content, form, m), f"frames_motion d 16, vectors            {tag}", motion(pairs, 16, (), mv, st))
                row(("all", content, form, m), f"frames_motion d 16, vectors + 5 planes {tag}", motion(pairs, 16, 31, mv, st))
            del mv, st, sc
            torch.cuda.empty_cache()
        if with_torch:
            for m in (1, 8):
                pairs = [(i, (i + 1) % n) for i in range(m)]
                for rnd in range(2):
                    tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                    row(("torch", content, form, m), f"yardstick  torch shifted |s - r| pooled {tag}", lambda: torch_motion(P, ctx, pairs, w, h, 16), 1)
                    row(("mv8", content, form, m), f"frames_motion d 16, vectors + sad      {tag}", lambda: ctx.frames_motion(pairs, 16))
                ours = ctx.frames_motion(pairs, 16)
                theirs = torch_motion(P, ctx, pairs, w, h, 16)
                tr, tc = theirs[1].shape[1] - 1, theirs[1].shape[2]           # (the last whole row reaches coded rows frames_scaled does not give)
                same = bool((ours[0][:, :, :tr, :tc] == theirs[0][:, :, :tr]).all()) and bool((ours[1][:, 0, :tr, :tc] == theirs[1][:, :tr]).all())
                say(f"   the torch formulation's vectors and SADs equal frames_motion's on the first {tr} x {tc} macroblocks: {same}")

    measure("decoded", "tiles", True)
    assert ctx.memory_usage()["raster_pool"] == 0
    # the other distances, on the decoded tiles
    for d, m in ((8, n), (32, n), (64, min(n, 64))):
        pairs = [(i, (i + 1) % n) for i in range(m)]
        mv = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
        for rnd in range(2):
            row(("d", d), f"frames_motion d {d}, vectors            decoded, tiles, {m} jobs, round {rnd}", motion(pairs, d, (), mv, None), 2)
        del mv
    ctx.frames_to_raster(0, n)
    ctx.sync()
    measure("decoded", "raster", False)
    some = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
    for i in range(n):
        ctx.upload_frame(i, some[i % 4])
    measure("noise", "raster", False)
    for i in range(n):
        ctx.upload_frame(i, some[0])
    measure("identical", "raster", False)
    del some
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("noise", "raster"), ("identical", "raster")):
            k = (content, form, m)
            say(f"{content:9s} {form:7s} vectors {mean(('mv',) + k):10.4f} ms   / frames_ssim scores {mean(('mv',) + k) / mean(('ssim',) + k):7.2f}   "
                f"with 5 planes / vectors {mean(('all',) + k) / mean(('mv',) + k):6.3f}   "
                f"spread of vectors between the rounds {abs(times[('mv',) + k][0] - times[('mv',) + k][1]) / mean(('mv',) + k) * 100:5.1f} %")
    for m in (1, 8):
        k = ("decoded", "tiles", m)
        say(f"torch formulation / frames_motion, {m} job{'s' if m > 1 else ''}: {mean(('torch',) + k) / mean(('mv8',) + k):8.1f}")
    say("--- the model: wave-instructions of v_qsad_pk_u16_u8 = macroblocks * candidates * 64 / 4 / 64 lanes")
    for d, key, m in ((8, ("d", 8), n), (16, ("mv", "decoded", "tiles", n), n), (32, ("d", 32), n), (64, ("d", 64), min(n, 64))):
        items = ((2 * d + 3) // 4) * ((2 * d + 3) // 4)
        qsad = m * nmb * items * 256 / 64                                    # an item is 4 x 4 candidates: 256 instructions a lane
        say(f"d {d:2d}: {m} jobs, {mean(key):10.4f} ms, {qsad / 1e6:9.1f} M wave-instructions, {qsad / mean(key) / 1e6:8.2f} G wave-instructions/s")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
