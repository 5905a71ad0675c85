"""Dev aid (GPU): the sub-pixel refinement of block motion at 1920x1080 (8160 macroblocks a pair) over 1 job and over a batch (1024),
at precision 4 and 2, with vectors alone and with all four planes, and, in the same process, what it is held against, which is not
the code under test:
  frames_motion d = 16, vectors   -- the first call of the two-call recipe, over the same jobs;
  the torch formulation of the same eleven evaluations, for scale: frames_scaled of both pictures, the reference picture padded by
      replication, the 49 bilinear predictions of the 7 x 7 quarter-pel positions around the zero vector with the variance of each
      pooled over the macroblocks, and the four decisions as gathers; over 1 and 8 jobs.
The pictures come in three contents: kf_1920x1080's decoded key frames -- as the tiles a large launch leaves and, after
vp8hip_frames_to_raster, as raster --, uniform noise and identical pictures (uploaded: raster).  The sides of a comparison alternate
over two rounds, and both rounds are printed: their difference is the spread.  Device events around each call after warm-up.  The
last lines put the call's rate beside the byte model: both coded lumas read once.
   python3 tools/subpel_time.py [frames (1024)] [timed calls (5)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_subpel(P, ctx, pairs, w, h, precision=4):
    """the formulation frames_subpel replaces: -> (mv int16 [n, 2, rows, cols] in 1/8 pel, value int64 [n, rows, cols]) over the
    macroblock rows and columns the display size covers whole, zero start, no cost"""
    rows, cols = h // 16, w // 16
    s = P.split_i420(ctx.frames_scaled([p[0] for p in pairs]), w, h)[0][:, :16 * rows, :16 * cols].long()
    r = P.split_i420(ctx.frames_scaled([p[1] for p in pairs]), w, h)[0].float()[:, None]
    r = torch.nn.functional.pad(r, (1, 2, 1, 2), mode="replicate")[:, 0].long()
    n = s.shape[0]
    maps = []
    for vy in range(-6, 7, 2):
        for vx in range(-6, 7, 2):
            by, bx, oy, ox = vy >> 3, vx >> 3, vy & 7, vx & 7
            win = r[:, 1 + by:1 + by + 16 * rows + 1, 1 + bx:1 + bx + 16 * cols + 1]
            hp = (win[:, :, :-1] * (128 - 16 * ox) + win[:, :, 1:] * (16 * ox) + 64) >> 7
            d = s - ((hp[:, :-1] * (128 - 16 * oy) + hp[:, 1:] * (16 * oy) + 64) >> 7)
            d = d.view(n, rows, 16, cols, 16)
            sse, sm = (d * d).sum((2, 4)), d.sum((2, 4))
            maps.append(sse - ((sm * sm) >> 8))
    maps = torch.stack(maps, -1)                                 # [n, rows, cols, 49]

    def at(vy, vx):
        return torch.gather(maps, 3, (((vy + 6) >> 1) * 7 + ((vx + 6) >> 1))[..., None])[..., 0]
    zero = torch.zeros((n, rows, cols), dtype=torch.long, device=s.device)
    by_, bx_, best = zero, zero, at(zero, zero)
    for hstep in (4, 2)[:1 if precision == 2 else 2]:
        cy, cx = by_, bx_
        four = [(cy, cx - hstep), (cy, cx + hstep), (cy - hstep, cx), (cy + hstep, cx)]
        vals = [at(*c) for c in four]
        dy = torch.where(vals[2] < vals[3], cy - hstep, cy + hstep)
        dx = torch.where(vals[0] < vals[1], cx - hstep, cx + hstep)
        for (vy, vx), v in zip(four + [(dy, dx)], vals + [at(dy, dx)]):
            less = v < best
            best, by_, bx_ = torch.where(less, v, best), torch.where(less, vy, by_), torch.where(less, vx, bx_)
    return torch.stack((bx_, by_), 1).short(), best


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

    def subpel(pairs, start, precision, planes, mv, st):
        return lambda: ctx.frames_subpel(pairs, start=start, precision=precision, planes=planes, out_mv=mv, out_stats=st if planes else None)

    def measure(content, form, with_torch):
        for m in (1, n):
            pairs = [(i, (i + 1) % n) for i in range(m)]
            whole = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
            mv = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
            st = torch.empty((m, 4, rows, cols), dtype=torch.int32, device="cuda:0")
            for rnd in range(2):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                row(("motion", content, form, m), f"yardstick  frames_motion d 16, vectors     {tag}", lambda: ctx.frames_motion(pairs, 16, planes=(), out_mv=whole))
                row(("p4", content, form, m), f"frames_subpel precision 4, vectors     {tag}", subpel(pairs, whole, 4, (), mv, st))
                row(("p4all", content, form, m), f"frames_subpel precision 4, + 4 planes  {tag}", subpel(pairs, whole, 4, 15, mv, st))
                row(("p2", content, form, m), f"frames_subpel precision 2, vectors     {tag}", subpel(pairs, whole, 2, (), mv, st))
                row(("p4zero", content, form, m), f"frames_subpel precision 4, no start    {tag}", subpel(pairs, None, 4, (), mv, st))
            del whole, mv, st
            torch.cuda.empty_cache()
        if with_torch:
            for m in (1, 8):
                pairs = [(i, (i + 1) % n) for i in range(m)]
                for rnd in range(2):
                    tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                    row(("torch", content, form, m), f"yardstick  torch 49 predictions, gathers {tag}", lambda: torch_subpel(P, ctx, pairs, w, h), 1)
                    row(("p4val", content, form, m), f"frames_subpel precision 4, vectors + val {tag}", lambda: ctx.frames_subpel(pairs))
                ours = ctx.frames_subpel(pairs)
                theirs = torch_subpel(P, ctx, pairs, w, h)
                tr, tc = theirs[1].shape[1], theirs[1].shape[2]
                same = bool((ours[0][:, :, :tr, :tc] == theirs[0]).all()) and bool((ours[1][:, 0, :tr, :tc].long() == theirs[1]).all())
                say(f"   the torch formulation's vectors and values equal frames_subpel's on the first {tr} x {tc} macroblocks: {same}")

    measure("decoded", "tiles", True)
    assert ctx.memory_usage()["raster_pool"] == 0
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
    luma_bytes = 2 * 16 * cols * 16 * rows
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds; the byte model: both coded lumas read once, {luma_bytes} bytes a pair")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("noise", "raster"), ("identical", "raster")):
            k = (content, form, m)
            p4 = mean(("p4",) + k)
            say(f"{content:9s} {form:7s} precision 4 {p4:9.4f} ms   / frames_motion d 16 {p4 / mean(('motion',) + k):6.3f}   "
                f"with 4 planes / vectors {mean(('p4all',) + k) / p4:6.3f}   precision 2 / 4 {mean(('p2',) + k) / p4:6.3f}   "
                f"no start / start {mean(('p4zero',) + k) / p4:6.3f}   {m * luma_bytes / p4 / 1e9:8.3f} TB/s   "
                f"spread between the rounds {abs(times[('p4',) + k][0] - times[('p4',) + k][1]) / p4 * 100:5.1f} %")
    for m in (1, 8):
        k = ("decoded", "tiles", m)
        say(f"torch formulation / frames_subpel, {m} job{'s' if m > 1 else ''}: {mean(('torch',) + k) / mean(('p4val',) + k):8.1f}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
