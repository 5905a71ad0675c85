"""Dev aid (GPU): the structural similarity of picture pairs at 1920x1080 over 1 job and over a batch (1024), and, in the same process,
what it is held against, which is not the code under test:
  frames_ssim, scores only        -- the reduction alone;
  frames_ssim, scores and F32 map -- plus a store per window;
  frames_hist in pair mode        -- over the same jobs: it reads the same bytes and makes no division;
  the torch formulation the call replaces, for scale: frames_scaled of both pictures, then per plane the five pooled moments
      (avg_pool2d 8x8, stride 4, of s, r, s*s, r*r, s*r in float32) and similarity() in float -- not the reference's integers.
The pictures come in three contents: kf_1920x1080's decoded key frames -- as the tiles a large launch leaves and, after
vp8hip_frames_to_raster, as raster --, uniform noise and identical pictures (uploaded: raster).  The sides of a comparison alternate
over two rounds, and both rounds are printed: their difference is the spread.  Device events around each call after warm-up.
   python3 tools/ssim_time.py [frames (1024)] [timed calls (10)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_ssim(P, ctx, pairs, w, h, chunk=64):
    """the formulation frames_ssim replaces: -> float32 [n, 3], the mean over vp8_ssim2's windows of a float similarity()"""
    pool = torch.nn.functional.avg_pool2d
    out = []
    for i0 in range(0, len(pairs), chunk):
        part = pairs[i0:i0 + chunk]
        a = P.split_i420(ctx.frames_scaled([p[0] for p in part]), w, h)
        b = P.split_i420(ctx.frames_scaled([p[1] for p in part]), w, h)
        means = []
        for s, r in zip(a, b):
            nwx, nwy = P.ssim_windows(s.shape[2], s.shape[1])
            s, r = s.float()[:, None], r.float()[:, None]
            ms, mr, mss, mrr, msr = (pool(x, 8, 4)[:, 0, :nwy, :nwx] * 64 for x in (s, r, s * s, r * r, s * r))
            n = (2 * ms * mr + 26634) * (2 * 64 * msr - 2 * ms * mr + 239708)
            d = (ms * ms + mr * mr + 26634) * (64 * mss - ms * ms + 64 * mrr - mr * mr + 239708)
            means.append((n / d).flatten(1).mean(1))
        out.append(torch.stack(means, 1))
    return torch.cat(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 1024
    reps = int(args[1]) if len(args) > 1 else 10
    P = load_package()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    times = {}

    def row(key, what, fn, in_bytes, r=None):
        ms = timed(fn, 2 if r is None else 1, reps if r is None else r)
        times.setdefault(key, []).append(ms)
        say(f"{what:78s} {ms:9.4f} ms per call, {in_bytes / ms / 1e9:7.3f} TB/s of bytes read")

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
    say(f"kf_1920x1080 x {n} frame buffers; {reps} timed calls after 2 (the torch formulation: 2 after 1); memory {ctx.memory_usage()}")
    pic = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    elems = P.ssim_sizes(w, h, 7, "float32")[1] // 4
    say(f"windows a pair: {elems}; workgroups a job at 1 job: {ctx.ssim_share(1)}, at {n}: {ctx.ssim_share(n)}")
    rng = np.random.default_rng(7)
    g = ctx.g

    def measure(content, form):
        for m in (1, n):
            pairs = [(i, (i + 1) % n) for i in range(m)]
            sc = torch.empty((m, 3, 2), dtype=torch.int64, device="cuda:0")
            mp = torch.empty((m, elems), dtype=torch.float32, device="cuda:0")
            hout = torch.empty((m, 3, 256), dtype=torch.int32, device="cuda:0")
            for rnd in range(2):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                row(("pair", content, form, m), f"yardstick  frames_hist pairs  {tag}", lambda: ctx.frames_hist(pairs, out=hout), 2 * pic * m)
                row(("scores", content, form, m), f"frames_ssim scores            {tag}", lambda: ctx.frames_ssim(pairs, out_scores=sc), 2 * pic * m)
                row(("map", content, form, m), f"frames_ssim scores + F32 map  {tag}",
                    lambda: ctx.frames_ssim(pairs, 7, torch.float32, out_scores=sc, out_map=mp), 2 * pic * m)
                row(("torch", content, form, m), f"yardstick  torch pooled float {tag}", lambda: torch_ssim(P, ctx, pairs, w, h), 2 * pic * m, 2)
            ours = torch.from_numpy(P.ssim_mean(ctx.frames_ssim(pairs))).to("cuda:0")
            theirs = torch_ssim(P, ctx, pairs, w, h).double()
            say(f"   largest |frames_ssim mean - float formulation| over {m} job{'s' if m > 1 else ''}: {float((ours - theirs).abs().max()):.3e}")
            del sc, mp, hout
            torch.cuda.empty_cache()

    measure("decoded", "tiles")
    assert ctx.memory_usage()["raster_pool"] == 0
    ctx.frames_to_raster(0, n)
    ctx.sync()
    measure("decoded", "raster")
    some = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
    for i in range(n):
        ctx.upload_frame(i, some[i % 4])
    measure("noise", "raster")
    for i in range(n):
        ctx.upload_frame(i, some[0])
    measure("identical", "raster")
    del some
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("noise", "raster"), ("identical", "raster")):
            k = (content, form, m)
            say(f"{content:9s} {form:7s} scores / frames_hist pairs {mean(('scores',) + k) / mean(('pair',) + k):6.3f}   "
                f"with map / scores {mean(('map',) + k) / mean(('scores',) + k):6.3f}   torch / scores {mean(('torch',) + k) / mean(('scores',) + k):7.2f}   "
                f"spread of scores between the rounds {abs(times[('scores',) + k][0] - times[('scores',) + k][1]) / mean(('scores',) + k) * 100:5.1f} %")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
