"""Dev aid (GPU): the byte histograms at 1920x1080 over 1 job and over a batch (1024), and, in the same process, the yardsticks they
are held against, which are not the code under test:
  frames_hist (Y|U|V, single frames and pairs)  beside  frames_scaled of the same frames at the display size -- the copy that moves the
      same bytes in -- and the torch formulation the call replaces: frames_scaled, then per plane
      (x.long() + 256 * frame).flatten().bincount(minlength=256 * n);
  slots_hist (seven planes)                     beside  frames_side at the native grid (vectors and six planes);
  trace_wear_hist (four planes)                 beside  trace_wear U8 with all planes at the display size.
Same-address LDS atomics are the risk, so the pictures come in three contents: kf_1920x1080's decoded key frames -- as the tiles a
large launch leaves and, after vp8hip_frames_to_raster, as raster --, uniform noise and a flat picture (uploaded: raster); the wear
pool in two: random counters and zeros.  The sides of a comparison alternate over two rounds, and both rounds are printed: their
difference is the spread.  Device events around each call after warm-up.
   python3 tools/hist_time.py [frames (1024)] [timed calls (10)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_hist(P, ctx, fbs, w, h):
    """the formulation frames_hist replaces: -> int64 [3][256 * n]"""
    n = len(fbs)
    frame = 256 * torch.arange(n, device="cuda:0")[:, None]
    return [(x.flatten(1).long() + frame).flatten().bincount(minlength=256 * n) for x in P.split_i420(ctx.frames_scaled(fbs), w, h)]


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
        ms = timed(fn, 2, reps if r is None else r)
        times.setdefault(key, []).append(ms)
        say(f"{what:74s} {ms:9.4f} ms per call, {in_bytes / ms / 1e9:7.3f} TB/s of bytes read")

    def mean(key):
        return sum(times[key]) / len(times[key])

    # ---- pictures ----
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
    rng = np.random.default_rng(7)
    g = ctx.g

    def measure(content, form):
        for m in (1, n):
            fbs = list(range(m))
            pairs = [(i, (i + 1) % n) for i in range(m)]
            hout = torch.empty((m, 3, 256), dtype=torch.int32, device="cuda:0")
            sout = torch.empty((m, pic), dtype=torch.uint8, device="cuda:0")
            for rnd in range(2):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                row(("scaled", content, form, m), f"yardstick  frames_scaled   {tag}", lambda: ctx.frames_scaled(fbs, out=sout), pic * m)
                row(("hist", content, form, m), f"frames_hist single         {tag}", lambda: ctx.frames_hist(fbs, out=hout), pic * m)
                row(("pair", content, form, m), f"frames_hist pairs          {tag}", lambda: ctx.frames_hist(pairs, out=hout), 2 * pic * m)
                row(("torch", content, form, m), f"yardstick  torch bincount  {tag}", lambda: torch_hist(P, ctx, fbs, w, h), pic * m, 2)
            want = torch.stack(torch_hist(P, ctx, fbs, w, h)).view(3, m, 256).transpose(0, 1)
            assert torch.equal(ctx.frames_hist(fbs).long(), want), (content, form, m)      # (the two sides count the same)
            del hout, sout, want
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
    some = [np.full(g.frame_size, v, np.uint8) for v in (128, 16, 128, 235)]
    for i in range(n):
        ctx.upload_frame(i, some[i % 4])
    measure("flat", "raster")
    del some
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("noise", "raster"), ("flat", "raster")):
            k = (content, form, m)
            say(f"{content:8s} {form:7s} frames_hist / frames_scaled {mean(('hist',) + k) / mean(('scaled',) + k):6.3f}   "
                f"pairs / single {mean(('pair',) + k) / mean(('hist',) + k):6.3f}   torch / frames_hist {mean(('torch',) + k) / mean(('hist',) + k):7.2f}   "
                f"spread of frames_hist between the rounds {abs(times[('hist',) + k][0] - times[('hist',) + k][1]) / mean(('hist',) + k) * 100:5.1f} %")
        say(f"flat / noise, frames_hist from raster: {mean(('hist', 'flat', 'raster', m)) / mean(('hist', 'noise', 'raster', m)):6.3f}")

    # ---- slots and wear entries ----
    w, h, frames = P.read_ivf(ivf_path("p_dense_1920x1080"))
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, 1, n)
    parser = P.Parser()
    k = min(4, n, len(frames))
    for i, data in enumerate(frames[:k]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
    parser.close()
    for i in range(k, n):
        ctx.ir_copy(i, i % k)
    ctx.sync()
    nmb = ctx.nmb
    say(f"p_dense_1920x1080 (a key frame and {k - 1} inter frames) x {n} slots")
    for m in (1, n):
        slots = [(i + 1) % n for i in range(m)]                              # (one job: an inter frame)
        hout = torch.empty((m, 7, 256), dtype=torch.int32, device="cuda:0")
        mv = torch.empty((m, 2, 4 * ctx.g.aligned_h // 16, 4 * ctx.g.aligned_w // 16), dtype=torch.int16, device="cuda:0")
        info = torch.empty((m, 6) + tuple(mv.shape[2:]), dtype=torch.uint8, device="cuda:0")
        for rnd in range(2):
            tag = f"{m} job{'s' if m > 1 else ''}, round {rnd}"
            row(("side", m), f"yardstick  frames_side native grid, vectors and six planes, {tag}",
                lambda: ctx.frames_side(slots, planes=63, out_mv=mv, out_info=info), nmb * 128 * m)
            row(("slots", m), f"slots_hist seven planes, {tag}", lambda: ctx.slots_hist(slots, 127, out=hout), nmb * 128 * m)
        say(f"slots_hist / frames_side, {m} job{'s' if m > 1 else ''}: {mean(('slots', m)) / mean(('side', m)):6.3f}")
        del hout, mv, info
    pool = ctx.wear_pool(n)
    some = torch.from_numpy(rng.integers(0, 256, (4, h, w, 4)).astype(np.uint8)).to("cuda:0")
    for content in ("random counters", "zeros"):
        for i in range(n):
            pool[i] = some[i % 4]
        for m in (1, n):
            idx = list(range(m))
            hout = torch.empty((m, 4, 256), dtype=torch.int32, device="cuda:0")
            tout = torch.empty((m, 4, h, w), dtype=torch.uint8, device="cuda:0")
            for rnd in range(2):
                tag = f"{content}, {m} job{'s' if m > 1 else ''}, round {rnd}"
                row(("wear", content, m), f"yardstick  trace_wear U8 four planes, {tag}", lambda: ctx.trace_wear(pool, idx, out=tout), 4 * w * h * m)
                row(("whist", content, m), f"trace_wear_hist four planes, {tag}", lambda: ctx.trace_wear_hist(pool, idx, out=hout), 4 * w * h * m)
            say(f"trace_wear_hist / trace_wear, {content}, {m} job{'s' if m > 1 else ''}: {mean(('whist', content, m)) / mean(('wear', content, m)):6.3f}")
            want = torch.stack([tout[:, c].flatten(1).long().add_(256 * torch.arange(m, device="cuda:0")[:, None]).flatten().bincount(minlength=256 * m)
                                for c in range(4)]).view(4, m, 256).transpose(0, 1)
            assert torch.equal(hout.long(), want), (content, m)
            del hout, tout, want
            torch.cuda.empty_cache()
        some.zero_()
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
