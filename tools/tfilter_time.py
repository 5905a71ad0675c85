"""Dev aid (GPU): the motion-compensated temporal filter at 1920x1080 (8160 macroblocks a picture) over 1 job and over a batch (256),
with 3, 7 and 15 sources a job, six-tap and bilinear, with no vectors (every plane copied), whole-pixel vectors, sub-pixel vectors
and frames_subpel's own vectors and errors, and, in the same process, what it is held against, which is not the code under test:
  frames_subpel precision 4, vectors + val  -- over the very pairs the jobs take (and frames_motion d = 16 in front of it);
  the torch formulation of the same filter, bilinear: frames_scaled of every picture, each source's three planes padded by
      replication, a gather per tap per plane per source at the per-pixel expansion of the macroblock vectors, the blend and the
      normalisation; over 1 job of 3 sources.
The pictures come in three contents: kf_1920x1080's decoded key frames -- as the tiles a large launch leaves and, after
vp8hip_frames_to_raster, as raster -- and uniform noise (uploaded: raster).  Job i filters frame buffer i over frame buffers i, i + 1,
.. (mod the pool).  The sides alternate over two rounds, and both rounds are printed: their difference is the spread.  Device events
around each call after warm-up.  The last lines put the call's rate beside the byte model: 1.5 bytes a pixel read per source, 1.5
written per job (the count plane, 3 more, where it is asked for).
   python3 tools/tfilter_time.py [jobs (256)] [timed calls (5)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_tfilter(P, ctx, fb, refs, mv, err, w, h, strength=3, thresh=(10000, 20000)):
    """the formulation frames_tfilter replaces, bilinear, one job: -> (picture uint8 [i420_size], count int32 [i420_size]) over the
    display size (a multiple of 16 each way is assumed for the expansion of the vectors; 1080 is cropped to 1072 rows)"""
    rows, cols = h // 16, w // 16
    hh, ww = 16 * rows, 16 * cols
    dev = mv.device
    centre = [p[0, :hh >> s, :ww >> s].long() for p, s in zip(P.split_i420(ctx.frames_scaled([fb]), w, h), (0, 1, 1))]
    acc = [torch.zeros_like(c) for c in centre]
    cnt = [torch.zeros_like(c) for c in centre]
    rnd = (1 << (strength - 1)) if strength else 0
    for k, ref in enumerate(refs):
        e = err[k].reshape(err.shape[-2], err.shape[-1])[:rows, :cols].long() & 0xffffffff
        wgt = torch.where(e < thresh[0], 2, torch.where(e < thresh[1], 1, 0))
        src = P.split_i420(ctx.frames_scaled([ref]), w, h)
        for pl in range(3):
            n, s = (16, 0) if pl == 0 else (8, 1)
            vx, vy = mv[k, 0, :rows, :cols].long() >> s, mv[k, 1, :rows, :cols].long() >> s
            up = lambda t: t.repeat_interleave(n, 0).repeat_interleave(n, 1)
            ph, pw = hh >> s, ww >> s
            plane = src[pl][0].long()
            yy = torch.arange(ph, device=dev)[:, None] + up(vy >> 3)
            xx = torch.arange(pw, device=dev)[None, :] + up(vx >> 3)
            oy, ox = up(vy & 7), up(vx & 7)

            def at(y, x):
                return plane[y.clamp(0, plane.shape[0] - 1), x.clamp(0, plane.shape[1] - 1)]
            top = (at(yy, xx) * (128 - 16 * ox) + at(yy, xx + 1) * (16 * ox) + 64) >> 7
            bot = (at(yy + 1, xx) * (128 - 16 * ox) + at(yy + 1, xx + 1) * (16 * ox) + 64) >> 7
            q = (top * (128 - 16 * oy) + bot * (16 * oy) + 64) >> 7
            d = centre[pl] - q
            m = (16 - ((d * d * 3 + rnd) >> strength).clamp(max=16)) * up(wgt)
            cnt[pl] += m
            acc[pl] += m * q
    out = [(((a + (c >> 1)) * torch.where(c > 0, 0x80000 // c.clamp(min=1), 0)) >> 19) & 0xff for a, c in zip(acc, cnt)]
    return out, cnt


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 256
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
        say(f"{what:96s} {ms:10.4f} ms per call")
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
    say(f"kf_1920x1080 x {n} frame buffers, {rows * cols} macroblocks a picture; {reps} timed calls after 1 (the torch formulation: 1 after 1); "
        f"memory {ctx.memory_usage()}")
    rng = np.random.default_rng(7)
    g = ctx.g
    size = P.tfilter_sizes(w, h)[0]
    COUNTS = (3, 7, 15)

    def measure(content, form, with_torch):
        for m in (1, n):
            out = torch.empty((m, size), dtype=torch.uint8, device="cuda:0")
            out_count = torch.empty((m, size), dtype=torch.int16, device="cuda:0")
            for S in COUNTS:
                pairs = [(i, (i + s) % n) for i in range(m) for s in range(S)]
                jobs = [(i, i * S, S) for i in range(m)]
                np_ = len(pairs)
                whole = torch.empty((np_, 2, rows, cols), dtype=torch.int16, device="cuda:0")
                own = torch.empty((np_, 2, rows, cols), dtype=torch.int16, device="cuda:0")
                val = torch.empty((np_, 1, rows, cols), dtype=torch.int32, device="cuda:0")
                ctx.frames_motion(pairs, 16, planes=(), out_mv=whole)
                ctx.frames_subpel(pairs, start=whole, planes=("val",), out_mv=own, out_stats=val)
                rnd8 = torch.from_numpy(rng.integers(-64, 65, (np_, 2, rows, cols), dtype=np.int16)).to("cuda:0")
                vectors = {"none": None, "whole": (rnd8 >> 3) << 3, "subpel": rnd8, "own": own}
                for rd in range(2):
                    tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''} x {S}, round {rd}"
                    k = (content, form, m, S)
                    row(("motion",) + k, f"yardstick  frames_motion d 16, vectors            {tag}", lambda: ctx.frames_motion(pairs, 16, planes=(), out_mv=whole))
                    row(("subpel",) + k, f"yardstick  frames_subpel precision 4, vectors + val {tag}",
                        lambda: ctx.frames_subpel(pairs, start=whole, planes=("val",), out_mv=own, out_stats=val))
                    for filt in ("sixtap", "bilinear"):
                        for name, mv in vectors.items():
                            err = val if name == "own" else None
                            row((filt, name) + k, f"frames_tfilter {filt:8s} vectors {name:6s}             {tag}",
                                lambda: ctx.frames_tfilter(jobs, pairs, mv, err, 3, filt, out=out))
                    row(("counted",) + k, f"frames_tfilter sixtap   vectors own, + count        {tag}",
                        lambda: ctx.frames_tfilter(jobs, pairs, own, val, 3, "sixtap", out=out, out_count=out_count))
                if with_torch and m == 1 and S == 3:
                    for rd in range(2):
                        row(("torch",), f"yardstick  torch bilinear, gathers, 1 job x 3        {content}, {form}, round {rd}",
                            lambda: torch_tfilter(P, ctx, 0, [p[1] for p in pairs], own, val, w, h), 1)
                        row(("ours",), f"frames_tfilter bilinear vectors own, + count         {content}, {form}, round {rd}",
                            lambda: ctx.frames_tfilter(jobs, pairs, own, val, 3, "bilinear", want_count=True))
                    ours = ctx.frames_tfilter(jobs, pairs, own, val, 3, "bilinear", want_count=True)
                    theirs = torch_tfilter(P, ctx, 0, [p[1] for p in pairs], own, val, w, h)
                    hh, ww = 16 * (h // 16), 16 * (w // 16)
                    same = True
                    for a, c, mine, cmine, s in zip(theirs[0], theirs[1], P.split_i420(ours[0], w, h), P.split_i420(ours[1], w, h), (0, 1, 1)):
                        # (a source's window may reach past the rows the expansion covers: the last macroblock row is left out)
                        rr = (hh >> s) - (16 >> s)
                        same &= bool((mine[0, :rr, :ww >> s].long() == a[:rr]).all()) and bool((cmine[0, :rr, :ww >> s].long() == c[:rr]).all())
                    say(f"   the torch formulation's picture and count equal frames_tfilter's on the rows compared: {same}")
                del whole, own, val, rnd8, vectors
                torch.cuda.empty_cache()
            del out, out_count
            torch.cuda.empty_cache()

    measure("decoded", "tiles", True)
    assert ctx.memory_usage()["raster_pool"] == 0
    ctx.frames_to_raster(0, n)
    ctx.sync()
    measure("decoded", "raster", False)
    some = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
    for i in range(n):
        ctx.upload_frame(i, some[i % 4])
    measure("noise", "raster", False)
    del some
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    pixels = 16 * cols * 16 * rows
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds; the byte model: 1.5 B a coded pixel per source read + {size} B written a job; "
            f"the HBM rate it is held against: 6.29 TB/s (a float4 copy)")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("noise", "raster")):
            for S in COUNTS:
                k = (content, form, m, S)
                moved = m * (1.5 * pixels * S + size)
                floor = moved / 6.29e12 * 1e3
                six, bil = mean(("sixtap", "own") + k), mean(("bilinear", "own") + k)
                say(f"{content:8s} {form:6s} x {S:2d}: sixtap none {mean(('sixtap', 'none') + k):9.4f} whole {mean(('sixtap', 'whole') + k):9.4f} "
                    f"subpel {mean(('sixtap', 'subpel') + k):9.4f} own {six:9.4f} (+ count {mean(('counted',) + k):9.4f}) | bilinear subpel "
                    f"{mean(('bilinear', 'subpel') + k):9.4f} own {bil:9.4f} ms | byte floor {floor:8.4f} ms, sixtap own {moved / six / 1e9:6.3f} TB/s | "
                    f"/ frames_subpel {six / mean(('subpel',) + k):6.3f} (subpel {mean(('subpel',) + k):9.4f}, motion {mean(('motion',) + k):9.4f} ms) | "
                    f"spread {abs(times[('sixtap', 'own') + k][0] - times[('sixtap', 'own') + k][1]) / six * 100:5.1f} %")
    say(f"torch formulation / frames_tfilter, 1 job x 3 sources, bilinear: {mean(('torch',)) / mean(('ours',)):8.1f}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
