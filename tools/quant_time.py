"""Dev aid (GPU): transform and quantisation of the motion-compensated residual at 1920x1080 (8160 macroblocks a picture) over 1 job
and over a batch (256): levels alone, every output, every output but the inverse side's (no rec, no RECSSE), both quantisers, with
frames_subpel's own vectors and with none, and, in the same process, what it is held against, which is not the code under test:
  frames_tfilter with ONE source and the same vectors -- the same prediction work: the difference is what the block phase costs;
  frames_coef (levels, Y U V Y2, int16) over as many IR slots -- the same output volume;
  the torch formulation of the forward steps with no vectors and the fast quantiser: frames_scaled of both pictures, the residual,
      both DCT passes and the Walsh transform as integer tensor arithmetic on [blocks, 4, 4], the quantiser as sixteen masked
      steps; over 1 job.
The pictures come in three contents: kf_1920x1080's decoded key frames -- as the tiles a large launch leaves and, after
vp8hip_frames_to_raster, as raster --, uniform noise (uploaded: raster), and identical pictures (job i against itself).  Job i takes
frame buffer i against frame buffer i + 1 (mod the pool).  The order inside a round is A B B A over (the call, the yardsticks), two
rounds, both printed (--out keeps their means and the spread between them).  Device events around each call after warm-up.  The last lines put the call
beside the byte floor: 1.5 bytes a coded pixel read twice (source and reference) plus the outputs written.
   python3 tools/quant_time.py [jobs (256)] [timed calls (5)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)


def torch_quant(P, ctx, fb, ref, w, h, q):
    """the forward steps as tensor arithmetic, no vectors, fast quantiser: -> levels int64 [rows, cols, 25, 16] over the macroblocks
    wholly inside the display size"""
    rows, cols = h // 16, w // 16
    f = P.quant_factors(q)
    s = P.split_i420(ctx.frames_scaled([fb]), w, h)
    r = P.split_i420(ctx.frames_scaled([ref]), w, h)
    blocks = []
    for pl, g in ((0, 4), (1, 2), (2, 2)):
        n = 4 * g
        d = s[pl][0, :n * rows, :n * cols].long() - r[pl][0, :n * rows, :n * cols].long()
        blocks.append(d.reshape(rows, g, 4, cols, g, 4).permute(0, 3, 1, 4, 2, 5).reshape(rows, cols, g * g, 4, 4))
    d = torch.cat(blocks, 2)                                                  # [rows, cols, 24, 4 (row), 4 (col)]
    a, b, c, e = (d[..., 0] + d[..., 3]) * 8, (d[..., 1] + d[..., 2]) * 8, (d[..., 1] - d[..., 2]) * 8, (d[..., 0] - d[..., 3]) * 8
    t = torch.stack([a + b, (c * 2217 + e * 5352 + 14500) >> 12, a - b, (e * 2217 - c * 5352 + 7500) >> 12], -1)
    a, b, c, e = t[..., 0, :] + t[..., 3, :], t[..., 1, :] + t[..., 2, :], t[..., 1, :] - t[..., 2, :], t[..., 0, :] - t[..., 3, :]
    co = torch.stack([(a + b + 7) >> 4, ((c * 2217 + e * 5352 + 12000) >> 16) + (e != 0), (a - b + 7) >> 4, (e * 2217 - c * 5352 + 51000) >> 16], -2)
    dc = co[:, :, :16, 0, 0].reshape(rows, cols, 4, 4)
    a, e, c, b = (dc[..., 0] + dc[..., 2]) * 4, (dc[..., 1] + dc[..., 3]) * 4, (dc[..., 1] - dc[..., 3]) * 4, (dc[..., 0] - dc[..., 2]) * 4
    t = torch.stack([a + e + (a != 0), b + c, b - c, a - e], -1)
    a, e, c, b = t[..., 0, :] + t[..., 2, :], t[..., 1, :] + t[..., 3, :], t[..., 1, :] - t[..., 3, :], t[..., 0, :] - t[..., 2, :]
    y2 = torch.stack([((x + (x < 0)) + 3) >> 3 for x in (a + e, b + c, b - c, a - e)], -2)
    co = torch.cat([co.reshape(rows, cols, 24, 16), y2.reshape(rows, cols, 1, 16)], 2)
    table = [0] * 16 + [2] * 8 + [1]
    ac = [0] + [1] * 15
    rnd = torch.tensor([[int(f["round"][t][k]) for k in ac] for t in table], device=co.device)
    qf = torch.tensor([[int(f["quant_fast"][t][k]) for k in ac] for t in table], device=co.device)
    y = ((co.abs() + rnd) * qf) >> 16
    return torch.where(co < 0, -y, y)


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
        print(f"{what:100s} {ms:10.4f} ms per call", flush=True)          # (every round on the terminal; --out keeps the means and the spread)
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
    planes = ("erry", "erry2", "erruv", "eobs", "recsse")
    csize, esize, ssize, rsize = P.quant_sizes(w, h, planes)
    q = 40

    def measure(content, form, with_torch):
        for m in (1, n):
            jobs = [(i, i if content == "same" else (i + 1) % n) for i in range(m)]
            pairs = jobs
            tjobs = [(i, i, 1) for i in range(m)]
            coef = torch.empty((m, rows, cols, 25, 16), dtype=torch.int16, device="cuda:0")
            eob = torch.empty((m, rows, cols, 32), dtype=torch.uint8, device="cuda:0")
            st5 = torch.empty((m, 5, rows, cols), dtype=torch.int32, device="cuda:0")
            st4 = torch.empty((m, 4, rows, cols), dtype=torch.int32, device="cuda:0")
            rec = torch.empty((m, rsize), dtype=torch.uint8, device="cuda:0")
            pic = torch.empty((m, rsize), dtype=torch.uint8, device="cuda:0")
            whole = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
            own = torch.empty((m, 2, rows, cols), dtype=torch.int16, device="cuda:0")
            ctx.frames_motion(pairs, 16, planes=(), out_mv=whole)
            ctx.frames_subpel(pairs, start=whole, planes=(), out_mv=own)
            k = (content, form, m)

            def ours(rd):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rd}"
                for name, mv in (("own", own), ("none", None)):
                    row(("levels", name) + k, f"frames_quant regular, levels alone, vectors {name:5s}              {tag}",
                        lambda: ctx.frames_quant(jobs, mv, q, want=(), out_coef=coef))
                    row(("forward", name) + k, f"frames_quant regular, coef + eob + 4 planes (no inverse), {name:5s} {tag}",
                        lambda: ctx.frames_quant(jobs, mv, q, planes=planes[:4], want=(), out_coef=coef, out_eob=eob, out_stats=st4))
                    row(("all", name) + k, f"frames_quant regular, every output, vectors {name:5s}              {tag}",
                        lambda: ctx.frames_quant(jobs, mv, q, planes=planes, want=(), out_coef=coef, out_eob=eob, out_stats=st5, out_rec=rec))
                row(("fast", "own") + k, f"frames_quant fast,    every output, vectors own                {tag}",
                    lambda: ctx.frames_quant(jobs, own, q, quantizer="fast", planes=planes, want=(), out_coef=coef, out_eob=eob, out_stats=st5, out_rec=rec))
                row(("rec", "own") + k, f"frames_quant regular, rec alone, vectors own                   {tag}",
                    lambda: ctx.frames_quant(jobs, own, q, want=(), out_rec=rec))

            def yardsticks(rd):
                tag = f"{content}, {form}, {m} job{'s' if m > 1 else ''}, round {rd}"
                for name, mv in (("own", own), ("none", None)):
                    row(("tfilter", name) + k, f"yardstick  frames_tfilter, one source, vectors {name:5s}           {tag}",
                        lambda: ctx.frames_tfilter(tjobs, pairs, mv, None, 3, "sixtap", out=pic))
                if content == "decoded":
                    row(("coef",) + k, f"yardstick  frames_coef levels, Y U V Y2, int16                 {tag}",
                        lambda: ctx.frames_coef(list(range(m)), "levels", planes=("y", "u", "v", "y2")))
            for rd in range(2):                          # A B B A
                (ours if rd == 0 else yardsticks)(rd)
                (yardsticks if rd == 0 else ours)(rd)
            if with_torch and m == 1:
                for rd in range(2):
                    row(("torch",), f"yardstick  torch forward steps, fast, no vectors, 1 job        {content}, {form}, round {rd}",
                        lambda: torch_quant(P, ctx, jobs[0][0], jobs[0][1], w, h, q), 1)
                    row(("ours",), f"frames_quant fast, levels alone, no vectors, 1 job             {content}, {form}, round {rd}",
                        lambda: ctx.frames_quant(jobs, None, q, quantizer="fast", want=(), out_coef=coef))
                mine = ctx.frames_quant(jobs, None, q, quantizer="fast", want=("coef",))["coef"][0, :h // 16].long()
                say(f"   the torch formulation's levels equal frames_quant's on the macroblock rows compared: "
                    f"{bool((mine == torch_quant(P, ctx, jobs[0][0], jobs[0][1], w, h, q)).all())}")
            del coef, eob, st5, st4, rec, pic, whole, own
            torch.cuda.empty_cache()

    measure("decoded", "tiles", True)
    assert ctx.memory_usage()["raster_pool"] == 0
    ctx.frames_to_raster(0, n)
    ctx.sync()
    measure("decoded", "raster", False)
    measure("same", "raster", False)
    some = [rng.integers(0, 256, g.frame_size, dtype=np.uint8) for _ in range(4)]
    for i in range(n):
        ctx.upload_frame(i, some[i % 4])
    measure("noise", "raster", False)
    del some
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    pixels = 16 * cols * 16 * rows
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds, ms a call; the byte floor: 1.5 B a coded pixel read twice + the outputs "
            f"written ({csize} coef, {esize} eob, {ssize} stats, {rsize} rec a job), at the 6.29 TB/s a float4 copy reaches")
        for content, form in (("decoded", "tiles"), ("decoded", "raster"), ("same", "raster"), ("noise", "raster")):
            k = (content, form, m)
            allo, lev, fwd, tf = mean(("all", "own") + k), mean(("levels", "own") + k), mean(("forward", "own") + k), mean(("tfilter", "own") + k)
            moved = m * (3.0 * pixels + csize + esize + ssize + rsize)
            say(f"{content:8s} {form:6s}: own vectors: levels {lev:9.4f} forward {fwd:9.4f} every output {allo:9.4f} fast {mean(('fast', 'own') + k):9.4f} "
                f"rec alone {mean(('rec', 'own') + k):9.4f} | no vectors: levels {mean(('levels', 'none') + k):9.4f} every output "
                f"{mean(('all', 'none') + k):9.4f} | frames_tfilter one source {tf:9.4f} (none {mean(('tfilter', 'none') + k):9.4f}): every output / it "
                f"{allo / tf:6.3f}, levels / it {lev / tf:6.3f}" + (f" | frames_coef {mean(('coef',) + k):9.4f}" if ("coef",) + k in times else "") +
                f" | byte floor {moved / 6.29e12 * 1e3:8.4f} ms, every output {moved / allo / 1e9:6.3f} TB/s | spread "
                f"{abs(times[('all', 'own') + k][0] - times[('all', 'own') + k][1]) / allo * 100:5.1f} %")
    say(f"torch formulation / frames_quant, 1 job, forward steps, fast, no vectors: {mean(('torch',)) / mean(('ours',)):8.1f}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
